"""K11 (NORM_HAMMING on binary banks) beside its yardsticks, in one process: fm_xcheck1 and fm_knn2 on 100k x 100k ORB-32 and
BRISK-64 rows, the same calls on 100k x 100k SIFT-like uint8 rows (K1), and the k = 3 vector-ALU kernel on the ORB shape (the
popcount baseline).  Kernel ms per call from fm_get_stats (median of reps), pairs/s, and the fraction of the FP4 peak (10 PF
dense: a pair costs 2 * 8 * bytes_padded FLOP on the matrix cores).  One JSON line per case.
  python scripts/gpu_hamming.py [reps]"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fastmatch_amd                                      # noqa: E402
from fastmatch_amd import synth                           # noqa: E402

FP4_PEAK = 10.0e15


def _kernel_ms(ctx, f, reps):
    f()
    ms = []
    for _ in range(reps):
        ctx.reset_stats()
        f()
        ms.append(ctx.stats()["kernel_ms"])
    return float(np.median(ms))


def run(ctx, name, qb, tb, reps, bits=None):
    pairs = qb.n * tb.n
    for call, f in (("xcheck1", lambda: ctx.xcheck1(qb, tb)), ("knn2", lambda: ctx.knn2(qb, tb)),
                    ("knn3", lambda: ctx.knn(qb, tb, 3))):
        if call == "knn3" and bits is None:
            continue
        ms = _kernel_ms(ctx, f, reps)
        out = {"case": name, "call": call, "nq": qb.n, "nt": tb.n, "kernel_ms": ms, "pairs_per_s": pairs / (ms * 1e-3)}
        if bits is not None and call != "knn3":
            out["fp4_peak_fraction"] = pairs * 2.0 * bits / (ms * 1e-3) / FP4_PEAK
        out["device"] = ctx.device_name()
        print(json.dumps(out), flush=True)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    ctx = fastmatch_amd.Context(0)
    rng = np.random.default_rng(1)
    n = 100000
    for name, width in (("orb32", 32), ("brisk64", 64)):
        Q = rng.integers(0, 256, (n, width), dtype=np.uint8)
        T = rng.integers(0, 256, (n, width), dtype=np.uint8)
        qb, tb = ctx.bank_binary(Q), ctx.bank_binary(T)
        run(ctx, name, qb, tb, reps, bits=8 * ((width + 15) // 16 * 16))
        qb.close(); tb.close()
    Q, T, _ = synth.planted_pair(n, n, seed=1)
    qb, tb = ctx.bank(Q), ctx.bank(T)
    run(ctx, "sift_u8", qb, tb, reps)
    qb.close(); tb.close()
    ctx.close()


if __name__ == "__main__":
    main()
