"""K11b (NORM_HAMMING2) beside K11 (NORM_HAMMING) on the SAME rows, in one process: the 2-NN sweep (fm_knn2) on 100k x 100k
random rows of 32 and 64 bytes, the two norms interleaved call by call -- H2, H, H2, H, ... -- so that whatever else the host or
the device is doing falls on both alike.  Kernel ms per call from fm_get_stats (the HIP events round the sweep), after a warm-up
of each; median (min - max) per norm, the ratio of the medians, and the K-step ratio it is to be read against (3 : 2 at 32
bytes, 6 : 4 at 64).  fm_xcheck1 (the top-1 sweep) the same way.  One JSON line per case and call.
  python scripts/gpu_hamming2.py [reps] [rows]"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fastmatch_amd                                      # noqa: E402


def _one(ctx, f):
    ctx.reset_stats()
    f()
    return ctx.stats()["kernel_ms"]


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 100000
    ctx = fastmatch_amd.Context(0)
    rng = np.random.default_rng(1)
    for width in (32, 64):
        Q = rng.integers(0, 256, (n, width), dtype=np.uint8)
        T = rng.integers(0, 256, (n, width), dtype=np.uint8)
        q2, t2 = ctx.bank_binary2(Q), ctx.bank_binary2(T)
        q1, t1 = ctx.bank_binary(Q), ctx.bank_binary(T)
        ks2, ks1 = (12 * width + 127) // 128, (width + 15) // 16
        for call, f2, f1 in (("knn2", lambda: ctx.knn2(q2, t2), lambda: ctx.knn2(q1, t1)),
                             ("xcheck1", lambda: ctx.xcheck1(q2, t2), lambda: ctx.xcheck1(q1, t1))):
            f2(); f1()                                      # warm-up: code objects, workspaces
            ms2, ms1 = [], []
            for _ in range(reps):
                ms2.append(_one(ctx, f2))
                ms1.append(_one(ctx, f1))
            m2, m1 = float(np.median(ms2)), float(np.median(ms1))
            print(json.dumps({"bytes": width, "call": call, "n": n, "reps": reps,
                              "hamming2_ms": m2, "hamming2_min": min(ms2), "hamming2_max": max(ms2),
                              "hamming_ms": m1, "hamming_min": min(ms1), "hamming_max": max(ms1),
                              "ratio": m2 / m1, "ksteps": [ks2, ks1], "kstep_ratio": ks2 / ks1,
                              "device": ctx.device_name()}), flush=True)
        for b in (q2, t2, q1, t1):
            b.close()
    ctx.close()


if __name__ == "__main__":
    main()
