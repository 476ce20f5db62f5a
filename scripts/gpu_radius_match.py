"""K10 (fm_radius_match) against the box's own yardsticks, in one process:
  integer route  100k x 100k uint8 rows, r set for ~2 entries per query row   vs K1 (fm_knn2) on the same pair
  float32 route  10k queries x 1M non-integer rows, r for ~2 entries per row     vs K8 (fm_knn2, 2-NN) on the same pair
Wall time of whole synchronous calls (median of reps): the counts-only call (cap = 0: sweep + scan), the sized call
(sweep, scan, fill sweep, sort, compaction, copies) and ctx.radius_match (both).  One JSON line per route.
  python scripts/gpu_radius_match.py [reps]"""
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fastmatch_amd                                      # noqa: E402
from fastmatch_amd import synth                           # noqa: E402


def _med(f, reps):
    f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts))


def _raw(ctx, qb, tb, r, cap, offs, idx, dist):
    tot = ctypes.c_int64(0)
    ctx._check(ctx.lib.fm_radius_match(ctx.handle, qb.handle, tb.handle, None, float(r), int(cap), offs.ctypes.data,
                                       idx.ctypes.data if idx is not None else None,
                                       dist.ctypes.data if dist is not None else None, ctypes.byref(tot)))
    return tot.value


def run(ctx, name, Q, T, reps):
    qb, tb = ctx.bank(Q), ctx.bank(T)
    kidx, kdist = ctx.knn2(qb, tb)
    # ~2 entries per row on average: the radius between the 2nd and 3rd neighbour of a typical row
    r = float(np.float32(np.median(kdist[:, 1]) * 1.0005))
    offs = np.zeros(qb.n + 1, np.int64)
    n = _raw(ctx, qb, tb, r, 0, offs, None, None)
    idx, dist = np.empty(max(n, 1), np.int32), np.empty(max(n, 1), np.float32)
    out = {
        "route": name, "nq": qb.n, "nt": tb.n, "r": r, "entries": n, "entries_per_row": n / qb.n,
        "knn2_ms": _med(lambda: ctx.knn2(qb, tb), reps),
        "radius_counts_ms": _med(lambda: _raw(ctx, qb, tb, r, 0, offs, None, None), reps),
        "radius_sized_ms": _med(lambda: _raw(ctx, qb, tb, r, n, offs, idx, dist), reps),
        "radius_match_py_ms": _med(lambda: ctx.radius_match(qb, tb, r), reps),
    }
    out["sized_over_knn2"] = out["radius_sized_ms"] / out["knn2_ms"]
    out["device"] = ctx.device_name()
    qb.close()
    tb.close()
    print(json.dumps(out), flush=True)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    ctx = fastmatch_amd.Context(0)
    Q, T, _ = synth.planted_pair(100000, 100000, seed=1)
    run(ctx, "i8", Q, T, reps)
    rng = np.random.default_rng(2)
    Q, T, _ = synth.planted_pair(10000, 1000000, seed=3)
    Q = Q.astype(np.float32) / 512.0 + rng.random(Q.shape, dtype=np.float32) * 1e-3
    T = T.astype(np.float32) / 512.0 + rng.random(T.shape, dtype=np.float32) * 1e-3
    run(ctx, "f32", Q, T, reps)
    ctx.close()


if __name__ == "__main__":
    main()
