"""Wide radiusMatch (fm_wide_radius_match: radius_wide_kernel, radius_wide_rescore_kernel) against its yardstick, in one process:
  pair      nq = 10 000 queries against nt = 1 000 000 rows of clustered unit-norm data (tests/wide_ref.py's recipe: a 16-D
            subspace plus noise, every query a near copy of a train row), at 256 and at 160 values per row; a radius that
            gives on the order of ten entries per query row, found by bisection with counts-only calls on the first 512 queries
  yardstick fm_knn2 on the same two banks: the same fp16 planes and the same K steps, ONE sweep with a running bound.  The radius
            call makes TWO sweeps (count, fill) plus the exact rescoring, a scan and a segment sort.
Per dim: wall time of whole synchronous calls -- the counts-only call (cap = 0: limits, count sweep, scan) and the sized call
(+ fill sweep, rescoring, sort, compaction, copies) -- and the count sweep's kernel time from the library's own events
(fm_stats kernel_ms); the same two figures for fm_knn2.  One warm-up, `reps` repeats, median and (min, max) of each.  One JSON
line per case and one with the ratios.
  python scripts/gpu_wide_radius.py [reps] [nt] [nq]"""
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fastmatch_amd                                      # noqa: E402
import wide_ref                                           # noqa: E402


def _timed(ctx, f, reps):
    """(wall ms [median, min, max], kernel ms [median, min, max]) of f over reps calls after one warm-up."""
    f()
    wall, kern = [], []
    for _ in range(reps):
        ctx.reset_stats()
        t0 = time.perf_counter()
        f()
        wall.append(1e3 * (time.perf_counter() - t0))
        kern.append(ctx.stats()["kernel_ms"])
    return [[float(np.median(x)), float(np.min(x)), float(np.max(x))] for x in (wall, kern)]


def _raw(ctx, qb, tb, r, cap, offs, idx, dist):
    tot = ctypes.c_int64(0)
    ctx._check(ctx.lib.fm_wide_radius_match(ctx.handle, qb.handle, tb.handle, None, float(r), int(cap), offs.ctypes.data,
                                            idx.ctypes.data if idx is not None else None,
                                            dist.ctypes.data if dist is not None else None, ctypes.byref(tot)))
    return tot.value


def _radius_for(ctx, Q, tb, target, rows=512):
    """The radius whose mean list size over the first `rows` queries is closest to `target` from above: bisection in (0, 2)."""
    qs = ctx.bank(np.ascontiguousarray(Q[:rows]))
    offs = np.zeros(qs.n + 1, np.int64)
    lo, hi = 0.0, 2.0
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        if _raw(ctx, qs, tb, mid, 0, offs, None, None) / qs.n >= target:
            hi = mid
        else:
            lo = mid
    qs.close()
    return float(np.float32(hi))


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    nt = int(sys.argv[2]) if len(sys.argv) > 2 else 1000000
    nq = int(sys.argv[3]) if len(sys.argv) > 3 else 10000
    ctx = fastmatch_amd.Context(0)
    for dim in (256, 160):
        Q, T = wide_ref.clustered(nq, nt, dim, 9)
        qb, tb = ctx.bank(Q), ctx.bank(T)
        del T
        r = _radius_for(ctx, Q, tb, 10.0)
        offs = np.zeros(nq + 1, np.int64)
        l0 = ctx.f32_filter_stats()
        n = _raw(ctx, qb, tb, r, 0, offs, None, None)
        assert ctx.f32_filter_stats()[0] == l0[0] + 1              # the fp16 sweep, not the all-pairs path
        idx, dist = np.empty(max(n, 1), np.int32), np.empty(max(n, 1), np.float32)
        cw, ck = _timed(ctx, lambda: _raw(ctx, qb, tb, r, 0, offs, None, None), reps)
        sw, _ = _timed(ctx, lambda: _raw(ctx, qb, tb, r, n, offs, idx, dist), reps)
        l1 = ctx.f32_filter_stats()
        kw, kk = _timed(ctx, lambda: ctx.knn2(qb, tb), reps)
        l2 = ctx.f32_filter_stats()
        out = {"case": "wide_radius_pair", "dim": dim, "nq": nq, "nt": nt, "r": r, "entries": n, "entries_per_row": n / nq, "reps": reps,
               "counts_ms": cw, "count_sweep_kernel_ms": ck, "sized_ms": sw, "knn2_ms": kw, "knn2_kernel_ms": kk,
               "knn2_filter_launches": l2[0] - l1[0], "knn2_fallbacks": l2[1] - l1[1], "device": ctx.device_name()}
        print(json.dumps(out), flush=True)
        print(json.dumps({"case": "wide_radius_vs_knn2", "dim": dim, "counts_over_knn2_wall": cw[0] / kw[0], "sized_over_knn2_wall": sw[0] / kw[0],
                          "count_sweep_kernel_over_knn2_kernel": ck[0] / max(kk[0], 1e-9)}), flush=True)
        qb.close()
        tb.close()
    ctx.close()


if __name__ == "__main__":
    main()
