"""Hamming radiusMatch (fm_hamming_radius_match, radius_ham_kernel) against its two comparators, in one process:
  pair        100k x 100k binary rows of 32 bytes, clustered (below); a radius for ~2 entries per query row and one for ~50,
              read off the NumPy reference of a 2 000-row query sample
  collection  10k queries against a train collection of 100 images x 1 000 rows, the ~2 radius
  (a) fm_knn2 on the same binary banks (K11: the same MFMAs, a heavier epilogue)
  (b) fm_radius_match, counts only, on 100k x 100k uint8 128-D rows at ~2 entries per row (K10's integer sweep: the same
      MFMA count per tile)
Per case: wall time of whole synchronous calls -- the counts-only call (cap = 0: limits, count sweep, scan) and the sized
call (+ fill sweep, sort, compaction, copies) -- and the count sweep's kernel time from the library's own events
(fm_stats kernel_ms).  One warm-up, `reps` repeats, median and (min, max) of each.  One JSON line per case.
The fill sweep's kernel time is not bracketed by events of its own: a `rocprofv3 --kernel-trace --stats` run of this script
lists radius_ham_kernel<true, 2> beside radius_ham_kernel<false, 2>.
  python scripts/gpu_hamming_radius.py [reps] [rows]

Data: the tests' clustered recipe (tests/hamming_radius_ref.py) -- a row is a random base row with k of {0, 1, 2, 5, 17, 40}
random bits flipped -- with one base per 40 rows, so that the neighbourhoods stay as dense as in the tests at any size."""
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
from fastmatch_amd import synth                           # noqa: E402
import hamming_ref                                        # noqa: E402
import hamming_radius_ref as HR                           # noqa: E402

NBYTES = 32


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


def _raw(ctx, fn, handles, r, cap, offs, lists):
    tot = ctypes.c_int64(0)
    ptrs = [a.ctypes.data if a is not None else None for a in lists]
    ctx._check(getattr(ctx.lib, fn)(ctx.handle, *handles, None, float(r), int(cap), offs.ctypes.data, *ptrs, ctypes.byref(tot)))
    return tot.value


def _radii_for(Q, T, targets, sample=2000):
    """Per target: (r = H + 0.5, mean list size of a query sample at h <= H), the H whose mean is closest to the target --
    from the NumPy reference."""
    rng = np.random.default_rng(4)
    rows = rng.choice(len(Q), min(sample, len(Q)), replace=False)
    h = hamming_ref.distances(Q[rows], T)
    mean = np.cumsum(np.bincount(h.reshape(-1), minlength=8 * NBYTES + 1)) / len(rows)       # mean entries at h <= H
    return [(int(np.argmin(np.abs(mean - t))) + 0.5, float(mean[int(np.argmin(np.abs(mean - t)))])) for t in targets]


def _case(ctx, name, fn, handles, nq, nt, r, reps, with_img, extra):
    offs = np.zeros(nq + 1, np.int64)
    none = [None] * (3 if with_img else 2)
    n = _raw(ctx, fn, handles, r, 0, offs, none)
    lists = [np.empty(max(n, 1), np.int32) for _ in range(len(none) - 1)] + [np.empty(max(n, 1), np.float32)]
    cw, ck = _timed(ctx, lambda: _raw(ctx, fn, handles, r, 0, offs, none), reps)
    sw, _ = _timed(ctx, lambda: _raw(ctx, fn, handles, r, n, offs, lists), reps)
    out = {"case": name, "call": fn, "nq": nq, "nt": nt, "bytes": NBYTES, "r": r, "entries": n, "entries_per_row": n / max(nq, 1),
           "reps": reps, "counts_ms": cw, "count_sweep_kernel_ms": ck, "sized_ms": sw}
    out.update(extra)
    out["device"] = ctx.device_name()
    print(json.dumps(out), flush=True)
    return out


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 100000
    ctx = fastmatch_amd.Context(0)
    rng = np.random.default_rng(77)
    base = rng.integers(0, 256, (max(HR.NBASE, n // 40), NBYTES), dtype=np.uint8)
    Q, T = HR.clustered(n, NBYTES, rng, base), HR.clustered(n, NBYTES, rng, base)
    (r2, m2), (r50, m50) = _radii_for(Q, T, (2.0, 50.0))
    qb, tb = ctx.bank_binary(Q), ctx.bank_binary(T)
    kw, kk = _timed(ctx, lambda: ctx.knn2(qb, tb), reps)                     # comparator (a)
    a = {"knn2_ms": kw, "knn2_kernel_ms": kk, "splits": HR.sweep_splits(n, n)}
    for name, r, m in (("pair_2", r2, m2), ("pair_50", r50, m50)):
        o = _case(ctx, name, "fm_hamming_radius_match", [qb.handle, tb.handle], n, n, r, reps, False, dict(a, sample_mean=m))
        print(json.dumps({"case": name + "_vs_knn2", "count_sweep_kernel_over_knn2_kernel": o["count_sweep_kernel_ms"][0] / max(kk[0], 1e-9),
                          "counts_over_knn2_wall": o["counts_ms"][0] / kw[0], "sized_over_knn2_wall": o["sized_ms"][0] / kw[0]}), flush=True)
    # the collection: 100 images x n / 100 rows, n / 10 queries
    per, nqc = max(1, n // 100), max(1, n // 10)
    qc = ctx.bank_binary(Q[:nqc])
    with ctx.collection() as c:
        for i in range(100):
            c.add_binary(T[i * per:(i + 1) * per])
        c.train()
        _case(ctx, "collection_2", "fm_collection_hamming_radius_match", [c.handle, qc.handle], nqc, 100 * per, r2, reps, True,
              {"images": 100, "rows_per_image": per, "splits": HR.sweep_splits(nqc, 100 * ((per + 127) // 128 * 128))})
    qc.close()
    qb.close()
    tb.close()
    # comparator (b): K10's integer sweep, counts only, ~2 entries per row (scripts/gpu_radius_match.py's pair and radius)
    Q8, T8, _ = synth.planted_pair(n, n, seed=1)
    q8, t8 = ctx.bank(Q8), ctx.bank(T8)
    _, kdist = ctx.knn2(q8, t8)
    r8 = float(np.float32(np.median(kdist[:, 1]) * 1.0005))
    offs = np.zeros(n + 1, np.int64)
    n8 = _raw(ctx, "fm_radius_match", [q8.handle, t8.handle], r8, 0, offs, [None, None])
    bw, bk = _timed(ctx, lambda: _raw(ctx, "fm_radius_match", [q8.handle, t8.handle], r8, 0, offs, [None, None]), reps)
    print(json.dumps({"case": "l2_i8_counts", "call": "fm_radius_match", "nq": n, "nt": n, "r": r8, "entries_per_row": n8 / n, "reps": reps,
                      "counts_ms": bw, "count_sweep_kernel_ms": bk, "device": ctx.device_name()}), flush=True)
    q8.close()
    t8.close()
    ctx.close()


if __name__ == "__main__":
    main()
