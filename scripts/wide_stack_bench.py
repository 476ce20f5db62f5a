"""Times the stacked 2-NN of a wide query against a whole wide train collection (fm_collection_wide_knn, K14 over the stack)
against its floor and against the route the commit before it had, alternating the cases in one process, with option
"f32_filter" 2 (the fp16 matrix-core filter forced on for all three):

    stacked   fm_collection_wide_knn(q, collection, 2): ONE sweep over the stack, the stage table read per tile
    bank      fm_knn2(q, bank of the images' rows concatenated): the same arithmetic without table or padding -- the floor
    each      fm_collection_wide_knn2_each(q, collection) plus the merge of its [n_images][nq][2] lists on the host (NumPy:
              keys (distance bits << 32 | global row), the two smallest per query row) -- the only route there was

Two times per case, both from the library's own HIP events: `*_ms` is the kernel bracket (fm_stats.kernel_ms of one call) and
`*_call_ms` the whole call (fm_stats.total_ms: every kernel and the copy of the lists to the host) -- the interval to compare
across cases; `each_merge_ms` is the host merge behind `each` (wall clock), which the other two do not need.  Warm-up calls of
every case come first; the cases alternate inside every repetition, so drift of the clock or of a shared host hits all of them
alike.  Before any timing the three results are compared bit for bit.  `padding_share` is the part of the stack's physical
rows that is padding (what `stacked` sweeps, or skips, and `bank` does not have); `filter_stats` is fm_f32_filter_stats'
(launches, fallbacks) over the timed calls: a fallback means a record list overflowed and the exact kernel redid the call.
One JSON line on stdout.

    python scripts/wide_stack_bench.py [--images 1000] [--rows 1000] [--jitter 100] [--nq 2048] [--dim 256] [--reps 10] [--warmup 2]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fastmatch_amd                      # noqa: E402


def _times_ms(ctx, fn):
    """(kernel bracket, whole call) of one call, both from the library's HIP events"""
    ctx.reset_stats()
    fn()
    st = ctx.stats()
    return float(st["kernel_ms"]), float(st["total_ms"])


def _unit_rows(rng, n, dim):
    """Unit-norm rows on a 16-D subspace plus noise: learned descriptors are L2-normalised and far from isotropic."""
    B = rng.standard_normal((16, dim))
    a = (rng.standard_normal((n, 16)) @ B + 0.05 * rng.standard_normal((n, dim))).astype(np.float32)
    return (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)


def _merge_each(idx, dist, first):
    """The stacked top-2 from per-image lists [n_images, nq, 2]: (global row [nq, 2], dist [nq, 2])"""
    keys = (dist.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (idx.astype(np.int64) + first[:-1, None, None]).astype(np.uint64)
    keys[idx < 0] = np.uint64(0xFFFFFFFFFFFFFFFF)
    keys = np.ascontiguousarray(keys.transpose(1, 0, 2)).reshape(idx.shape[1], -1)
    two = np.sort(np.partition(keys, 1, axis=1)[:, :2], axis=1)
    g = (two & np.uint64(0xFFFFFFFF)).astype(np.int64)
    d = (two >> np.uint64(32)).astype(np.uint32).view(np.float32)
    return g, d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1000)
    ap.add_argument("--rows", type=int, default=1000, help="rows per image, on average")
    ap.add_argument("--jitter", type=int, default=100, help="image sizes are drawn from rows - jitter .. rows + jitter")
    ap.add_argument("--nq", type=int, default=2048)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    ctx = fastmatch_amd.Context(0)
    ctx.set_option("f32_filter", 2)
    rng = np.random.default_rng(17)
    sizes = rng.integers(max(a.rows - a.jitter, 1), a.rows + a.jitter + 1, a.images)
    first = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    T = _unit_rows(rng, int(first[-1]), a.dim)
    Q = (T[rng.integers(0, len(T), a.nq)] + 0.02 / np.sqrt(a.dim) * rng.standard_normal((a.nq, a.dim))).astype(np.float32)
    qb, tb, coll = ctx.bank(Q), ctx.bank(T), ctx.collection()
    for i in range(a.images):
        coll.add_wide(T[first[i]:first[i + 1]])
    coll.train()
    physical = int(((sizes + 127) // 128 * 128).sum())
    rec = {"images": a.images, "rows_total": int(first[-1]), "rows_physical": physical, "padding_share": 1.0 - float(first[-1]) / physical,
           "nq": a.nq, "dim": a.dim, "reps": a.reps, "device": ctx.device_name()}

    # the three routes give the same lists, bit for bit
    img, idx, dist = coll.wide_knn(qb, 2)
    g = first[img] + idx
    bi, bd = ctx.knn2(qb, tb)
    if not (np.array_equal(g, bi) and np.array_equal(dist.view(np.uint32), bd.view(np.uint32))):
        raise SystemExit("stacked differs from fm_knn2 on the concatenated rows")
    eg, ed = _merge_each(*coll.wide_knn2_each(qb), first)
    if not (np.array_equal(g, eg) and np.array_equal(dist.view(np.uint32), ed.view(np.uint32))):
        raise SystemExit("stacked differs from the merged per-image lists")

    each_out = []
    cases = [("stacked", lambda: coll.wide_knn(qb, 2)), ("bank", lambda: ctx.knn2(qb, tb)),
             ("each", lambda: each_out.append(coll.wide_knn2_each(qb)))]
    for _ in range(a.warmup):
        for _, fn in cases:
            fn()
    each_out.clear()
    times = {name: [] for name, _ in cases}
    calls = {name: [] for name, _ in cases}
    merge = []
    l0, f0 = ctx.f32_filter_stats()
    for _ in range(a.reps):
        for name, fn in cases:
            k_ms, c_ms = _times_ms(ctx, fn)
            times[name].append(k_ms)
            calls[name].append(c_ms)
        t0 = time.perf_counter()
        _merge_each(*each_out.pop(), first)
        merge.append(1e3 * (time.perf_counter() - t0))
    l1, f1 = ctx.f32_filter_stats()
    rec["filter_stats"] = [l1 - l0, f1 - f0]
    for name, t in times.items():
        rec[name + "_ms"] = float(np.median(t))
        rec[name + "_min_ms"] = float(min(t))
        rec[name + "_max_ms"] = float(max(t))
        rec[name + "_call_ms"] = float(np.median(calls[name]))
        rec[name + "_call_min_ms"] = float(min(calls[name]))
        rec[name + "_call_max_ms"] = float(max(calls[name]))
    rec["each_merge_ms"] = float(np.median(merge))
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
