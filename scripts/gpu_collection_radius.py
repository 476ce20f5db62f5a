"""K10 against a train collection: ONE stacked radius query (fm_collection_radius_match) against the only other way to the
same answer -- a loop of fm_radius_match over one bank per image plus the host merge of the per-image lists.
  10 000 query rows x 100 images of 10 000 rows, one radius per query row set for ~10 hits per row (just above the row's
  8th neighbour in the collection), on the integer route (uint8 rows) and the float32 route (non-integer float32 rows).
Wall time of whole synchronous calls, one warm-up, then `reps` repetitions: median [min .. max].  The stacked lists are
checked against the merged ones before anything is timed.  Also timed: the device form through torchmatch (radii from a
CUDA tensor, lists left in CUDA tensors).  One JSON line per route.
  python scripts/gpu_collection_radius.py [reps] [images] [rows per image] [query rows]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fastmatch_amd                                      # noqa: E402
from fastmatch_amd import synth, torchmatch               # noqa: E402


def _timed(f, reps):
    f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append(1e3 * (time.perf_counter() - t0))
    return {"median_ms": float(np.median(ts)), "min_ms": float(np.min(ts)), "max_ms": float(np.max(ts))}


def _loop(ctx, qb, banks, r):
    """radius_match image by image, then the merge: per query row ascending (distance bits, image, row)."""
    parts = [ctx.radius_match(qb, tb, r) for tb in banks]
    nq = qb.n
    row = np.concatenate([np.repeat(np.arange(nq), np.diff(off)) for off, _, _ in parts])
    img = np.concatenate([np.full(idx.shape[0], i, np.int32) for i, (_, idx, _) in enumerate(parts)])
    idx = np.concatenate([p[1] for p in parts])
    dist = np.concatenate([p[2] for p in parts])
    order = np.lexsort((idx, img, dist.view(np.uint32), row))
    offsets = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=nq))]).astype(np.int64)
    return offsets, img[order], idx[order], dist[order]


def run(ctx, name, Q, images, reps):
    import torch
    f32 = name == "f32"
    qb = ctx.bank(Q, float_route=f32)
    banks = [ctx.bank(im, float_route=f32) for im in images]
    coll = ctx.collection()
    for im in images:
        coll.add(im)
    _, _, d8 = coll.knn(qb, 8)
    r = np.nextafter(d8[:, 7] * np.float32(1.002), np.float32(np.inf)).astype(np.float32)
    stacked, merged = coll.radius_match(qb, r), _loop(ctx, qb, banks, r)
    same = all(np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
               for a, b in zip(stacked, merged))
    r_t = torch.from_numpy(r).cuda()
    tcoll = torchmatch.Collection(context=ctx)
    tcoll._coll = coll                       # (the same resident collection through the tensor front end)

    def dev():
        out = tcoll.radius_match(qb, r_t)
        torch.cuda.synchronize()
        return out
    out = {"route": name, "nq": qb.n, "images": len(images), "rows_per_image": int(images[0].shape[0]),
           "entries": int(stacked[0][-1]), "entries_per_row": float(stacked[0][-1]) / qb.n, "stacked_equals_merged_loop": bool(same),
           "stacked": _timed(lambda: coll.radius_match(qb, r), reps),
           "stacked_device_form": _timed(dev, reps),
           "loop_and_merge": _timed(lambda: _loop(ctx, qb, banks, r), reps),
           "loop_only": _timed(lambda: [ctx.radius_match(qb, tb, r) for tb in banks], reps),
           "device": ctx.device_name()}
    out["loop_over_stacked"] = out["loop_and_merge"]["median_ms"] / out["stacked"]["median_ms"]
    tcoll._coll = None
    coll.close()
    for b in banks:
        b.close()
    qb.close()
    print(json.dumps(out), flush=True)


def main():
    a = [int(x) for x in sys.argv[1:]]
    reps, ni, per, nq = (a + [5, 100, 10000, 10000][len(a):])[:4]
    ctx = fastmatch_amd.Context(0)
    rng = np.random.default_rng(4)
    U = synth.synth_sift(nq + ni * per, rng)
    for name in ("i8", "f32"):
        V = U if name == "i8" else (U.astype(np.float32) / 512.0 + rng.random(U.shape, dtype=np.float32) * 1e-3).astype(np.float32)
        run(ctx, name, V[:nq], [V[nq + i * per: nq + (i + 1) * per] for i in range(ni)], reps)
    ctx.close()


if __name__ == "__main__":
    main()
