"""Train collections against the ways to get the same numbers without them (one MI355X, one process, same data):
  * Collection.knn2_each          vs a loop of Context.knn2(q, bank_i) over resident banks,
  * Collection.knn(q, 2) (stacked) vs Context.knn2 on one bank of the same rows concatenated on the host.
Wall time around synchronous calls after warm-up, median of --reps repetitions; both answers are compared before timing.
    python scripts/gpu_collection.py [--reps 15]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import fastmatch_amd                          # noqa: E402
from fastmatch_amd import synth               # noqa: E402


def median_ms(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(np.min(t)), float(np.max(t))


def case(ctx, n_images, rows, nq, reps, seed):
    rng = np.random.default_rng(seed)
    T = synth.synth_sift(n_images * rows, rng)
    Q = synth.synth_sift(nq, rng)
    images = [T[rows * i:rows * (i + 1)] for i in range(n_images)]
    qb = ctx.bank(Q)
    for bk in [ctx.bank(im) for im in images[:8]]:          # warm-up of the upload path
        bk.close()
    t0 = time.perf_counter()
    banks = [ctx.bank(im) for im in images]
    ctx.sync()
    t_banks = (time.perf_counter() - t0) * 1e3
    whole = ctx.bank(T)
    t0 = time.perf_counter()
    coll = ctx.collection()
    for im in images:
        coll.add(im)
    coll.train()
    ctx.sync()
    t_coll = (time.perf_counter() - t0) * 1e3
    build = (t_banks, t_coll)

    def loop():
        return [ctx.knn2(qb, b) for b in banks]

    ref = loop()
    idx, dist = coll.knn2_each(qb)
    assert all(np.array_equal(idx[i], r[0]) and np.array_equal(dist[i].view(np.uint32), r[1].view(np.uint32))
               for i, r in enumerate(ref)), "knn2_each differs from the loop"
    widx, wdist = ctx.knn2(qb, whole)
    img, lidx, ldist = coll.knn(qb, 2)
    assert np.array_equal(img.astype(np.int64) * rows + lidx, widx) and np.array_equal(ldist.view(np.uint32), wdist.view(np.uint32))
    pad = coll_rows_padded(rows) * n_images
    print("case %d images x %d rows (%d rows, %d with padding: +%.1f %%) vs %d query rows" %
          (n_images, rows, n_images * rows, pad, 100.0 * (pad - n_images * rows) / (n_images * rows), nq))
    print("  build, once: %d fm_bank_create_u8 calls %.1f ms; collection create + %d adds + train %.1f ms" %
          (n_images, build[0], n_images, build[1]))
    a = median_ms(loop, reps)
    b = median_ms(lambda: coll.knn2_each(qb), reps)
    print("  knn2 loop over %d resident banks : median %.3f ms (min %.3f, max %.3f)" % ((n_images,) + a))
    print("  Collection.knn2_each              : median %.3f ms (min %.3f, max %.3f)  -> %.2f x the loop's speed" % (b + (a[0] / b[0],)))
    v = median_ms(lambda: coll.votes(qb, 0.8, 1), reps)
    print("  Collection.votes(mode 1)          : median %.3f ms (min %.3f, max %.3f)  (no [n_images][nq][2] copy out)" % v)
    c = median_ms(lambda: ctx.knn2(qb, whole), reps)
    d = median_ms(lambda: coll.knn(qb, 2), reps)
    print("  knn2 on one concatenated bank     : median %.3f ms (min %.3f, max %.3f)" % c)
    print("  Collection.knn(k = 2), stacked    : median %.3f ms (min %.3f, max %.3f)  -> overhead %+.1f %%" % (d + (100.0 * (d[0] / c[0] - 1.0),)))
    coll.close(); whole.close(); qb.close()
    for bk in banks:
        bk.close()


def coll_rows_padded(rows):
    return (rows + 127) // 128 * 128


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    args = ap.parse_args()
    print("command: python scripts/gpu_collection.py --reps %d" % args.reps)
    ctx = fastmatch_amd.Context(0)
    print("device:", ctx.device_name())
    case(ctx, 500, 2000, 10000, args.reps, 1)
    case(ctx, 1000, 500, 2000, args.reps, 2)


if __name__ == "__main__":
    main()
