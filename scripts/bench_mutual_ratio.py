"""Times fm_mutual_ratio / fm_collection_mutual_ratio_each against the composition they replace (fm_knn2_ratio + fm_xcheck1;
on a collection fm_collection_knn2_each + fm_collection_xcheck1_each), alternating the two in one process.

Every call here ends in a host synchronisation of its own, so wall-clock time around a call, after a sync in front of it,
is device-synchronised host time.  The baseline is timed twice per repetition, before and after the new call: the distance
of the two medians is the run-to-run spread the verdict is held against.  One JSON line per case on stdout.

    python scripts/bench_mutual_ratio.py [--reps 20] [--warmup 3] [--rows 100000]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fastmatch_amd                      # noqa: E402
from fastmatch_amd import synth           # noqa: E402


def _timed(ctx, fn):
    ctx.sync()
    t0 = time.perf_counter()
    out = fn()
    ctx.sync()
    return (time.perf_counter() - t0) * 1e3, out


def _run(ctx, name, new, base, reps, warmup, extra):
    for _ in range(warmup):
        base(); new()
    t_new, t_b0, t_b1 = [], [], []
    for _ in range(reps):
        t_b0.append(_timed(ctx, base)[0])
        t_new.append(_timed(ctx, new)[0])
        t_b1.append(_timed(ctx, base)[0])
    med = lambda x: float(np.median(x))       # noqa: E731
    rec = {"case": name, "reps": reps, "new_ms": med(t_new), "base_ms": med(t_b0 + t_b1), "base_first_ms": med(t_b0),
           "base_second_ms": med(t_b1), "spread_ms": abs(med(t_b0) - med(t_b1)), "new_min_ms": min(t_new),
           "base_min_ms": min(t_b0 + t_b1), "new_iqr_ms": float(np.subtract(*np.percentile(t_new, [75, 25]))),
           "base_iqr_ms": float(np.subtract(*np.percentile(t_b0 + t_b1, [75, 25])))}
    rec.update(extra)
    rec["not_slower"] = bool(rec["new_ms"] <= rec["base_ms"] + max(rec["spread_ms"], rec["base_iqr_ms"]))
    print(json.dumps(rec), flush=True)


def _binary_pair(n, seed, p=0.2, w=32):
    rng = np.random.default_rng(seed)
    T = rng.integers(0, 256, (n, w), dtype=np.uint8)
    Q = rng.integers(0, 256, (n, w), dtype=np.uint8)
    k = int(p * n)
    qs, ts = rng.choice(n, k, replace=False), rng.choice(n, k, replace=False)
    flips = np.zeros((k, w), np.uint8)
    for _ in range(24):                       # 24 of 256 bits flipped (independent rows sit near 128)
        flips[np.arange(k), rng.integers(0, w, k)] ^= (1 << rng.integers(0, 8, k)).astype(np.uint8)
    Q[qs] = T[ts] ^ flips
    return Q, T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--tau", type=float, default=0.8)
    a = ap.parse_args()
    ctx = fastmatch_amd.Context(0)
    tau, n = a.tau, a.rows

    Q, T, _ = synth.planted_pair(n, n, seed=11, p=0.2)
    qb, tb = ctx.bank(Q), ctx.bank(T)
    n_cand = ctx.knn2_ratio(qb, tb, tau)[0].shape[0]
    n_acc = ctx.mutual_ratio(qb, tb, tau)[0].shape[0]
    _run(ctx, "u8 %dx%d" % (n, n), lambda: ctx.mutual_ratio(qb, tb, tau), lambda: (ctx.knn2_ratio(qb, tb, tau), ctx.xcheck1(qb, tb)),
         a.reps, a.warmup, {"n_cand": n_cand, "accepted": n_acc, "device": ctx.device_name()})
    qb.close(); tb.close()

    Q, T = _binary_pair(n, 12)
    qb, tb = ctx.bank_binary(Q), ctx.bank_binary(T)
    n_cand = ctx.knn2_ratio(qb, tb, tau)[0].shape[0]
    n_acc = ctx.mutual_ratio(qb, tb, tau)[0].shape[0]
    _run(ctx, "bin32 %dx%d" % (n, n), lambda: ctx.mutual_ratio(qb, tb, tau), lambda: (ctx.knn2_ratio(qb, tb, tau), ctx.xcheck1(qb, tb)),
         a.reps, a.warmup, {"n_cand": n_cand, "accepted": n_acc})
    qb.close(); tb.close()

    rng = np.random.default_rng(13)
    images = [synth.synth_sift(4096, rng) for _ in range(64)]
    Q = synth.synth_sift(4096, rng)
    for i in range(0, 4096, 4):               # a quarter of the query rows are noisy copies of rows of the first images
        src = images[(i // 4) % 8][i]
        Q[i] = np.clip(src.astype(np.float64) + np.rint(rng.normal(0.0, 6.0, 128)), 0, 255).astype(np.uint8)
    coll = ctx.collection()
    for im in images:
        coll.add(im)
    qb = ctx.bank(Q)
    n_cand = int(coll.votes(qb, tau, 1).sum())
    n_acc = int(coll.mutual_ratio_votes(qb, tau).sum())
    _run(ctx, "collection 64x4096, query 4096", lambda: coll.mutual_ratio_each(qb, tau),
         lambda: (coll.knn2_each(qb), coll.xcheck1_each(qb)), a.reps, a.warmup, {"n_cand": n_cand, "accepted": n_acc})
    _run(ctx, "collection 64x4096, query 4096, counts only", lambda: coll.mutual_ratio_votes(qb, tau),
         lambda: (coll.votes(qb, tau, 1), coll.mutual_votes(qb)), a.reps, a.warmup, {"n_cand": n_cand, "accepted": n_acc})
    qb.close(); coll.close()


if __name__ == "__main__":
    main()
