"""Fast-Match's accepted-match test of one query against a database of images, two ways on one MI355X in one process:
  * baseline: Context.match_accepted_batch over (query, bank_i) pairs, one resident bank per image made beforehand
    (page-locked outputs, the batched per-pair launches);
  * Collection.match_accepted_each on a collection of the same images, and its counts-only call Collection.accepted_votes.
Both answers are compared row by row before anything is timed.  Each figure is the median over --reps repetitions, the two
paths alternating, of (a) a host clock around the call and the synchronisation that completes its results in host memory
and (b) the library's own HIP-event time of the same calls (fm_get_stats: total_ms).
    python scripts/bench_collection_accepted.py [--reps 21] [--images 64] [--nq 10000] [--json FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import fastmatch_amd                          # noqa: E402
from fastmatch_amd import synth               # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--tau", type=float, default=0.9)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    ctx = fastmatch_amd.Context(0)
    rng = np.random.default_rng(7)
    ni, nq, tau = args.images, args.nq, args.tau
    sizes = [int(s) for s in np.linspace(8000, 16000, ni).round()]          # 8k .. 16k rows, all different
    sizes = [s + i % 2 for i, s in enumerate(sizes)]
    assert len(set(sizes)) == ni
    order = rng.permutation(ni)
    sizes = [sizes[i] for i in order]
    images = [synth.synth_sift(n, rng) for n in sizes]
    Q = synth.synth_sift(nq, rng)
    pool = np.concatenate([im[:400] for im in images])
    take = rng.random(nq) < 0.5                                               # half the query rows have a near copy somewhere
    noisy = np.clip(pool[rng.integers(0, pool.shape[0], nq)].astype(np.int32) + rng.integers(-4, 5, (nq, 128)), 0, 255).astype(np.uint8)
    Q[take] = noisy[take]
    qb = ctx.bank(Q)
    ctx.self_dist_batch([qb], want_host=False)
    banks = [ctx.bank(im) for im in images]
    coll = ctx.collection()
    for im in images:
        coll.add(im)
    coll.train()
    outs = [tuple(ctx.pinned_empty(nq, dt) for dt in (np.int32, np.int32, np.float32, np.float64)) for _ in range(ni)]
    counts = [ctx.pinned_empty(1, np.int64) for _ in range(ni)]
    batch = ctx.prepare_batch([(qb, b) for b in banks], outs, counts)

    def run_batch():
        ctx.match_accepted_batch(batch, tau)
        ctx.sync()

    res = {}

    def run_each():
        res["each"] = coll.match_accepted_each(qb, tau)

    def run_votes():
        res["votes"] = coll.accepted_votes(qb, tau)

    run_batch(); run_each(); run_votes()
    total = 0
    for i in range(ni):
        m = int(counts[i][0])
        total += m
        got = res["each"][i]
        assert len(got[0]) == m == int(res["votes"][i]), "image %d: counts differ" % i
        assert np.array_equal(got[0], outs[i][0][:m]) and np.array_equal(got[1], outs[i][1][:m])
        assert np.array_equal(got[2].view(np.uint32), outs[i][2][:m].view(np.uint32))
        assert np.array_equal(got[3].view(np.uint64), outs[i][3][:m].view(np.uint64))
    paths = [("match_accepted_batch", run_batch), ("match_accepted_each", run_each), ("accepted_votes", run_votes)]
    for _ in range(args.warmup):
        for _, fn in paths:
            fn()
    wall = {k: [] for k, _ in paths}
    dev = {k: [] for k, _ in paths}
    for _ in range(args.reps):
        for k, fn in paths:                                                   # alternating: the paths share whatever the box does
            ctx.reset_stats()
            t0 = time.perf_counter()
            fn()
            wall[k].append((time.perf_counter() - t0) * 1e3)
            dev[k].append(ctx.stats()["total_ms"])
    out = {"device": ctx.device_name(), "images": ni, "rows_min": min(sizes), "rows_max": max(sizes), "rows_total": int(sum(sizes)),
           "nq": nq, "tau": tau, "accepted_total": total, "reps": args.reps, "warmup": args.warmup}
    for k, _ in paths:
        out[k] = {"wall_ms_median": float(np.median(wall[k])), "wall_ms_min": float(np.min(wall[k])), "wall_ms_max": float(np.max(wall[k])),
                  "event_ms_median": float(np.median(dev[k]))}
    base = out["match_accepted_batch"]["wall_ms_median"]
    out["each_over_batch"] = out["match_accepted_each"]["wall_ms_median"] / base
    out["votes_over_batch"] = out["accepted_votes"]["wall_ms_median"] / base
    line = json.dumps(out)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
