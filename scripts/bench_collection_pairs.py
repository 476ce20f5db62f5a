"""Times the match graph of a train collection -- ONE fm_collection_pairs_mutual_ratio call -- against what it replaces: the
loop of fm_mutual_ratio over banks created beforehand, one call per pair (that path is untouched by the match graph, so it is
the parent commit's).  100 images x 2 000 rows on the three routes (uint8 in SIFT range, float32 with the fp16 filter,
32-byte binary); the exhaustive pair set (4 950 pairs) and a window of 5 (every i < j <= i + 5).  --routes wide: the same for a
WIDE collection (unit-norm 256-D float rows, fm_collection_add_wide) against the loop of fm_mutual_ratio on wide banks
(profiles/wide_collection_pairs.jsonl holds a recorded run).

The answers are compared bit for bit first.  Then the two alternate in one process and the medians of fm_stats' total_ms
(HIP-event time of the calls, the loop's summed over its calls) are reported, with the wall-clock medians beside them (the
loop's host time between its calls is in the wall clock only).  One JSON line per (route, pair set) on stdout and, with --out,
appended to that file (profiles/collection_pairs.jsonl holds a recorded run).

    python scripts/bench_collection_pairs.py [--images 100] [--rows 2000] [--reps 11] [--routes u8,f32,bin32,wide] [--out FILE]
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


def _images(route, n_images, rows, seed):
    """Images that share content: every image holds noisy views of a third of its rows' worth of a common pool."""
    rng = np.random.default_rng(seed)
    shared = rows // 3
    if route == "u8":
        pool = synth.synth_sift(4 * rows, rng)
        images = [synth.synth_sift(rows, rng) for _ in range(n_images)]
        for im in images:
            src = pool[rng.choice(pool.shape[0], shared, replace=False)]
            im[:shared] = np.clip(src.astype(np.int32) + rng.integers(-4, 5, src.shape), 0, 255).astype(np.uint8)
        return images
    if route == "wide":
        def unit(x):
            return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
        pool = unit(rng.normal(0.0, 1.0, (4 * rows, 256)))
        images = [unit(rng.normal(0.0, 1.0, (rows, 256))) for _ in range(n_images)]
        for im in images:
            src = pool[rng.choice(pool.shape[0], shared, replace=False)]
            im[:shared] = unit(src + rng.normal(0.0, 0.02 / 16.0, src.shape))
        return images
    if route == "f32":
        pool = rng.normal(0.0, 1.0, (4 * rows, 128)).astype(np.float32)
        images = [rng.normal(0.0, 1.0, (rows, 128)).astype(np.float32) for _ in range(n_images)]
        for im in images:
            src = pool[rng.choice(pool.shape[0], shared, replace=False)]
            im[:shared] = src + rng.normal(0.0, 0.05, src.shape).astype(np.float32)
        return images
    pool = rng.integers(0, 256, (4 * rows, 32), dtype=np.uint8)
    images = [rng.integers(0, 256, (rows, 32), dtype=np.uint8) for _ in range(n_images)]
    for im in images:
        src = pool[rng.choice(pool.shape[0], shared, replace=False)].copy()
        for _ in range(12):                   # 12 of 256 bits flipped (independent rows sit near 128)
            src[np.arange(shared), rng.integers(0, 32, shared)] ^= (1 << rng.integers(0, 8, shared)).astype(np.uint8)
        im[:shared] = src
    return images


def _same(a, b):
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32))
            and np.array_equal(a[3].view(np.uint64), b[3].view(np.uint64)))


def _measure(ctx, fn):
    ctx.sync()
    ctx.reset_stats()
    t0 = time.perf_counter()
    fn()
    ctx.sync()
    wall = (time.perf_counter() - t0) * 1e3
    return ctx.stats()["total_ms"], wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=100)
    ap.add_argument("--rows", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--tau", type=float, default=0.8)
    ap.add_argument("--routes", default="u8,f32,bin32")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = fastmatch_amd.Context(0)
    ni, tau = a.images, a.tau
    sets = (("exhaustive", None, [(i, j) for i in range(ni) for j in range(i + 1, ni)]),
            ("window5", [(i, j) for i in range(ni) for j in range(i + 1, min(ni, i + 6))], None))
    for route in a.routes.split(","):
        images = _images(route, ni, a.rows, 21)
        binary, fr, wide = route == "bin32", route == "f32", route == "wide"
        coll = ctx.collection()
        banks = []
        for im in images:
            coll.add_wide(im) if wide else coll.add_binary(im) if binary else coll.add(im)
            banks.append(ctx.bank_binary(im) if binary else ctx.bank(im, float_route=fr))
        ctx.set_option("f32_filter", 2 if fr else 1)       # (wide: the default rule takes the filter on both sides at these sizes)
        for name, pairs, implied in sets:
            plist = implied if pairs is None else pairs

            def loop():
                return [ctx.mutual_ratio(banks[i], banks[j], tau, True) for i, j in plist]
            offsets = coll.pairs_mutual_ratio_counts(pairs, tau, True)
            total = int(offsets[-1])

            def one():
                return coll.pairs_mutual_ratio(pairs, tau, True, cap=total)

            def counts():
                return coll.pairs_mutual_ratio_counts(pairs, tau, True)
            got, want = one(), loop()                       # (warm-up as well)
            same = len(got) == len(want) and all(_same(g, w) for g, w in zip(got, want))
            if not same:
                print(json.dumps({"route": route, "pairs": name, "identical": False}), flush=True)
                sys.exit("the match graph and the loop of pair calls disagree on %s / %s" % (route, name))
            t_one, t_loop, t_cnt, w_one, w_loop, w_cnt = [], [], [], [], [], []
            for _ in range(a.reps):
                for fn, ts, ws in ((loop, t_loop, w_loop), (one, t_one, w_one), (counts, t_cnt, w_cnt)):
                    t, w = _measure(ctx, fn)
                    ts.append(t); ws.append(w)
            med = lambda x: float(np.median(x))             # noqa: E731
            iqr = lambda x: float(np.subtract(*np.percentile(x, [75, 25])))      # noqa: E731
            rec = {"route": route, "pairs": name, "n_pairs": len(plist), "images": ni, "rows": a.rows, "tau": tau, "symmetric": True,
                   "matches": total, "identical": True, "reps": a.reps,
                   "one_call_total_ms": med(t_one), "loop_total_ms": med(t_loop), "counts_only_total_ms": med(t_cnt),
                   "one_call_iqr_ms": iqr(t_one), "loop_iqr_ms": iqr(t_loop),
                   "one_call_wall_ms": med(w_one), "loop_wall_ms": med(w_loop), "counts_only_wall_ms": med(w_cnt),
                   "speedup_total_ms": med(t_loop) / med(t_one), "speedup_wall": med(w_loop) / med(w_one),
                   "pairs_per_s_one_call": 2.0 * len(plist) * a.rows * a.rows / (med(t_one) * 1e-3), "device": ctx.device_name()}
            if wide:
                l0, f0 = ctx.f32_filter_stats()
                counts()
                l1, f1 = ctx.f32_filter_stats()
                rec["chunks_filtered_per_call"], rec["chunks_redone_per_call"] = l1 - l0, f1 - f0
                rec["t_one_ms"], rec["t_loop_ms"] = t_one, t_loop
            line = json.dumps(rec)
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")
        ctx.set_option("f32_filter", 1)
        for b in banks:
            b.close()
        coll.close()


if __name__ == "__main__":
    main()
