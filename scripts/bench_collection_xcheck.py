"""crossCheck of one query against a database of images, two ways on one MI355X in one process:
  * the loop people write by hand: Context.xcheck1(q, bank_i) over one resident bank per image made beforehand;
  * Collection.xcheck1_each on a collection of the same images, and its counts-only call Collection.mutual_votes.
The answers are compared bit for bit before anything is timed.  Each figure is the median over --reps repetitions, the
paths alternating, of the library's own HIP-event time of the calls (fm_get_stats: total_ms, kernel_ms) and of a host
clock around them.  Routes: the integer route (uint8 rows), binary rows of 32 bytes, the float32 route.
    python scripts/bench_collection_xcheck.py [--reps 11] [--images 200] [--rows 2000] [--nq 2000] [--json FILE]
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


def _route_data(route, ni, rows, nq, rng):
    if route == "bin32":
        images = [rng.integers(0, 256, (rows, 32), dtype=np.uint8) for _ in range(ni)]
        return images, rng.integers(0, 256, (nq, 32), dtype=np.uint8)
    images = [synth.synth_sift(rows, rng) for _ in range(ni)]
    Q = synth.synth_sift(nq, rng)
    if route == "f32":
        images = [(im.astype(np.float32) + np.float32(0.25)) / np.float32(512) for im in images]
        Q = (Q.astype(np.float32) + np.float32(0.25)) / np.float32(512)
    return images, Q


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--images", type=int, default=200)
    ap.add_argument("--rows", type=int, default=2000)
    ap.add_argument("--nq", type=int, default=2000)
    ap.add_argument("--routes", default="u8,bin32,f32")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    ctx = fastmatch_amd.Context(0)
    out = {"device": ctx.device_name(), "images": args.images, "rows": args.rows, "nq": args.nq, "reps": args.reps}
    for route in args.routes.split(","):
        rng = np.random.default_rng(9)
        images, Q = _route_data(route, args.images, args.rows, args.nq, rng)
        binary, f32 = route == "bin32", route == "f32"
        mk = ctx.bank_binary if binary else (lambda a: ctx.bank(a, float_route=f32))
        qb = mk(Q)
        banks = [mk(im) for im in images]
        coll = ctx.collection()
        for im in images:
            coll.add_binary(im) if binary else coll.add(im)
        coll.train()
        res = {}

        def run_loop():
            res["loop"] = [ctx.xcheck1(qb, b) for b in banks]

        def run_each():
            res["each"] = coll.xcheck1_each(qb)

        def run_votes():
            res["votes"] = coll.mutual_votes(qb)

        paths = [("xcheck1_loop", run_loop), ("xcheck1_each", run_each), ("mutual_votes", run_votes)]
        for _, fn in paths:
            fn()
        for i, (t, d) in enumerate(res["loop"]):
            assert np.array_equal(t, res["each"][0][i]) and np.array_equal(d.view(np.uint32), res["each"][1][i].view(np.uint32)), (route, i)
            assert int((t >= 0).sum()) == int(res["votes"][i])
        for _ in range(args.warmup):
            for _, fn in paths:
                fn()
        wall = {k: [] for k, _ in paths}
        total = {k: [] for k, _ in paths}
        kern = {k: [] for k, _ in paths}
        for _ in range(args.reps):
            for k, fn in paths:
                ctx.reset_stats()
                t0 = time.perf_counter()
                fn()
                wall[k].append((time.perf_counter() - t0) * 1e3)
                st = ctx.stats()
                total[k].append(st["total_ms"])
                kern[k].append(st["kernel_ms"])
        r = {"matched_total": int(sum(int(v) for v in res["votes"]))}
        for k, _ in paths:
            r[k] = {"event_total_ms_median": float(np.median(total[k])), "event_kernel_ms_median": float(np.median(kern[k])),
                    "wall_ms_median": float(np.median(wall[k]))}
        r["loop_over_each_event_total"] = r["xcheck1_loop"]["event_total_ms_median"] / r["xcheck1_each"]["event_total_ms_median"]
        out[route] = r
        coll.close()
        qb.close()
        for b in banks:
            b.close()
    line = json.dumps(out)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
