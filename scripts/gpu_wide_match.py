"""K14 (wide float banks, 129 .. 256 values per row) beside its yardstick, in one process: fm_knn2 and fm_xcheck1 at 256-D and
160-D on 4096 x 4096 (one SuperPoint pair), 10k x 100k and 10k x 1M rows, on the filter route ("f32_filter" 2) and the exact
route (0), and the same calls on the 128-D float32 route (K8 / K5) at the same row counts.  Kernel ms per call from
fm_get_stats (HIP events around the sweep's kernels), one warm-up call, then `reps` windows: median, min, max of the window's
mean (a window is 20 calls at 4096 x 4096, whose calls take a tenth of a millisecond, one call elsewhere).  Rows are
unit-norm and clustered (16-D subspace + noise), query rows near copies of train rows.  One JSON line per case; the last
column of each wide line is its time over the 128-D line of the same call, rows and route.
  python scripts/gpu_wide_match.py [reps] [out.jsonl] [max_nt]
  python scripts/gpu_wide_match.py profile      the 256-D filter route at 10k x 1M alone, three calls each: the run to put
                                                under rocprofv3 (--kernel-trace --stats; counters in a run of their own)
  python scripts/gpu_wide_match.py query [reps] [out.jsonl] [loop.jsonl]
        a wide QUERY against a wide collection: 2 000 query rows against 100 images of 2 000 rows and against 1 000 images of
        500 rows (256-D), Collection.wide_mutual_ratio_each beside its yardstick, the loop of ctx.mutual_ratio(q, bank_i) over
        resident banks of the same images.  Kernel ms (fm_get_stats, summed over the loop's calls) AND wall ms per call of
        the whole query (time.perf_counter around the call or the loop: the loop's per-call costs are what the table form
        removes).  One JSON line per case.  loop.jsonl: the lines of a `query-loop` run, whose loop figures replace this
        process's as the yardstick (that run is made with the library of the commit before the call existed).
  python scripts/gpu_wide_match.py query-loop [reps] [out.jsonl]        the yardstick alone: needs nothing but fm_mutual_ratio"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fastmatch_amd                                      # noqa: E402


def rows(rng, n, dim, B):
    out = np.empty((n, dim), np.float32)
    for i in range(0, n, 65536):
        m = min(65536, n - i)
        a = rng.standard_normal((m, 16), dtype=np.float32) @ B + 0.05 * rng.standard_normal((m, dim), dtype=np.float32)
        out[i:i + m] = a / np.linalg.norm(a, axis=1, keepdims=True)
    return out


def kernel_ms(ctx, f, reps, inner=1):
    f()
    ms = []
    for _ in range(reps):
        ctx.reset_stats()
        for _ in range(inner):
            f()
        ms.append(ctx.stats()["kernel_ms"] / inner)
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def profile_run():
    ctx = fastmatch_amd.Context(0)
    nq, nt, dim = 10000, 1000000, 256
    rng = np.random.default_rng(nt + dim)
    B = rng.standard_normal((16, dim), dtype=np.float32)
    T = rows(rng, nt, dim, B)
    Q = T[rng.integers(0, nt, nq)] + (0.02 / np.sqrt(dim)) * rng.standard_normal((nq, dim), dtype=np.float32)
    Q = (Q / np.linalg.norm(Q, axis=1, keepdims=True)).astype(np.float32)
    qb, tb = ctx.bank(Q), ctx.bank(T)
    ctx.set_option("f32_filter", 2)
    for _ in range(3):
        ctx.knn2(qb, tb)
    for _ in range(3):
        ctx.xcheck1(qb, tb)
    print("profile run done, fallbacks", ctx.f32_filter_stats()[1])


QUERY_CASES = ((100, 2000), (1000, 500))       # (images, rows per image); the query has 2 000 rows


def window_ms(ctx, f, reps):
    """(kernel ms, wall ms) of one f(): one warm-up call, then the median, min and max over `reps` calls."""
    f()
    k, w = [], []
    for _ in range(reps):
        ctx.sync()
        ctx.reset_stats()
        t0 = time.perf_counter()
        f()
        ctx.sync()
        w.append((time.perf_counter() - t0) * 1e3)
        k.append(ctx.stats()["kernel_ms"])
    return [float(np.median(k)), float(min(k)), float(max(k))], [float(np.median(w)), float(min(w)), float(max(w))]


def query_run(loop_only):
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    out_path = sys.argv[3] if len(sys.argv) > 3 else None
    yard = {}
    if not loop_only and len(sys.argv) > 4:
        for line in open(sys.argv[4]):
            r = json.loads(line)
            yard[(r["images"], r["rows"])] = r
    ctx = fastmatch_amd.Context(0)
    out = open(out_path, "w") if out_path else None
    dim, nq, tau = 256, 2000, 0.8
    for ni, n in QUERY_CASES:
        rng = np.random.default_rng(ni + n)
        B = rng.standard_normal((16, dim), dtype=np.float32)
        images = [rows(rng, n, dim, B) for _ in range(ni)]
        # every query row a near copy of a row of some image
        src = np.stack([images[i][r] for i, r in zip(rng.integers(0, ni, nq), rng.integers(0, n, nq))])
        Q = src + (0.02 / np.sqrt(dim)) * rng.standard_normal((nq, dim), dtype=np.float32)
        Q = (Q / np.linalg.norm(Q, axis=1, keepdims=True)).astype(np.float32)
        qb = ctx.bank(Q)
        banks = [ctx.bank(im) for im in images]
        rec = {"call": "wide_mutual_ratio_each", "dim": dim, "nq": nq, "images": ni, "rows": n, "tau": tau, "reps": reps,
               "device": ctx.device_name()}
        ctx.set_option("f32_filter", 1)             # the option's default, for the loop and for the call: what a caller gets
        accepted = [0]

        def loop():
            accepted[0] = sum(ctx.mutual_ratio(qb, b, tau)[0].shape[0] for b in banks)
        k, w = window_ms(ctx, loop, reps)
        rec.update({"loop_kernel_ms": k, "loop_wall_ms": w, "loop_accepted": accepted[0], "loop_lib": "this"})
        if not loop_only:
            coll = ctx.collection()
            for im in images:
                coll.add_wide(im)
            got = [0]

            def each():
                got[0] = sum(g[0].shape[0] for g in coll.wide_mutual_ratio_each(qb, tau))

            def counts():
                got[0] = int(coll.wide_mutual_ratio_each_counts(qb, tau)[-1])
            for route, opt in (("default", 1), ("exact", 0)):
                ctx.set_option("f32_filter", opt)
                l0, f0 = ctx.f32_filter_stats()
                k, w = window_ms(ctx, counts, reps)             # ONE C call (wide_mutual_ratio_each makes two: counts, fill)
                l1, f1 = ctx.f32_filter_stats()
                rec.update({route + "_kernel_ms": k, route + "_wall_ms": w, route + "_chunks_filtered": (l1 - l0) // (reps + 1),
                            route + "_fallbacks": f1 - f0})
                assert got[0] == accepted[0], (got[0], accepted[0])
            ctx.set_option("f32_filter", 1)
            k, w = window_ms(ctx, each, reps)
            rec.update({"fill_kernel_ms": k, "fill_wall_ms": w, "accepted": got[0]})
            assert got[0] == accepted[0]
            y = yard.get((ni, n))
            if y:
                assert y["loop_accepted"] == accepted[0]
                rec.update({"loop_kernel_ms": y["loop_kernel_ms"], "loop_wall_ms": y["loop_wall_ms"], "loop_lib": "parent commit",
                            "loop_kernel_ms_this_lib": rec["loop_kernel_ms"], "loop_wall_ms_this_lib": rec["loop_wall_ms"]})
            rec["wall_speedup_over_loop"] = rec["loop_wall_ms"][0] / rec["default_wall_ms"][0]
            rec["kernel_speedup_over_loop"] = rec["loop_kernel_ms"][0] / rec["default_kernel_ms"][0]
            coll.close()
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
        qb.close()
        for b in banks:
            b.close()
    ctx.set_option("f32_filter", 1)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "profile":
        return profile_run()
    if len(sys.argv) > 1 and sys.argv[1] in ("query", "query-loop"):
        return query_run(sys.argv[1] == "query-loop")
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    out_path = sys.argv[2] if len(sys.argv) > 2 else None
    max_nt = int(sys.argv[3]) if len(sys.argv) > 3 else 1000000
    ctx = fastmatch_amd.Context(0)
    out = open(out_path, "w") if out_path else None
    base = {}
    for nq, nt in ((4096, 4096), (10000, 100000), (10000, 1000000)):
        if nt > max_nt:
            continue
        for dim in (128, 160, 256):
            rng = np.random.default_rng(nt + dim)
            B = rng.standard_normal((16, dim), dtype=np.float32)
            T = rows(rng, nt, dim, B)
            Q = T[rng.integers(0, nt, nq)] + (0.02 / np.sqrt(dim)) * rng.standard_normal((nq, dim), dtype=np.float32)
            Q = (Q / np.linalg.norm(Q, axis=1, keepdims=True)).astype(np.float32)
            qb, tb = ctx.bank(Q, float_route=True), ctx.bank(T, float_route=True)
            del T
            for route, opt in (("filter", 2), ("exact", 0)):
                ctx.set_option("f32_filter", opt)
                for call, f in (("knn2", lambda: ctx.knn2(qb, tb)), ("xcheck1", lambda: ctx.xcheck1(qb, tb))):
                    l0, f0 = ctx.f32_filter_stats()
                    med, lo, hi = kernel_ms(ctx, f, reps, 20 if nt <= 4096 else 1)
                    l1, f1 = ctx.f32_filter_stats()
                    rec = {"call": call, "route": route, "dim": dim, "kind": qb.kind, "nq": nq, "nt": nt, "reps": reps,
                           "kernel_ms": med, "min_ms": lo, "max_ms": hi, "pairs_per_s": nq * nt / (med * 1e-3),
                           "filter_launches": l1 - l0, "fallbacks": f1 - f0, "device": ctx.device_name()}
                    key = (call, route, nq, nt)
                    if dim == 128:
                        base[key] = med
                    else:
                        rec["over_128d"] = med / base[key]
                    line = json.dumps(rec)
                    print(line, flush=True)
                    if out:
                        out.write(line + "\n")
                        out.flush()
            qb.close(); tb.close()
    ctx.set_option("f32_filter", 1)


if __name__ == "__main__":
    main()
