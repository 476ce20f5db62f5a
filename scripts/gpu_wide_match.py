"""K14 (wide float banks, 129 .. 256 values per row) beside its yardstick, in one process: fm_knn2 and fm_xcheck1 at 256-D and
160-D on 4096 x 4096 (one SuperPoint pair), 10k x 100k and 10k x 1M rows, on the filter route ("f32_filter" 2) and the exact
route (0), and the same calls on the 128-D float32 route (K8 / K5) at the same row counts.  Kernel ms per call from
fm_get_stats (HIP events around the sweep's kernels), one warm-up call, then `reps` windows: median, min, max of the window's
mean (a window is 20 calls at 4096 x 4096, whose calls take a tenth of a millisecond, one call elsewhere).  Rows are
unit-norm and clustered (16-D subspace + noise), query rows near copies of train rows.  One JSON line per case; the last
column of each wide line is its time over the 128-D line of the same call, rows and route.
  python scripts/gpu_wide_match.py [reps] [out.jsonl] [max_nt]
  python scripts/gpu_wide_match.py profile      the 256-D filter route at 10k x 1M alone, three calls each: the run to put
                                                under rocprofv3 (--kernel-trace --stats; counters in a run of their own)"""
import json
import os
import sys

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


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "profile":
        return profile_run()
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
