"""Times knnMatch(k = 2) under a mask on wide float descriptors (fm_wide_knn_masked, K14 under a mask) against the calls next to
it, alternating the cases in one process:

    knn2             fm_knn2 on the wide pair -- K14's filter, unmasked: the yardstick (its kernels are pinned, so this figure
                     must not move between the commit before the masked unit and this one: run --knn2-only on both)
    masked_ones      fm_wide_knn_masked(k = 2), every pair permitted
    masked_band      ... a band of 64 train rows round i * nt / nq per query row (guided matching: the tile skip)
    masked_exact_band  the same band on the masked exact kernel (option "f32_filter" 0): what the workgroup skip gives it
    f32_128_ones     fm_knn_masked(k = 2) on 128-D float banks of the same row counts, every pair permitted -- the vector-ALU
                     route, the figure a float user has today

Two times per case, both from the library's own HIP events: `*_ms` is the kernel bracket (fm_stats.kernel_ms of one call; for
the masked calls sweep, rescoring and merge, for fm_knn2 the sweep and rescoring, whose merge lies outside its bracket) and
`*_call_ms` the whole call (fm_stats.total_ms: every kernel and the copy of the [nq][2] lists to the host) -- the same
interval for every case, the one to compare across cases.  Warm-up calls of every case come first; the cases alternate
inside every repetition, so drift of the clock or of a shared host hits all of them alike.  The band is drawn on the device
(torch) and packed by fm_mask_set_dev.  Before any timing the masked all-ones result is compared with fm_knn2's, bit for
bit, and the band result of the filter with the exact kernel's.  One JSON line on stdout.

    python scripts/wide_masked_bench.py [--nq 10000] [--nt 100000] [--dim 256] [--reps 10] [--warmup 2] [--knn2-only]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fastmatch_amd                      # noqa: E402


def _times_ms(ctx, fn):
    """(kernel bracket, whole call) of one call, both from the library's HIP events"""
    ctx.reset_stats()
    fn()
    st = ctx.stats()
    return float(st["kernel_ms"]), float(st["total_ms"])


def _band_mask(ctx, nq, nt, width=64):
    """An fm_mask that permits `width` train rows round i * nt / nq for query row i, drawn on the device."""
    import torch
    dev = torch.device("cuda", ctx.device)
    m = torch.empty((nq, nt), dtype=torch.bool, device=dev)
    cols = torch.arange(nt, device=dev)[None, :]
    for r0 in range(0, nq, 1000):
        r1 = min(nq, r0 + 1000)
        centre = (torch.arange(r0, r1, device=dev, dtype=torch.int64) * nt // nq)[:, None]
        m[r0:r1] = (cols >= centre - width // 2) & (cols < centre + width // 2)
    mk = ctx.mask(nq, nt)
    mk.set_dev(m.data_ptr(), pitch=m.stride(0), stream=torch.cuda.current_stream().cuda_stream)
    return mk


def _unit_rows(rng, n, dim):
    """Unit-norm rows on a 16-D subspace plus noise: learned descriptors are L2-normalised and far from isotropic."""
    B = rng.standard_normal((16, dim))
    a = rng.standard_normal((n, 16)) @ B + 0.05 * rng.standard_normal((n, dim))
    return (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--nt", type=int, default=100000)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--knn2-only", action="store_true", help="fm_knn2 alone: runs on a library without the masked unit too")
    a = ap.parse_args()
    ctx = fastmatch_amd.Context(0)
    rng = np.random.default_rng(13)
    Q, T = _unit_rows(rng, a.nq, a.dim), _unit_rows(rng, a.nt, a.dim)
    qb, tb = ctx.bank(Q), ctx.bank(T)
    cases = [("knn2", lambda: ctx.knn2(qb, tb))]
    rec = {"nq": a.nq, "nt": a.nt, "dim": a.dim, "reps": a.reps, "device": ctx.device_name()}
    if not a.knn2_only:
        ones = ctx.mask(a.nq, a.nt).set_all(True)
        band = _band_mask(ctx, a.nq, a.nt)
        q128, t128 = ctx.bank(Q[:, :128], float_route=True), ctx.bank(T[:, :128], float_route=True)

        def exact(mk):
            old = ctx.get_option("f32_filter")
            ctx.set_option("f32_filter", 0)
            try:
                return ctx.wide_knn_masked(qb, tb, mk, 2)
            finally:
                ctx.set_option("f32_filter", old)

        cases += [("masked_ones", lambda: ctx.wide_knn_masked(qb, tb, ones, 2)),
                  ("masked_band", lambda: ctx.wide_knn_masked(qb, tb, band, 2)),
                  ("masked_exact_band", lambda: exact(band)),
                  ("f32_128_ones", lambda: ctx.knn_masked(q128, t128, ones, 2))]
        if not _same(ctx.wide_knn_masked(qb, tb, ones, 2), ctx.knn2(qb, tb)):
            raise SystemExit("masked_ones differs from fm_knn2")
        if not _same(ctx.wide_knn_masked(qb, tb, band, 2), exact(band)):
            raise SystemExit("masked_band: the filter differs from the exact kernel")
        rec["mask_bytes"] = ones.nbytes
        rec["filter_stats"] = list(ctx.f32_filter_stats())
    for _ in range(a.warmup):
        for _, fn in cases:
            fn()
    times = {name: [] for name, _ in cases}
    calls = {name: [] for name, _ in cases}
    for _ in range(a.reps):
        for name, fn in cases:
            k_ms, c_ms = _times_ms(ctx, fn)
            times[name].append(k_ms)
            calls[name].append(c_ms)
    for name, t in times.items():
        rec[name + "_ms"] = float(np.median(t))
        rec[name + "_min_ms"] = float(min(t))
        rec[name + "_max_ms"] = float(max(t))
        rec[name + "_call_ms"] = float(np.median(calls[name]))
        rec[name + "_call_min_ms"] = float(min(calls[name]))
        rec[name + "_call_max_ms"] = float(max(calls[name]))
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
