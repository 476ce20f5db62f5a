"""Times knnMatch(k = 2) under a mask (fm_knn_masked, K13) against the unmasked fm_knn it shares its contract with, on uint8
rows, alternating the cases in one process:

    knn             fm_knn(k = 2) -- K2's matrix-core sweep, the yardstick
    masked_ones     fm_knn_masked(k = 2), every pair permitted
    masked_0.5      ... a random mask of density 0.5
    masked_0.01     ... of density 0.01
    masked_k9_ones  the masked vector-ALU instantiation (option "masked_mfma" = 0), every pair permitted
    masked_k9_0.01  ... at density 0.01

Two times per case, both from the library's own HIP events: `*_ms` is the kernel bracket (fm_stats.kernel_ms of one call: sweep
+ merge for the masked calls, the sweep alone for fm_knn, whose merge lies outside its bracket) and `*_call_ms` the whole
call (fm_stats.total_ms: every kernel and the copy of the [nq][2] lists to the host) -- the same interval for every case,
the one to compare across cases.  Warm-up calls of every case come first; the cases alternate inside every repetition, so drift of the clock or of a shared host hits all
of them alike.  The masks are drawn on the device (torch) and packed by fm_mask_set_dev.  Before any timing the masked
all-ones result is compared with fm_knn's, bit for bit.  One JSON line on stdout.

    python scripts/bench_knn_masked.py [--nq 10000] [--nt 100000] [--reps 10] [--warmup 2]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fastmatch_amd                      # noqa: E402
from fastmatch_amd import synth           # noqa: E402


def _times_ms(ctx, fn):
    """(kernel bracket, whole call) of one call, both from the library's HIP events"""
    ctx.reset_stats()
    fn()
    st = ctx.stats()
    return float(st["kernel_ms"]), float(st["total_ms"])


def _random_mask(ctx, nq, nt, density, seed):
    """An fm_mask of the given density, drawn on the device in chunks of query rows."""
    import torch
    dev = torch.device("cuda", ctx.device)
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    m = torch.empty((nq, nt), dtype=torch.bool, device=dev)
    for r0 in range(0, nq, 1000):
        r1 = min(nq, r0 + 1000)
        m[r0:r1] = torch.rand((r1 - r0, nt), device=dev, generator=g) < density
    mk = ctx.mask(nq, nt)
    mk.set_dev(m.data_ptr(), pitch=m.stride(0), stream=torch.cuda.current_stream().cuda_stream)
    return mk


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--nt", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    ctx = fastmatch_amd.Context(0)
    rng = np.random.default_rng(13)
    qb, tb = ctx.bank(synth.synth_sift(a.nq, rng)), ctx.bank(synth.synth_sift(a.nt, rng))
    ones = ctx.mask(a.nq, a.nt).set_all(True)
    half = _random_mask(ctx, a.nq, a.nt, 0.5, 1)
    sparse = _random_mask(ctx, a.nq, a.nt, 0.01, 2)

    def k9(mk):
        ctx.set_option("masked_mfma", 0)
        try:
            return ctx.knn_masked(qb, tb, mk, 2)
        finally:
            ctx.set_option("masked_mfma", 1)

    cases = [("knn", lambda: ctx.knn(qb, tb, 2)), ("masked_ones", lambda: ctx.knn_masked(qb, tb, ones, 2)),
             ("masked_0.5", lambda: ctx.knn_masked(qb, tb, half, 2)), ("masked_0.01", lambda: ctx.knn_masked(qb, tb, sparse, 2)),
             ("masked_k9_ones", lambda: k9(ones)), ("masked_k9_0.01", lambda: k9(sparse))]
    want = ctx.knn(qb, tb, 2)
    for name in ("masked_ones", "masked_k9_ones"):
        got = dict(cases)[name]()
        if not (np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))):
            raise SystemExit("%s differs from fm_knn" % name)
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
    rec = {"nq": a.nq, "nt": a.nt, "reps": a.reps, "device": ctx.device_name(), "mask_bytes": ones.nbytes}
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
