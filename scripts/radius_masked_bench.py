"""Masked radiusMatch (fm_radius_match_masked: the rmask_* sweeps of radius.hip) beside the unmasked call, in one process.
  python scripts/radius_masked_bench.py [--reps N] [--nq N] [--nt N] [--nt-wide N] [--kinds i8,f32,ham,wide] [--lib PATH]

Per kind -- i8 (uint8 128-D), f32 (float32 128-D, the fp16 filter + exact rescoring), ham (32-byte binary rows), wide (256-D
float32) -- 10 000 query rows against 1 000 000 train rows (wide: 200 000), a scalar radius found by bisection on counts-only
calls so that the unmasked call lists about 10 rows per query row:
  unmasked   the unmasked call of this library (fm_radius_match / fm_hamming_radius_match / fm_wide_radius_match)
  ones       the masked call under an all-ones mask: the mask's overhead
  band       the masked call under a band mask that permits 1 / 64 of every row (nt / 64 consecutive train rows per query row:
             63 of 64 mask words are zero, the stage skips run)
  hostfilter the unmasked call followed by a NumPy filter of its lists for the same band: what a caller did before
Each figure is the wall time in ms of the whole synchronous Python call (a counts call that sizes the arrays, then the fill
call; it ends in the library's stream synchronise), one warm-up, `reps` repeats: [median, min, max].  One JSON line per kind.
--lib PATH times a library built from ANOTHER commit (the baseline: the parent commit's unmasked call); the masked columns are
left out when that library lacks the masked entry points.  The spread of repeated runs is the min / max beside each median."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MASKED = ("fm_radius_match_masked", "fm_radius_match_masked_dev", "fm_collection_radius_match_masked", "fm_collection_radius_match_masked_dev")


def _timed(f, reps):
    f()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ms.append(1e3 * (time.perf_counter() - t0))
    return [round(float(np.median(ms)), 3), round(float(np.min(ms)), 3), round(float(np.max(ms)), 3)]


def _data(kind, nq, nt, rng):
    if kind == "ham":
        base = rng.integers(0, 256, (max(1, nt // 40), 32), dtype=np.uint8)

        def rows(n):
            x = base[rng.integers(0, len(base), n)].copy()
            flips = rng.integers(0, 256, (n, 3))
            for c in range(3):
                x[np.arange(n), flips[:, c] >> 3] ^= (1 << (flips[:, c] & 7)).astype(np.uint8)
            return x
        return rows(nq), rows(nt)
    dim = 256 if kind == "wide" else 128
    if kind == "i8":
        return rng.integers(0, 96, (nq, dim), dtype=np.uint8), rng.integers(0, 96, (nt, dim), dtype=np.uint8)
    return rng.random((nq, dim), dtype=np.float32), rng.random((nt, dim), dtype=np.float32)


def _radius_for(count, lo, hi, nq, target=10.0):
    """Bisection on the counts-only call: a radius whose mean list size is about `target`."""
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        mean = count(mid) / float(nq)
        if abs(mean - target) < 0.15 * target:
            return mid, mean
        lo, hi = (mid, hi) if mean < target else (lo, mid)
    return mid, mean


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--nt", type=int, default=1000000)
    ap.add_argument("--nt-wide", type=int, default=200000)
    ap.add_argument("--kinds", default="i8,f32,ham,wide")
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    from fastmatch_amd import _ffi
    if a.lib:
        _ffi.LIB_PATH = os.path.abspath(a.lib)
        import ctypes
        probe = ctypes.CDLL(_ffi.LIB_PATH)
        for name in MASKED:
            if not hasattr(probe, name):
                _ffi.SYMBOLS.pop(name, None)
    import fastmatch_amd
    ctx = fastmatch_amd.Context(0)
    have_masked = all(n in _ffi.SYMBOLS for n in MASKED)
    for kind in a.kinds.split(","):
        nq, nt = a.nq, (a.nt_wide if kind == "wide" else a.nt)
        rng = np.random.default_rng(11)
        Q, T = _data(kind, nq, nt, rng)
        mk = (lambda x: ctx.bank_binary(x)) if kind == "ham" else (lambda x: ctx.bank(x, float_route=True)) if kind == "f32" else ctx.bank
        qb, tb = mk(Q), mk(T)
        plain = {"ham": ctx.hamming_radius_match, "wide": ctx.wide_radius_match}.get(kind, ctx.radius_match)
        name = {"ham": "fm_hamming_radius_match", "wide": "fm_wide_radius_match"}.get(kind, "fm_radius_match")

        def count(r):
            import ctypes
            off = np.zeros(nq + 1, np.int64)
            tot = ctypes.c_int64(0)
            ctx._check(getattr(ctx.lib, name)(ctx.handle, qb.handle, tb.handle, None, float(np.float32(r)), 0, off.ctypes.data, None, None,
                                             ctypes.byref(tot)))
            return tot.value
        hi = {"i8": 2000.0, "ham": 256.0}.get(kind, 20.0)
        r, mean = _radius_for(count, 0.0, hi, nq)
        if kind == "ham":
            r = np.floor(r) + 0.5
            mean = count(r) / float(nq)
        out = {"kind": kind, "nq": nq, "nt": nt, "radius": float(r), "mean_list": round(mean, 2), "reps": a.reps,
               "lib": a.lib or "this commit", "unmasked_ms": _timed(lambda: plain(qb, tb, r), a.reps)}
        w = nt // 64
        start = (np.arange(nq, dtype=np.int64) * 7919) % (nt - w)

        def hostfilter():
            off, idx, dist = plain(qb, tb, r)
            rows = np.repeat(np.arange(nq), np.diff(off))
            keep = (idx >= start[rows]) & (idx < start[rows] + w)
            cnt = np.bincount(rows[keep], minlength=nq)
            return np.concatenate([[0], np.cumsum(cnt)]), idx[keep], dist[keep]
        out["hostfilter_ms"] = _timed(hostfilter, a.reps)
        if have_masked:
            import torch
            with ctx.mask(nq, nt) as m:
                m.set_all(True)
                got = ctx.radius_match_masked(qb, tb, m, r)
                ref = plain(qb, tb, r)
                assert all(np.array_equal(x, y) for x, y in zip(got, ref)), "all-ones differs from the unmasked call"
                out["ones_ms"] = _timed(lambda: ctx.radius_match_masked(qb, tb, m, r), a.reps)
                band = torch.zeros((nq, nt), dtype=torch.bool, device="cuda")
                for i in range(nq):
                    band[i, int(start[i]):int(start[i]) + w] = True
                torch.cuda.synchronize()
                m.set_dev(band.data_ptr(), pitch=nt, stream=torch.cuda.current_stream().cuda_stream)
                del band
                torch.cuda.empty_cache()
                got = ctx.radius_match_masked(qb, tb, m, r)
                want = hostfilter()
                assert all(np.array_equal(x, y) for x, y in zip(got, want)), "the band lists differ from the filtered unmasked lists"
                out["band_ms"] = _timed(lambda: ctx.radius_match_masked(qb, tb, m, r), a.reps)
                out["band_mean_list"] = round(float(got[0][-1]) / nq, 3)
        print(json.dumps(out), flush=True)
        qb.close()
        tb.close()


if __name__ == "__main__":
    main()
