"""Hamming Fast-Match (fm_hamming_self_dist(_batch), fm_hamming_match_accepted) against what it replaces, in one process:
  self     the masked-diagonal top-1 self sweep (ham_self_kernel) against the existing way to the same values, the second
           column of fm_knn2(b, b) (K11's top-2 sweep), on one bank of `rows` x 32-byte rows (default 100k)
  batch    fm_hamming_self_dist_batch on 64 banks of ~12k rows (enqueue only, one fm_sync) against 64 fm_hamming_self_dist calls
  match    fm_hamming_match_accepted against fm_xcheck1 on the same pair (rows / 2 x rows / 2): the same sweep and election,
           plus the ratio test and the compaction
Per case: wall time of whole synchronous calls and the sweep's kernel time from the library's own events (fm_stats
kernel_ms; the batch's enqueue-only form is accounted at fm_sync).  One warm-up, `reps` repeats, median and (min, max) of
each.  One JSON line per case.
  python scripts/gpu_hamming_fast.py [reps] [rows]

Data: clustered as in tests/hamming_radius_ref.py -- a row is a random base row with k of {0, 1, 2, 5, 17, 40} random bit
flips (drawn with replacement here, vectorised), one base per 40 rows."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fastmatch_amd                                      # noqa: E402

NBYTES = 32
FLIPS = np.array([0, 1, 2, 5, 17, 40])


def _clustered(n, rng, base):
    rows = base[rng.integers(0, len(base), n)].copy()
    k = FLIPS[rng.integers(0, len(FLIPS), n)]
    for j in range(int(FLIPS.max())):
        on = np.nonzero(k > j)[0]
        bits = rng.integers(0, 8 * NBYTES, len(on))
        rows[on, bits >> 3] ^= (1 << (bits & 7)).astype(np.uint8)
    return rows


def _timed(ctx, f, reps):
    """(wall ms [median, min, max], kernel ms [median, min, max]) of f over reps calls after one warm-up."""
    f()
    wall, kern = [], []
    for _ in range(reps):
        ctx.reset_stats()
        t0 = time.perf_counter()
        f()
        wall.append(1e3 * (time.perf_counter() - t0))
        kern.append(ctx.stats()["kernel_ms"])
    return [[float(np.median(x)), float(np.min(x)), float(np.max(x))] for x in (wall, kern)]


def _emit(ctx, **kw):
    kw["device"] = ctx.device_name()
    print(json.dumps(kw), flush=True)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 100000
    ctx = fastmatch_amd.Context(0)
    rng = np.random.default_rng(78)
    base = rng.integers(0, 256, (max(24, n // 40), NBYTES), dtype=np.uint8)
    B = _clustered(n, rng, base)

    # 1. the self sweep against the top-2 form
    b = ctx.bank_binary(B)
    sd = ctx.hamming_self_dist(b)
    assert np.array_equal(sd, ctx.knn2(b, b)[1][:, 1].astype(np.float64))
    sw, sk = _timed(ctx, lambda: ctx.hamming_self_dist(b), reps)
    kw, kk = _timed(ctx, lambda: ctx.knn2(b, b), reps)
    _emit(ctx, case="self", rows=n, bytes=NBYTES, reps=reps, self_dist_ms=sw, self_dist_kernel_ms=sk, knn2_ms=kw, knn2_kernel_ms=kk,
          kernel_ratio=sk[0] / max(kk[0], 1e-9), wall_ratio=sw[0] / kw[0])
    b.close()

    # 2. the batched launch against bank-by-bank calls: 64 banks of ~12k rows
    sizes = [int(s) for s in rng.integers(11000, 13000, 64)]
    banks = [ctx.bank_binary(_clustered(s, rng, base)) for s in sizes]

    def batched():
        ctx.hamming_self_dist_batch(banks, want_host=False)
        ctx.sync()

    def one_by_one():
        for x in banks:
            ctx.hamming_self_dist(x)

    bw, bk = _timed(ctx, batched, reps)
    ow, ok = _timed(ctx, one_by_one, reps)
    _emit(ctx, case="batch", banks=64, rows_mean=float(np.mean(sizes)), bytes=NBYTES, reps=reps, batch_group=ctx.get_option("batch_group"),
          batched_ms=bw, batched_kernel_ms=bk, one_by_one_ms=ow, one_by_one_kernel_ms=ok, wall_ratio=bw[0] / ow[0],
          per_bank_us=[1e3 * bw[0] / 64, 1e3 * ow[0] / 64])
    for x in banks:
        x.close()

    # 3. the accepted-match test against the cross-check it is built on
    m = n // 2
    q, t = ctx.bank_binary(B[:m]), ctx.bank_binary(_clustered(m, rng, base))
    ctx.hamming_self_dist_batch([q], want_host=False)
    out = tuple(ctx.pinned_empty(m, dt) for dt in (np.int32, np.int32, np.float32, np.float64))
    acc = len(ctx.hamming_match_accepted(q, t, 0.8, out=out)[0])
    aw, ak = _timed(ctx, lambda: ctx.hamming_match_accepted(q, t, 0.8, out=out), reps)
    xw, xk = _timed(ctx, lambda: ctx.xcheck1(q, t), reps)
    _emit(ctx, case="match", nq=m, nt=m, bytes=NBYTES, tau=0.8, accepted=acc, reps=reps, accepted_ms=aw, accepted_kernel_ms=ak,
          xcheck1_ms=xw, xcheck1_kernel_ms=xk, wall_ratio=aw[0] / xw[0])
    q.close()
    t.close()
    ctx.close()


if __name__ == "__main__":
    main()
