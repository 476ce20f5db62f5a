"""GPU: NORM_HAMMING on binary banks (K11, hamming.hip) -- fm_knn (k = 1 .. 8), fm_knn2, fm_xcheck1 and fm_knn2_ratio equal
the NumPy reference (tests/hamming_ref.py) bit for bit, ties included; every other entry point refuses a binary bank."""
import ctypes

import numpy as np
import pytest

import fastmatch_amd
import hamming_ref as H
from fastmatch_amd import matchutil, _ffi

pytestmark = pytest.mark.gpu

WIDTHS = [1, 8, 16, 31, 32, 33, 40, 48, 61, 64]
SHAPES = [(0, 5), (5, 0), (1, 1), (2, 2), (15, 17), (17, 15), (127, 129), (129, 127), (1000, 4099), (4099, 1000)]


def _rows(rng, n, width, pool):
    if pool:
        P = rng.integers(0, 256, (pool, width), dtype=np.uint8)
        return P[rng.integers(0, pool, n)]
    return rng.integers(0, 256, (n, width), dtype=np.uint8)


def _same(a, b):
    assert a.shape == b.shape
    assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)


def _check_all(ctx, Q, T):
    qb, tb = ctx.bank_binary(Q), ctx.bank_binary(T)
    try:
        assert qb.kind == tb.kind == _ffi.FM_BANK_BIN and qb.dim == Q.shape[1]
        ridx, rdist = H.knn(Q, T, 8)
        for k in range(1, 9):
            idx, dist = ctx.knn(qb, tb, k)
            _same(idx, ridx[:, :k]); _same(dist, rdist[:, :k])
        idx, dist = ctx.knn2(qb, tb)
        _same(idx, ridx[:, :2]); _same(dist, rdist[:, :2])
        tidx, tdist = ctx.xcheck1(qb, tb)
        rt, rd = H.xcheck(Q, T)
        _same(tidx, rt); _same(tdist, rd)
    finally:
        qb.close(); tb.close()


@pytest.mark.parametrize("width", WIDTHS)
def test_knn_and_crosscheck_equal_the_reference(ctx, width):
    rng = np.random.default_rng(width)
    for nq, nt in SHAPES:
        for pool in (0, 24):                                  # random bits; a few dozen distinct rows (mass ties)
            _check_all(ctx, _rows(rng, nq, width, pool), _rows(rng, nt, width, pool))


@pytest.mark.parametrize("width", WIDTHS)
def test_every_distance_value_appears(ctx, width):
    """Rows at exactly h = 0 .. 8 * width from q (h = 512 at 64 bytes), in shuffled order."""
    rng = np.random.default_rng(100 + width)
    q = rng.integers(0, 256, width, dtype=np.uint8)
    bits = np.unpackbits(q)
    rows = []
    for h in range(8 * width + 1):
        b = bits.copy()
        flip = rng.permutation(8 * width)[:h]
        b[flip] ^= 1
        rows.append(np.packbits(b))
    R = np.array(rows, np.uint8)[rng.permutation(8 * width + 1)]
    Q1 = q[None, :]
    rb, qb = ctx.bank_binary(R), ctx.bank_binary(Q1)
    try:
        idx, dist = ctx.knn2(rb, qb)                           # every row against q: all 8 * width + 1 values
        assert sorted(dist[:, 0].tolist()) == [float(h) for h in range(8 * width + 1)]
        assert np.all(idx[:, 1] == -1) and np.all(np.isinf(dist[:, 1]))
        _check_all(ctx, R, Q1)
        _check_all(ctx, Q1, R)
        _check_all(ctx, R, R)
    finally:
        rb.close(); qb.close()


def test_ties_across_splits(ctx):
    """1-byte rows, 2000 x 200 000: hundreds of equal candidates per row spread over many workgroups -- the lowest index wins,
    in both directions of crossCheck."""
    rng = np.random.default_rng(7)
    Q = rng.integers(0, 256, (2000, 1), dtype=np.uint8)
    T = rng.integers(0, 256, (200000, 1), dtype=np.uint8)
    qb, tb = ctx.bank_binary(Q), ctx.bank_binary(T)
    try:
        ridx, rdist = H.knn(Q, T, 2)
        idx, dist = ctx.knn2(qb, tb)
        _same(idx, ridx); _same(dist, rdist)
        tidx, tdist = ctx.xcheck1(qb, tb)
        rt, rd = H.xcheck(Q, T)
        _same(tidx, rt); _same(tdist, rd)
    finally:
        qb.close(); tb.close()


def test_orb_100k(ctx):
    rng = np.random.default_rng(11)
    n = 100000
    Q = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    T = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    T[:500] = Q[rng.permutation(n)[:500]]                     # some exact matches
    qb, tb = ctx.bank_binary(Q), ctx.bank_binary(T)
    try:
        s = np.sort(rng.permutation(n)[:1024])
        idx, dist = ctx.knn2(qb, tb)
        ridx, rdist = H.knn(Q[s], T, 2)
        _same(idx[s], ridx); _same(dist[s], rdist)
        # crossCheck against a host scatter-min of the device's own reverse 1-NN, itself checked on samples
        e_idx, e_dist = ctx.knn(tb, qb, 1)
        r1, d1 = H.knn(T[s], Q, 1)
        _same(e_idx[s], r1); _same(e_dist[s], d1)
        rt, rd = H.scatter_min(e_idx[:, 0], e_dist[:, 0], n)
        tidx, tdist = ctx.xcheck1(qb, tb)
        _same(tidx, rt); _same(tdist, rd)
    finally:
        qb.close(); tb.close()
    Q8, T8 = Q[:8000], T[:8000]
    q8, t8 = ctx.bank_binary(Q8), ctx.bank_binary(T8)
    try:
        got = ctx.knn2_ratio(q8, t8, 0.8)
        ref = H.ratio_match(Q8, T8, 0.8)
        for a, b in zip(got, ref):
            assert np.array_equal(a, b)
        assert len(got[0]) > 0
    finally:
        q8.close(); t8.close()


def _rc(ctx, fn, *args):
    return getattr(ctx.lib, fn)(ctx.handle, *args)


def test_refusals(ctx):
    import torch
    rng = np.random.default_rng(3)
    B = rng.integers(0, 256, (40, 32), dtype=np.uint8)
    qb, tb = ctx.bank_binary(B), ctx.bank_binary(B[:30])
    i8 = ctx.bank(B)                                           # a uint8 [n, 32] L2 bank of the same dim
    i8e, bine = ctx.bank(np.zeros((0, 32), np.uint8)), ctx.bank_binary(np.zeros((0, 32), np.uint8))
    n = qb.n
    i32, f32, f64, u8 = np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros(n, np.float64), np.zeros(n, np.uint8)
    cnt = ctypes.c_int64(0)
    d_rows = torch.zeros(3 * n, dtype=torch.int32, device="cuda")
    d_cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    P = ctypes.c_void_p
    p = lambda a: a.ctypes.data                                 # noqa: E731
    E = -4                                                      # FM_EUNSUPPORTED
    try:
        offs = np.zeros(n + 1, np.int64)
        assert _rc(ctx, "fm_radius_match", qb.handle, tb.handle, None, 5.0, 0, p(offs), None, None, ctypes.byref(cnt)) == E
        assert "binary" in ctx.lib.fm_last_error(ctx.handle).decode()
        assert _rc(ctx, "fm_self_dist", qb.handle, p(f64)) == E
        assert _rc(ctx, "fm_self_dist_batch", 1, (P * 1)(qb.handle), None) == E
        assert _rc(ctx, "fm_bank_set_selfdist", qb.handle, p(f64)) == E
        assert _rc(ctx, "fm_match_ratio", qb.handle, tb.handle, 0.8, p(i32), p(f32), p(f64), p(u8), ctypes.byref(cnt)) == E
        assert _rc(ctx, "fm_match_accepted", qb.handle, tb.handle, 0.8, n, p(i32), p(i32), p(f32), p(f64), ctypes.byref(cnt)) == E
        assert _rc(ctx, "fm_match_accepted_async", qb.handle, tb.handle, 0.8, n, p(i32), p(i32), p(f32), p(f64), p(offs)) == E
        assert _rc(ctx, "fm_match_accepted_dev", qb.handle, tb.handle, 0.8, n, d_rows.data_ptr(), d_cnt.data_ptr(), None) == E
        assert _rc(ctx, "fm_match_accepted_dev_async", qb.handle, tb.handle, 0.8, n, d_rows.data_ptr(), d_cnt.data_ptr(), None,
                   P(-1)) == E
        pq, pt = (P * 1)(qb.handle), (P * 1)(tb.handle)
        outs = [(P * 1)(p(a)) for a in (i32, i32, f32, f64, offs)]
        assert _rc(ctx, "fm_match_accepted_batch", 1, pq, pt, 0.8, n, *outs) == E
        assert _rc(ctx, "fm_match_accepted_dev_batch", 1, pq, pt, 0.8, n, d_rows.data_ptr(), d_cnt.data_ptr(), None, P(-1)) == E
        keys = np.zeros(n, np.uint64)
        assert _rc(ctx, "fm_xcheck1_keys", qb.handle, tb.handle, 0, p(keys)) == E
        assert _rc(ctx, "fm_xcheck1_keys_dev", qb.handle, tb.handle, 0, d_cnt.data_ptr()) == E
        qo, to = np.array([0, 2], np.int64), np.array([0, 2], np.int64)
        assert _rc(ctx, "fm_xcheck1_batched", qb.handle, p(np.arange(2, dtype=np.int32)), p(qo), tb.handle, p(to), 1,
                   p(i32), p(f32), None) == E
        assert _rc(ctx, "fm_bank_refill_u8_async", qb.handle, p(B), 10) == E
        first = ctypes.c_int64(0)
        assert _rc(ctx, "fm_bank_append_u8", qb.handle, p(B), 1, ctypes.byref(first)) == E
        assert _rc(ctx, "fm_bank_append_f32", qb.handle, p(B.astype(np.float32)), 1, ctypes.byref(first)) == E
        desc = _ffi.fm_expand_desc()
        desc.query, desc.target = qb.handle, tb.handle
        ex = P()
        assert _rc(ctx, "fm_expand_create", ctypes.byref(desc), ctypes.byref(ex)) == E
        # mixed kinds: FM_EINVAL, an empty bank on either side included
        idx2, d2 = np.zeros((n, 2), np.int32), np.zeros((n, 2), np.float32)
        for a, b in ((qb, i8), (i8, qb), (qb, i8e), (bine, i8), (i8, bine), (i8e, qb)):
            assert _rc(ctx, "fm_knn2", a.handle, b.handle, p(idx2), p(d2)) == -1
            assert _rc(ctx, "fm_xcheck1", a.handle, b.handle, p(i32), p(f32)) == -1
            assert _rc(ctx, "fm_knn", a.handle, b.handle, 3, p(np.zeros((n, 3), np.int32)), p(np.zeros((n, 3), np.float32))) == -1
        # widths
        h = P()
        assert _rc(ctx, "fm_bank_create_bin", p(B), 4, 0, ctypes.byref(h)) == -1
        assert _rc(ctx, "fm_bank_create_bin", p(B), 4, -3, ctypes.byref(h)) == -1
        assert _rc(ctx, "fm_bank_create_bin", p(np.zeros((4, 65), np.uint8)), 4, 65, ctypes.byref(h)) == E
        assert _rc(ctx, "fm_knn", qb.handle, tb.handle, 9, p(np.zeros((n, 9), np.int32)), p(np.zeros((n, 9), np.float32))) == E
        # the banks still work after the refusals
        _same(ctx.knn2(qb, tb)[0], H.knn(B, B[:30], 2)[0])
    finally:
        for b in (qb, tb, i8, i8e, bine):
            b.close()


def test_bank_cycles_give_the_memory_back():
    c = fastmatch_amd.Context(0)
    rng = np.random.default_rng(5)
    B = rng.integers(0, 256, (1000, 32), dtype=np.uint8)

    def cycle(k):
        b = c.bank_binary(B[: 900 + k % 100])
        if k % 50 == 0:
            c.knn2(b, b)
        b.close()
    for k in range(20):
        cycle(k)
    c.sync()
    base = c.mem_info()[0]
    for k in range(500):
        cycle(k)
    c.sync()
    after = c.mem_info()[0]
    assert base - after <= (4 << 20), (base, after)
    c.close()


def _dm(lists):
    return [[(m.queryIdx, m.trainIdx, m.distance) for m in row] for row in lists]


def test_matchutil_norm_hamming(ctx):
    rng = np.random.default_rng(9)
    Q = rng.integers(0, 256, (300, 32), dtype=np.uint8)
    T = rng.integers(0, 256, (500, 32), dtype=np.uint8)
    T[::7] = T[0]                                             # duplicates: ties
    opts = {"normType": matchutil.NORM_HAMMING, "context": ctx}
    for k in (1, 2, 5):
        idx, dist = H.knn(Q, T, k)
        assert _dm(matchutil.bf_match(Q, T, k=k, options=opts)) == _dm(matchutil.matches_from_arrays(idx, dist))
        assert _dm(matchutil.flann_match(Q, T, k=k, options=opts)) == _dm(matchutil.matches_from_arrays(idx, dist))
    tidx, tdist = H.xcheck(Q, T)
    got = matchutil.bf_match(Q, T, k=1, options=dict(opts, crossCheck=True))
    assert _dm(got) == _dm(matchutil.matches_from_arrays(tidx, tdist))
    for a, b in zip(matchutil.ratio_match_arrays(Q, T, 0.9, options=opts), H.ratio_match(Q, T, 0.9)):
        assert np.array_equal(a, b)
    # resident banks, and what is refused
    qb, tb, lb = ctx.bank_binary(Q), ctx.bank_binary(T), ctx.bank(T)
    try:
        assert _dm(matchutil.bf_match(qb, tb, k=2, options=opts)) == _dm(matchutil.matches_from_arrays(*H.knn(Q, T, 2)))
        with pytest.raises(ValueError):
            matchutil.bf_match(qb, tb, k=2, options={"context": ctx})           # a binary bank without NORM_HAMMING
        with pytest.raises(ValueError):
            matchutil.bf_match(Q, lb, k=2, options=opts)                       # a resident L2 bank with NORM_HAMMING
        with pytest.raises(ValueError):
            matchutil.bf_radius_match(qb, tb, 10.0, options=opts)
        with pytest.raises(ValueError):
            matchutil.bf_match(Q, T, k=1, options={"normType": 7, "context": ctx})
    finally:
        qb.close(); tb.close(); lb.close()
    # no normType: a uint8 [n, 32] array is still a 32-D L2 bank
    idx, dist = matchutil.bf_match_arrays(Q, T, k=2, options={"context": ctx})
    d2 = ((Q[:, None, :].astype(np.int64) - T[None, :, :].astype(np.int64)) ** 2).sum(axis=2)
    order = np.argsort(d2, axis=1, kind="stable")[:, :2]
    assert np.array_equal(idx, order)
    assert np.array_equal(dist, np.sqrt(np.take_along_axis(d2, order, axis=1).astype(np.float32)))


def test_opencv_norm_hamming_crosscheck(ctx):
    cv2 = pytest.importorskip("cv2")
    rng = np.random.default_rng(13)
    Q = rng.integers(0, 256, (700, 32), dtype=np.uint8)
    T = rng.integers(0, 256, (900, 32), dtype=np.uint8)
    for cc in (False, True):
        bf = cv2.BFMatcher(cv2.NORM_HAMMING, crossCheck=cc)
        ref = bf.knnMatch(Q, T, k=1)
        got = matchutil.bf_match(Q, T, k=1, options={"normType": matchutil.NORM_HAMMING, "crossCheck": cc, "context": ctx})
        assert [[(m.queryIdx, m.trainIdx, m.distance) for m in r] for r in ref] == _dm(got)
