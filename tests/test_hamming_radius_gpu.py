"""GPU: Hamming radiusMatch -- fm_hamming_radius_match(_dev), fm_collection_hamming_radius_match(_dev) and the Python surfaces
on top of them -- against the NumPy reference (tests/hamming_radius_ref.py).  Every value is an integer: offsets and indices
are compared exactly, distances as bit patterns; there is no tolerance anywhere.

nq = 300 throughout: two workgroups of 256 query rows, the second partly empty.  nt = 2100: 17 stages of 128 rows, the last
one partial, in 5 splits (asserted from the restated split rule)."""
import ctypes

import numpy as np
import pytest

import fastmatch_amd
import hamming_radius_ref as HR
import radius_coll_ref as RC
from fastmatch_amd import _ffi, matchutil, torchmatch

pytestmark = pytest.mark.gpu

NQ, NT = 300, 2100
WIDTHS = [1, 16, 17, 32, 33, 48, 61, 64]
EINVAL = -1
S_OFF, S_IMG, S_IDX, S_DIST = -7, -77, -78, -79.0          # sentinels
INF = np.float32(np.inf)


def _torch():
    import torch
    return torch


def _dev(a):
    return _torch().from_numpy(np.array(a, order="C")).cuda()


def _split_r(r):
    if np.ndim(r) == 0:
        return None, float(np.float32(r))
    return np.ascontiguousarray(r, dtype=np.float32), 0.0


def _raw(ctx, qb, target, r, cap, size=None, lists=True):
    """One HOST call into sentinel-filled arrays.  target: a Bank or a Collection.  Returns (rc, n_total, offsets, img, idx, dist)."""
    coll = isinstance(target, _ffi.Collection)
    size = cap if size is None else size
    off = np.full(qb.n + 1, S_OFF, np.int64)
    img, idx = np.full(size, S_IMG, np.int32), np.full(size, S_IDX, np.int32)
    dist = np.full(size, S_DIST, np.float32)
    rad, r_all = _split_r(r)
    p = (lambda a: a.ctypes.data_as(ctypes.c_void_p)) if lists and size else (lambda a: None)
    rp = rad.ctypes.data_as(ctypes.c_void_p) if rad is not None else None
    tot = ctypes.c_int64(-5)
    if coll:
        rc = ctx.lib.fm_collection_hamming_radius_match(ctx.handle, target.handle, qb.handle, rp, r_all, cap, off.ctypes.data_as(ctypes.c_void_p),
                                                        p(img), p(idx), p(dist), ctypes.byref(tot))
    else:
        rc = ctx.lib.fm_hamming_radius_match(ctx.handle, qb.handle, target.handle, rp, r_all, cap, off.ctypes.data_as(ctypes.c_void_p),
                                             p(idx), p(dist), ctypes.byref(tot))
    return rc, tot.value, off, img, idx, dist


def _call_dev(ctx, qb, target, r, cap, size=None, lists=True):
    """One DEVICE call into sentinel-filled tensors (device radii where r is an array or a tensor).  Returns (n_total, offsets,
    img or None, idx, dist) as NumPy arrays."""
    torch = _torch()
    coll = isinstance(target, _ffi.Collection)
    size = cap if size is None else size
    off = torch.full((qb.n + 1,), S_OFF, dtype=torch.int64, device="cuda")
    img = torch.full((size,), S_IMG, dtype=torch.int32, device="cuda")
    idx = torch.full((size,), S_IDX, dtype=torch.int32, device="cuda")
    dist = torch.full((size,), S_DIST, dtype=torch.float32, device="cuda")
    if isinstance(r, torch.Tensor):
        rt, r_all = r, 0.0
    elif np.ndim(r) == 0:
        rt, r_all = None, float(np.float32(r))
    else:
        rt, r_all = _dev(np.asarray(r, np.float32)), 0.0
    s = torch.cuda.current_stream().cuda_stream
    p = (lambda t: t.data_ptr()) if lists and size else (lambda t: 0)
    rp = rt.data_ptr() if rt is not None else 0
    if coll:
        n = target.hamming_radius_match_dev(qb, rp, r_all, cap, off.data_ptr(), p(img), p(idx), p(dist), consumer_stream=s)
    else:
        n = ctx.hamming_radius_match_dev(qb, target, rp, r_all, cap, off.data_ptr(), p(idx), p(dist), consumer_stream=s)
    return n, off.cpu().numpy(), (img.cpu().numpy() if coll else None), idx.cpu().numpy(), dist.cpu().numpy()


def _full_dev(ctx, qb, target, r):
    """Counts call, then fill call, of the device form: (offsets, [img,] idx, dist)."""
    n0, off0 = _call_dev(ctx, qb, target, r, 0, lists=False)[:2]
    assert n0 == off0[-1]
    n, off, img, idx, dist = _call_dev(ctx, qb, target, r, n0)
    assert n == n0 and np.array_equal(off, off0)
    return (off, img, idx, dist) if img is not None else (off, idx, dist)


@pytest.fixture(scope="module")
def std32(ctx):
    """(query bank, train bank, reference) of the 32-byte data."""
    Q, T = HR.data(32)
    qb, tb = ctx.bank_binary(Q), ctx.bank_binary(T)
    yield qb, tb, HR.data_ref(32)
    tb.close()
    qb.close()


# ---- 1. widths --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbytes", WIDTHS)
def test_every_width_equals_the_reference(ctx, nbytes):
    W = 8 * nbytes
    Q, T = HR.data(nbytes)
    ref = HR.data_ref(nbytes)
    assert HR.sweep_splits(NQ, NT) == (5, 4) and NT % 128 != 0          # more than one split, a partial last stage
    c3, cinf = ref.counts(np.float32(3)), ref.counts(INF)
    assert (cinf > 2048).all()                                           # the rocPRIM sort path
    if nbytes >= 16:      # the three sort paths inside ONE call (W = 8 has 256 distinct rows: every ball of radius 3 is crowded)
        assert (c3 == 0).any() and ((c3 >= 1) & (c3 <= 16)).any() and ((c3 >= 17) & (c3 <= 2048)).any()
    else:
        c1 = ref.counts(np.float32(1))
        assert ((c1 >= 1) & (c1 <= 16)).any() and ((c3 >= 17) & (c3 <= 2048)).all()
    qb, tb = ctx.bank_binary(Q), ctx.bank_binary(T)
    try:
        for r in (1, 3, W / 2 + 1, W, np.inf):
            HR.same_pair_lists(ctx.hamming_radius_match(qb, tb, np.float32(r)), ref.cut(np.float32(r)), "%d bytes, r = %r" % (nbytes, r))
        # the complement row (h = W; at W = 8 a few more rows are that far) is outside r = W ...
        assert ref.counts(np.float32(W))[5] == NT - int((ref.h[5] == W).sum()) <= NT - 1 and ref.h[5, NT // 2] == W
        off, idx, dist = ctx.hamming_radius_match(qb, tb, np.float32(W + 0.5))
        row5 = slice(off[5], off[6])                                     # ... and among the last inside W + 0.5
        assert off[6] - off[5] == NT and dist[off[6] - 1] == W and NT // 2 in idx[row5][dist[row5] == W]
    finally:
        qb.close(); tb.close()


# ---- 2. small banks ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nt", [0, 1, 127, 128, 129])
def test_small_train_banks_leak_no_padding_row(ctx, nt):
    Q, T = HR.data(32)
    T = np.ascontiguousarray(T[:nt])
    ref = HR.Ref(Q, T)
    qb, tb = ctx.bank_binary(Q), ctx.bank_binary(T)
    try:
        for r in (np.inf, 8 * 32 / 2 + 1):
            got = ctx.hamming_radius_match(qb, tb, np.float32(r))
            assert np.diff(got[0]).max(initial=0) <= nt                   # (a padding row sits at h = W / 2: inside both radii)
            HR.same_pair_lists(got, ref.cut(np.float32(r)), "nt = %d, r = %r" % (nt, r))
        assert np.array_equal(np.diff(ctx.hamming_radius_match(qb, tb, INF)[0]), np.full(NQ, nt))
        q0 = ctx.bank_binary(Q[:0])                                       # nq = 0
        off, idx, dist = ctx.hamming_radius_match(q0, tb, INF)
        assert off.shape == (1,) and off[0] == 0 and idx.size == dist.size == 0
        q0.close()
    finally:
        qb.close(); tb.close()


# ---- 3. per-row radii -------------------------------------------------------------------------------------------------------
def test_per_row_radii_host_and_device_forms(ctx, std32):
    qb, tb, ref = std32
    radii = HR.mixed_radii(ref)
    want = ref.cut(radii)
    assert np.isnan(radii).sum() >= 3 and np.isinf(radii).sum() >= 3 and (radii == 0).sum() >= 3 and (radii < 0).sum() >= 3
    exact = radii[0::2][np.isfinite(radii[0::2]) & (radii[0::2] > 0)]
    assert (exact == np.round(exact)).all() and len(exact) > 50          # radii exactly on a distance: that distance is outside
    HR.same_pair_lists(ctx.hamming_radius_match(qb, tb, radii), want, "host form")
    HR.same_pair_lists(_full_dev(ctx, qb, tb, radii), want, "device form, radii uploaded")
    HR.same_pair_lists(_full_dev(ctx, qb, tb, _dev(radii)), want, "device form, radii tensor")
    for r in (0.0, np.nan, -2.0):                                        # no entries: the offsets are still written
        rc, tot, off = _raw(ctx, qb, tb, np.float32(r), 0, lists=False)[:3]
        assert rc == 0 and tot == 0 and not off.any()
        n, off = _call_dev(ctx, qb, tb, np.float32(r), 0, lists=False)[:2]
        assert n == 0 and not off.any()


# ---- 4. cap -----------------------------------------------------------------------------------------------------------------
def test_cap_counts_call_full_call_and_a_cap_inside_a_row(ctx, std32):
    qb, tb, ref = std32
    r = np.float32(3)
    woff, _, _, wdist, wglobal = ref.cut(r)
    total = int(woff[-1])
    row = int(np.nonzero(np.diff(woff) >= 2)[0][40])                     # a row with at least two entries, some way in
    mid = int(woff[row]) + 1                                             # cap in the middle of that row
    assert 0 < woff[row] < mid < woff[row + 1]
    for form in ("host", "dev"):
        def call(cap, size=None, lists=True):
            if form == "host":
                rc, tot, off, _, idx, dist = _raw(ctx, qb, tb, r, cap, size, lists)
                assert rc == 0
                return tot, off, idx, dist
            tot, off, _, idx, dist = _call_dev(ctx, qb, tb, r, cap, size, lists)
            return tot, off, idx, dist
        tot, off, _, _ = call(0, lists=False)                            # counts call, NULL arrays
        assert tot == total and np.array_equal(off, woff), form
        tot, off, idx, dist = call(total)
        assert tot == total and np.array_equal(off, woff) and np.array_equal(idx, wglobal), form
        assert np.array_equal(HR.bits(dist), HR.bits(wdist)), form
        tot, off, idx, dist = call(mid, size=total)
        k = int(woff[row])                                               # only the whole rows before `row` are written
        assert tot == total and np.array_equal(off, woff), form
        assert np.array_equal(idx[:k], wglobal[:k]) and np.array_equal(HR.bits(dist[:k]), HR.bits(wdist[:k])), form
        assert (idx[k:] == S_IDX).all() and (dist[k:] == np.float32(S_DIST)).all(), form


# ---- 5. chunking ------------------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_the_chunk_budget(ctx):
    """radius_ws_bytes at its smallest, 65536 = 2730 candidates of 24 bytes: nt = 2900 so that one row's list at r = +inf is
    longer than a chunk (it runs in a chunk of its own), and r = W / 2 + 1 needs dozens of chunks."""
    nt = 2900
    Q, T = HR.data(32, NQ, nt)
    ref = HR.data_ref(32, NQ, nt)
    per_chunk = 65536 // 24
    r_mid = np.float32(8 * 32 / 2 + 1)
    assert ref.cut(r_mid)[0][-1] > 4 * per_chunk                          # several chunks
    assert ref.counts(r_mid).max() < per_chunk < ref.counts(INF).min()    # rows share chunks; one row alone exceeds a chunk
    qb, tb = ctx.bank_binary(Q), ctx.bank_binary(T)
    old = ctx.get_option("radius_ws_bytes")
    ctx.set_option("radius_ws_bytes", 65536)
    try:
        for r in (r_mid, INF):
            HR.same_pair_lists(ctx.hamming_radius_match(qb, tb, r), ref.cut(r), "chunked host form")
            HR.same_pair_lists(_full_dev(ctx, qb, tb, r), ref.cut(r), "chunked device form")
    finally:
        ctx.set_option("radius_ws_bytes", old)
        qb.close(); tb.close()


# ---- 6. collections ---------------------------------------------------------------------------------------------------------
def _images(nbytes):
    Q, T = HR.data(nbytes)
    assert sum(RC.SIZES) == 1423 <= NT
    cuts = np.cumsum(RC.SIZES)[:-1]
    return Q, [np.ascontiguousarray(im) for im in np.split(T[:1423], cuts)], np.ascontiguousarray(T[1423:1423 + 77])


@pytest.mark.parametrize("nbytes", [32, 17])
def test_collections_equal_the_reference(ctx, nbytes):
    W = 8 * nbytes
    Q, images, extra = _images(nbytes)
    ref = HR.Ref(Q, images)
    assert sum(RC.pad128(n) for n in RC.SIZES) == 1920 and HR.sweep_splits(NQ, 1920)[0] > 1
    qb = ctx.bank_binary(Q)
    with ctx.collection() as c:
        for im in images:
            c.add_binary(im)
        mixed = HR.mixed_radii(ref)
        for r in (np.float32(3), np.float32(W / 2 + 1), INF, mixed):
            want = ref.cut(r)
            HR.same_coll_lists(c.hamming_radius_match(qb, r), want, "host form")
            HR.same_coll_lists(_full_dev(ctx, qb, c, r), want, "device form")
        assert np.array_equal(np.diff(c.hamming_radius_match(qb, INF)[0]), np.full(NQ, 1423))      # padding masked by index
        rc, tot, off = _raw(ctx, qb, c, INF, 0, lists=False)[:3]
        assert rc == 0 and tot == NQ * 1423 and off[-1] == tot
        # cap inside a row, collection form: whole rows only, img beside idx and dist
        woff, wimg, widx, wdist = ref.cut(np.float32(3))[:4]
        row = int(np.nonzero(np.diff(woff) >= 2)[0][30])
        k = int(woff[row])
        rc, tot, off, img, idx, dist = _raw(ctx, qb, c, np.float32(3), k + 1, size=int(woff[-1]))
        assert rc == 0 and tot == woff[-1] and np.array_equal(off, woff)
        assert np.array_equal(img[:k], wimg[:k]) and np.array_equal(idx[:k], widx[:k]) and np.array_equal(HR.bits(dist[:k]), HR.bits(wdist[:k]))
        assert (img[k:] == S_IMG).all() and (idx[k:] == S_IDX).all() and (dist[k:] == np.float32(S_DIST)).all()
        c.add_binary(extra)                                               # one more image after a match
        ref2 = HR.Ref(Q, images + [extra])
        for r in (np.float32(W / 2 + 1), INF):
            HR.same_coll_lists(c.hamming_radius_match(qb, r), ref2.cut(r), "after another add")
    qb.close()


def test_empty_collections_and_empty_images(ctx):
    Q, _ = HR.data(32)
    qb, q0 = ctx.bank_binary(Q), ctx.bank_binary(Q[:0])
    for imgs in ([], [Q[:0], Q[:0]]):
        with ctx.collection() as c:
            for im in imgs:
                c.add_binary(im)
            for r in (INF, np.full(NQ, np.inf, np.float32)):
                off, img, idx, dist = c.hamming_radius_match(qb, r)
                assert off.shape == (NQ + 1,) and not off.any() and img.size == idx.size == dist.size == 0
            n, off = _call_dev(ctx, qb, c, INF, 0, lists=False)[:2]
            assert n == 0 and not off.any()
    with ctx.collection() as c:
        c.add_binary(Q[:40])
        off, img, idx, dist = c.hamming_radius_match(q0, INF)             # nq = 0
        assert off.shape == (1,) and off[0] == 0 and img.size == 0
    qb.close(); q0.close()


# ---- 7. error order ---------------------------------------------------------------------------------------------------------
def test_errors_in_their_order_leave_the_context_working(ctx, std32):
    torch = _torch()
    qb, tb, ref = std32
    Q, T = HR.data(32)
    lib, P = ctx.lib, ctypes.c_void_p
    other = fastmatch_amd.Context(0)
    i8 = ctx.bank(Q)                                                      # a uint8 [n, 32] L2 bank of the same dim
    i8e, bine = ctx.bank(np.zeros((0, 32), np.uint8)), ctx.bank_binary(np.zeros((0, 32), np.uint8))
    narrow = ctx.bank_binary(np.ascontiguousarray(Q[:, :31]))             # same K steps, another width
    narrow16 = ctx.bank_binary(np.ascontiguousarray(Q[:, :16]))
    off = np.zeros(NQ + 1, np.int64)
    idx, dist = np.zeros(8, np.int32), np.zeros(8, np.float32)
    d_off = torch.zeros(NQ + 1, dtype=torch.int64, device="cuda")
    d_idx, d_dist = torch.zeros(8, dtype=torch.int32, device="cuda"), torch.zeros(8, dtype=torch.float32, device="cuda")
    d_img = torch.zeros(8, dtype=torch.int32, device="cuda")
    d_rad = torch.ones(NQ, dtype=torch.float32, device="cuda")
    h_rad = np.ones(NQ, np.float32)
    p = lambda a: a.ctypes.data_as(P)                                     # noqa: E731
    dp = lambda t: P(t.data_ptr())                                        # noqa: E731
    NS = P(-1)                                                            # FM_NO_STREAM

    def pair(form, q, t, cap, o, i, d, rad=None):
        if form == "host":
            return lib.fm_hamming_radius_match(ctx.handle, q, t, rad, 3.0, cap, o, i, d, None)
        return lib.fm_hamming_radius_match_dev(ctx.handle, q, t, rad, 3.0, cap, o, i, d, None, NS)

    def refused(rc, word):
        assert rc == EINVAL, rc
        msg = lib.fm_last_error(ctx.handle).decode()
        assert word in msg, msg

    torch.cuda.synchronize()
    for form, o, i, d in (("host", p(off), p(idx), p(dist)), ("dev", dp(d_off), dp(d_idx), dp(d_dist))):
        name = "fm_hamming_radius_match" + ("_dev" if form == "dev" else "")
        # 1. NULL handles (check_pair; a bank carries no owner, so there is no foreign bank to refuse) -- in front of
        # everything else: the other arguments are wrong too
        refused(pair(form, None, tb.handle, -1, None, None, None), "NULL")
        refused(pair(form, qb.handle, None, -1, None, None, None), "NULL")
        # 2. a bank that is not binary, even an empty one -- in front of the width and cap checks
        for a, b in ((i8.handle, tb.handle), (qb.handle, i8.handle), (i8.handle, i8.handle), (i8e.handle, tb.handle),
                     (qb.handle, i8e.handle), (i8e.handle, i8e.handle)):
            refused(pair(form, a, b, -1, None, None, None), "binary")
        refused(pair(form, i8.handle, i8.handle, 0, o, None, None), "fm_radius_match")
        # 3. widths -- in front of cap
        refused(pair(form, narrow.handle, tb.handle, -1, None, None, None), "mismatch")
        refused(pair(form, qb.handle, narrow16.handle, -1, None, None, None), "mismatch")
        # 4. cap < 0 -- in front of offsets; 5. offsets NULL -- in front of the lists; 6. lists NULL with cap > 0
        refused(pair(form, qb.handle, tb.handle, -1, None, None, None), "cap")
        refused(pair(form, qb.handle, tb.handle, 8, None, None, None), "offsets")
        refused(pair(form, qb.handle, tb.handle, 8, o, None, d), "idx")
        refused(pair(form, qb.handle, tb.handle, 8, o, i, None), "dist")
        assert name in lib.fm_last_error(ctx.handle).decode()
        assert pair(form, qb.handle, tb.handle, 0, o, None, None) == 0    # NULL lists with cap = 0: a counts call
        assert pair(form, bine.handle, tb.handle, 0, o, None, None) == 0  # an empty BINARY bank is valid
    # 7. the device-pointer checks: host memory where device memory is due (checked, never dereferenced)
    refused(pair("dev", qb.handle, tb.handle, 8, dp(d_off), dp(d_idx), dp(d_dist), rad=p(h_rad)), "d_radius")
    refused(pair("dev", qb.handle, tb.handle, 8, p(off), dp(d_idx), dp(d_dist), rad=dp(d_rad)), "d_offsets")
    refused(pair("dev", qb.handle, tb.handle, 8, dp(d_off), p(idx), dp(d_dist)), "d_idx")
    refused(pair("dev", qb.handle, tb.handle, 8, dp(d_off), dp(d_idx), p(dist)), "d_dist")

    # the collection forms
    def coll(form, c, q, cap, o, im, i, d, rad=None):
        if form == "host":
            return lib.fm_collection_hamming_radius_match(ctx.handle, c, q, rad, 3.0, cap, o, im, i, d, None)
        return lib.fm_collection_hamming_radius_match_dev(ctx.handle, c, q, rad, 3.0, cap, o, im, i, d, None, NS)

    img = np.zeros(8, np.int32)
    with ctx.collection() as cb, ctx.collection() as cl, ctx.collection() as ce, other.collection() as cf:
        cb.add_binary(T[:200])
        cl.add(T[:200])                                                   # an L2 collection of the same width
        for form, o, im, i, d in (("host", p(off), p(img), p(idx), p(dist)), ("dev", dp(d_off), dp(d_img), dp(d_idx), dp(d_dist))):
            # 1. coll_query_check: NULL handles, a query of another kind or width -- in front of the output checks
            refused(coll(form, None, qb.handle, -1, None, None, None, None), "NULL")
            refused(coll(form, cb.handle, None, -1, None, None, None, None), "NULL")
            refused(coll(form, cf.handle, qb.handle, -1, None, None, None, None), "another context")
            refused(coll(form, cb.handle, i8.handle, -1, None, None, None, None), "kind")
            refused(coll(form, cb.handle, narrow16.handle, -1, None, None, None, None), "width")
            # 2. rows of another kind: an L2 collection (with an L2 query, or an empty one), an L2 query of an empty collection
            refused(coll(form, cl.handle, i8.handle, -1, None, None, None, None), "binary")
            refused(coll(form, cl.handle, i8e.handle, -1, None, None, None, None), "binary")
            refused(coll(form, ce.handle, i8.handle, -1, None, None, None, None), "binary")
            # 3. the output checks
            refused(coll(form, cb.handle, qb.handle, -1, None, None, None, None), "cap")
            refused(coll(form, cb.handle, qb.handle, 8, None, None, None, None), "offsets")
            refused(coll(form, cb.handle, qb.handle, 8, o, None, i, d), "img")
            refused(coll(form, cb.handle, qb.handle, 8, o, im, None, d), "idx")
            refused(coll(form, cb.handle, qb.handle, 8, o, im, i, None), "dist")
            assert coll(form, cb.handle, qb.handle, 0, o, None, None, None) == 0
            assert coll(form, ce.handle, qb.handle, 0, o, None, None, None) == 0      # an empty collection, a binary query
        refused(coll("dev", cb.handle, qb.handle, 8, dp(d_off), dp(d_img), dp(d_idx), dp(d_dist), rad=p(h_rad)), "d_radius")
        refused(coll("dev", cb.handle, qb.handle, 8, p(off), dp(d_img), dp(d_idx), dp(d_dist)), "d_offsets")
        refused(coll("dev", cb.handle, qb.handle, 8, dp(d_off), p(img), dp(d_idx), dp(d_dist)), "d_img")
        # the L2-named calls keep refusing binary data, and say where to go
        assert lib.fm_collection_radius_match(ctx.handle, cb.handle, qb.handle, None, 3.0, 0, p(off), None, None, None, None) == -4
        assert "fm_collection_hamming_radius_match" in lib.fm_last_error(ctx.handle).decode()
    assert lib.fm_radius_match(ctx.handle, qb.handle, tb.handle, None, 3.0, 0, p(off), None, None, None) == -4
    assert "binary" in lib.fm_last_error(ctx.handle).decode()
    # the context still answers
    ridx, rdist = ctx.knn2(qb, tb)
    assert np.array_equal(ridx[:, 0], ref.order[:, 0]) and np.array_equal(HR.bits(rdist[:, 1]), HR.bits(ref.sorted[:, 1]))
    HR.same_pair_lists(ctx.hamming_radius_match(qb, tb, np.float32(3)), ref.cut(np.float32(3)), "after the refusals")
    for b in (i8, i8e, bine, narrow, narrow16):
        b.close()
    other.close()


# ---- 8. Python surfaces -----------------------------------------------------------------------------------------------------
def test_matchutil_on_arrays_and_on_resident_banks(ctx, std32):
    qb, tb, ref = std32
    Q, T = HR.data(32)
    opts = {"context": ctx}
    radii = HR.mixed_radii(ref)
    for r in (np.float32(3), 129.0, radii):
        want = ref.cut(r)
        HR.same_pair_lists(matchutil.hamming_radius_match_arrays(Q, T, r, options=opts), want, "arrays")
        HR.same_pair_lists(matchutil.hamming_radius_match_arrays(qb, tb, r, options=opts), want, "banks")
        HR.same_pair_lists(matchutil.hamming_radius_match_arrays(Q, tb, r, options=opts), want, "array against bank")
    woff, _, _, wdist, wglobal = ref.cut(np.float32(3))
    lists = matchutil.hamming_radius_match(Q, T, 3.0, options=opts)
    assert len(lists) == NQ and [len(l) for l in lists] == list(np.diff(woff))
    flat = [m for l in lists for m in l]
    assert [m.trainIdx for m in flat] == list(wglobal) and [m.distance for m in flat] == list(wdist)
    assert all(m.queryIdx == i for i, l in enumerate(lists) for m in l)
    with pytest.raises(ValueError, match="radiusMatch"):                  # the L2-named call keeps refusing
        matchutil.bf_radius_match(Q, T, 3.0, options={"context": ctx, "normType": matchutil.NORM_HAMMING})
    l2 = ctx.bank(Q)
    with pytest.raises(ValueError, match="binary"):
        matchutil.hamming_radius_match_arrays(l2, tb, 3.0, options=opts)
    l2.close()


def test_torchmatch_with_a_tensor_of_radii(ctx, std32):
    torch = _torch()
    qb, tb, ref = std32
    Q, T = HR.data(32)
    radii = HR.mixed_radii(ref)
    tq, tt, tr = _dev(Q), _dev(T), _dev(radii)

    def host(out):
        return tuple(x.cpu().numpy() for x in out)

    HR.same_pair_lists(host(torchmatch.hamming_radius_match(tq, tt, tr)), ref.cut(radii), "tensors, tensor of radii")
    HR.same_pair_lists(host(torchmatch.hamming_radius_match(qb, tt, 3.0)), ref.cut(np.float32(3)), "bank and tensor, scalar")
    out = torchmatch.hamming_radius_match(tq, tt, np.inf)
    assert all(x.is_cuda for x in out) and out[0].dtype == torch.int64 and out[1].dtype == torch.int32 and out[2].dtype == torch.float32
    Qc, images, _ = _images(32)
    cref = HR.Ref(Qc, images)
    with torchmatch.Collection(context=ctx) as c:
        for im in images:
            c.add(_dev(im), binary=True)
        HR.same_coll_lists(host(c.hamming_radius_match(tq, tr)), cref.cut(radii), "collection, tensor of radii")
        HR.same_coll_lists(host(c.hamming_radius_match(qb, np.inf)), cref.cut(INF), "collection, +inf")
    for bad, word in ((lambda: torchmatch.hamming_radius_match(tq.float(), tt, 3.0), "uint8"),
                      (lambda: torchmatch.hamming_radius_match(tq[:, :16], tt, 3.0), "bytes"),
                      (lambda: torchmatch.hamming_radius_match(tq, tt, tr[:10]), "radii"),
                      (lambda: torchmatch.hamming_radius_match(tq, tt, tr.cpu()), "CUDA")):
        with pytest.raises(ValueError, match=word):
            bad()


def test_host_forms_are_accounted_with_the_real_rows(ctx, std32):
    qb, tb, ref = std32
    before = ctx.stats()
    assert _raw(ctx, qb, tb, np.float32(3), 0, lists=False)[0] == 0
    after = ctx.stats()
    assert after["calls"] - before["calls"] == 1 and after["pairs"] - before["pairs"] == NQ * NT
    Q, images, _ = _images(32)
    with ctx.collection() as c:
        for im in images:
            c.add_binary(im)
        c.train()
        before = ctx.stats()
        assert _raw(ctx, qb, c, np.float32(3), 0, lists=False)[0] == 0
        after = ctx.stats()
        assert after["calls"] - before["calls"] == 1 and after["pairs"] - before["pairs"] == NQ * 1423
        before = ctx.stats()
        _call_dev(ctx, qb, c, np.float32(3), 0, lists=False)               # the device forms are not accounted
        assert ctx.stats()["pairs"] == before["pairs"]
