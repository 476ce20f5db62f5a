"""GPU: radiusMatch of a wide float query bank against a WIDE train collection (129 .. 256 values per row) --
fm_collection_wide_radius_match, fm_collection_wide_radius_match_dev, torchmatch.Collection.wide_radius_match.

Every result is compared bit for bit with the reference (tests/wide_radius_ref.py: oracle.bf_knn with k = all rows on the
concatenated images, cut at dist < r_i, global rows turned into (image, row) through the cumulative image sizes): offsets,
img, idx and the distances as uint32 bit patterns.  The layout is radius_coll_ref.SIZES: padding rows behind every image whose
size is no multiple of 128, an empty image, a split of the sweep inside an image; r = +inf is the case that catches a
padding row let through."""
import ctypes

import numpy as np
import pytest

import fastmatch_amd
from fastmatch_amd import _ffi
import f16_margin_ref as F
import wide_radius_ref as WR
import wide_ref

pytestmark = pytest.mark.gpu

P = ctypes.c_void_p
EINVAL, EUNSUPPORTED = -1, -4
REAL = sum(WR.SIZES)            # 1423 real rows in 1920 physical ones


def _ptr(a):
    return a.ctypes.data_as(P)


def _torch():
    import torch
    return torch


def _dev(a):
    return _torch().from_numpy(np.array(a, order="C")).cuda()


def _collection(ctx, images):
    c = ctx.collection()
    for i, im in enumerate(images):
        assert c.add_wide(im) == i
    return c


def _swept(ctx, l0, calls):
    """fm_f32_filter_stats counts one launch per C call that ran the fp16 sweep; a Python call is a counts call and, when
    there are entries, a fill call."""
    return calls <= ctx.f32_filter_stats()[0] - l0 <= 2 * calls


def _pad128(n):
    return (n + 127) // 128 * 128


@pytest.fixture(scope="module", params=[129, 256])
def std(ctx, request):
    """(dim, query bank, collection, reference, Q, images) of the standard layout; every test leaves the collection unchanged."""
    dim = request.param
    Q, T = wide_ref.clustered(WR.NQ, REAL, dim, 50 + dim)
    images = WR.split_images(T)
    qb, c = ctx.bank(Q), _collection(ctx, images)
    assert c.info() == (len(WR.SIZES), REAL, dim, _ffi.FM_BANK_F32W) and sum(_pad128(n) for n in WR.SIZES) == 1920
    yield dim, qb, c, WR.Ref(Q, images), Q, images
    c.close()
    qb.close()


def test_layout_puts_a_split_boundary_inside_a_stage():
    # the wide sweep: 128 query rows per workgroup, ~2048 workgroups, a split of at least 1024 train rows, whole 64-row stages
    qg = (WR.NQ + 127) // 128
    s = max(1, min((2048 + qg - 1) // qg, (1920 + 1023) // 1024, 65535))
    per = ((1920 + s - 1) // s + 63) // 64 * 64
    assert (s, per) == (2, 960) and per % 128 == 64
    first = np.concatenate([[0], np.cumsum([_pad128(n) for n in WR.SIZES])])
    assert first[5] == 768 and first[6] == 1024        # ... of the 129-row image, whose second stage [896, 1024) holds one real row


def test_scalar_per_row_and_infinite_radius(ctx, std):
    dim, qb, c, ref, _, _ = std
    r = ref.kth(4)
    want = ref.cut(r)
    assert 2 * ref.nq < want[0][-1] < 12 * ref.nq                  # a few hits per row
    l0 = ctx.f32_filter_stats()[0]
    WR.same_lists(c.wide_radius_match(qb, r), want, "scalar")
    rows = WR.mixed_radii(ref)
    assert np.isnan(rows).any() and np.isinf(rows).any() and (rows == 0).any() and (rows < 0).any()
    WR.same_lists(c.wide_radius_match(qb, rows), ref.cut(rows), "per row")
    got = c.wide_radius_match(qb, np.inf)
    assert _swept(ctx, l0, 3)                                       # the fp16 sweep, in each of the three calls
    assert np.array_equal(np.diff(got[0]), np.full(ref.nq, REAL))   # exactly the real rows: no padding row, behind no image
    WR.same_lists(got, ref.cut(np.inf), "r = inf")
    for r in (0.0, -1.0, np.nan, -np.inf):
        off, img, idx, dist = c.wide_radius_match(qb, np.float32(r))
        assert not off.any() and img.size == idx.size == dist.size == 0
    # a per-row radius overrides radius_all: the C call with both
    off = np.zeros(ref.nq + 1, np.int64)
    tot = ctypes.c_int64(-1)
    rc = ctx.lib.fm_collection_wide_radius_match(ctx.handle, c.handle, qb.handle, _ptr(rows), 1e9, 0, _ptr(off), None, None, None,
                                                 ctypes.byref(tot))
    assert rc == 0 and np.array_equal(off, ref.cut(rows)[0]) and tot.value == off[-1]
    # the plain pair of the stacked real rows gives the same lists by global row
    tb = ctx.bank(np.concatenate([im for im in std[5]]))
    try:
        WR.same_pair(ctx.wide_radius_match(qb, tb, rows), ref.cut(rows), "the stacked rows as one bank")
    finally:
        tb.close()


def _raw(c, qb, r, cap, nq, size, with_lists=True):
    """The C call with sentinel-filled arrays of `size` entries: (rc, offsets, img, idx, dist, n_total)."""
    off = np.full(nq + 1, -7, np.int64)
    img, idx = np.full(size, -77, np.int32), np.full(size, -78, np.int32)
    dist = np.full(size, -79.0, np.float32)
    tot = ctypes.c_int64(-1)
    rows = None if np.ndim(r) == 0 else np.ascontiguousarray(r, np.float32)
    rc = c.ctx.lib.fm_collection_wide_radius_match(c.ctx.handle, c.handle, qb.handle, _ptr(rows) if rows is not None else None,
                                                   float(np.float32(r)) if rows is None else 0.0, cap, _ptr(off),
                                                   _ptr(img) if with_lists else None, _ptr(idx) if with_lists else None,
                                                   _ptr(dist) if with_lists else None, ctypes.byref(tot))
    return rc, off, img, idx, dist, tot.value


def test_cap_chunks_and_the_prefix_of_whole_rows(ctx, std):
    dim, qb, c, ref, _, _ = std
    r = WR.mixed_radii(ref, 4)
    woff, wimg, widx, wdist, _ = ref.cut(r)
    total = int(woff[-1])
    rc, off, _, _, _, tot = _raw(c, qb, r, 0, ref.nq, 1, with_lists=False)          # counts only, NULL lists
    assert rc == 0 and np.array_equal(off, woff) and tot == total
    k = ref.nq // 2 + int(np.argmax(np.diff(woff)[ref.nq // 2:] > 1))
    assert 0 < woff[k] < total and woff[k + 1] - woff[k] > 1
    old = ctx.get_option("radius_ws_bytes")
    try:
        for ws in (old, 65536):                                                      # 65536: 2340 candidates (28 B each) per chunk
            ctx.set_option("radius_ws_bytes", ws)
            for cap in (total - 1, int(woff[k]) + 1, total):                         # woff[k] + 1 cuts inside row k
                rc, off, img, idx, dist, tot = _raw(c, qb, r, cap, ref.nq, total + 5)
                assert rc == 0 and np.array_equal(off, woff) and tot == total
                m = int(woff[np.searchsorted(woff, cap, side="right") - 1])         # the longest prefix of whole rows within cap
                assert m <= cap and (cap < total) == (m < total)
                assert np.array_equal(img[:m], wimg[:m]) and np.array_equal(idx[:m], widx[:m])
                assert np.array_equal(WR.bits(dist[:m]), WR.bits(wdist[:m]))
                assert np.all(img[m:] == -77) and np.all(idx[m:] == -78) and np.all(dist[m:] == -79.0), "written beyond the prefix"
            if ws == 65536:
                for rr in (ref.kth(4), np.inf):
                    WR.same_lists(c.wide_radius_match(qb, rr), ref.cut(rr), "chunked")
    finally:
        ctx.set_option("radius_ws_bytes", old)
    before = ctx.stats()
    _raw(c, qb, np.float32(ref.kth(2)), 0, ref.nq, 1, with_lists=False)
    after = ctx.stats()
    assert after["calls"] - before["calls"] == 1 and after["pairs"] - before["pairs"] == ref.nq * REAL


def test_device_form_equals_the_host_form(ctx, std):
    torch = _torch()
    dim, qb, c, ref, _, _ = std
    rows = WR.mixed_radii(ref, 6)

    def call(r, cap, size=None, lists=True, want_total=True, stream="current"):
        size = cap if size is None else size
        off = torch.full((qb.n + 1,), -7, dtype=torch.int64, device="cuda")
        img = torch.full((size,), -77, dtype=torch.int32, device="cuda")
        idx = torch.full((size,), -78, dtype=torch.int32, device="cuda")
        dist = torch.full((size,), -79.0, dtype=torch.float32, device="cuda")
        rt, r_all = (r, 0.0) if isinstance(r, torch.Tensor) else (None, float(np.float32(r)))
        s = torch.cuda.current_stream().cuda_stream if stream == "current" else stream
        if stream is None:
            torch.cuda.synchronize()
        p = (lambda t: t.data_ptr()) if lists and size else (lambda t: 0)
        n = c.wide_radius_match_dev(qb, rt.data_ptr() if rt is not None else 0, r_all, cap, off.data_ptr(), p(img), p(idx), p(dist),
                                    want_total=want_total, consumer_stream=s)
        if stream is None:
            ctx.sync()
        return n, off.cpu().numpy(), img.cpu().numpy(), idx.cpu().numpy(), dist.cpu().numpy()

    d_rows = _dev(rows)
    for r, want_r in ((float(ref.kth(4)), ref.kth(4)), (d_rows, rows), (np.float32(np.inf), np.inf)):
        want = ref.cut(want_r)
        n0, off0 = call(r, 0, lists=False)[:2]
        assert n0 == want[0][-1] and np.array_equal(off0, want[0])
        for stream in ("current", None):
            n, off, img, idx, dist = call(r, n0, stream=stream)
            assert n == n0
            WR.same_lists((off, img, idx, dist), want, ("device form", stream))
        host = c.wide_radius_match(qb, want_r)
        WR.same_lists((off, img, idx, dist), (host[0], host[1], host[2], host[3]), "device form against the host form")
    # n_total NULL; a cap that cuts inside a row, across chunks
    want = ref.cut(rows)
    total = int(want[0][-1])
    n, off, img, idx, dist = call(d_rows, total, want_total=False)
    assert n is None
    WR.same_lists((off, img, idx, dist), want, "n_total NULL")
    old = ctx.get_option("radius_ws_bytes")
    try:
        ctx.set_option("radius_ws_bytes", 65536)
        k = ref.nq // 2 + int(np.argmax(np.diff(want[0])[ref.nq // 2:] > 1))
        cap, m = int(want[0][k]) + 1, int(want[0][k])
        n, off, img, idx, dist = call(d_rows, cap, size=total + 3)
        assert n == total and np.array_equal(off, want[0]) and 0 < m < cap < want[0][k + 1]
        assert np.array_equal(img[:m], want[1][:m]) and np.array_equal(idx[:m], want[2][:m])
        assert np.array_equal(WR.bits(dist[:m]), WR.bits(want[3][:m]))
        assert np.all(img[m:] == -77) and np.all(idx[m:] == -78) and np.all(dist[m:] == -79.0), "written beyond the prefix"
    finally:
        ctx.set_option("radius_ws_bytes", old)
    # torchmatch: a float32 tensor and a bank as the query, a scalar and a device radius tensor
    from fastmatch_amd import torchmatch
    with torchmatch.Collection(context=ctx) as tc:
        for im in std[5]:
            tc.add_wide(_dev(im))
        for q in (_dev(std[4]), qb):
            for r, want_r in ((float(ref.kth(4)), ref.kth(4)), (d_rows, rows)):
                got = tc.wide_radius_match(q, r)
                assert all(x.is_cuda for x in got)
                assert [x.dtype for x in got] == [torch.int64, torch.int32, torch.int32, torch.float32]
                WR.same_lists(tuple(x.cpu().numpy() for x in got), ref.cut(want_r), "torchmatch collection")


def test_an_add_that_lifts_the_stack_scale_and_alternating_host_and_device_adds(ctx):
    torch = _torch()
    dim = 192
    Q, T = wide_ref.clustered(150, 600, dim, 61)
    sizes = [130, 70, 0, 200, 200]
    parts = WR.split_images(T, sizes)
    parts[3] = (parts[3] * np.float32(16.0)).astype(np.float32)     # the fourth image lifts the stack's largest magnitude by 2^4
    assert F.kscale(np.concatenate(parts[:4])) <= F.kscale(np.concatenate(parts[:3])) - 3       # (the stack's fp16 planes are rewritten)
    qb = ctx.bank(Q)
    host = ctx.collection()
    mixed = ctx.collection()
    try:
        for i, im in enumerate(parts):
            assert host.add_wide(im) == i
            if i % 2 == 0:
                assert mixed.add_wide(im) == i
            else:
                d = _dev(im)
                assert mixed.add_wide_from_device(d.data_ptr(), _ffi.FM_DT_F32, im.shape[0], dim, 0,
                                                  stream=torch.cuda.current_stream().cuda_stream) == i
            # the stack's scale and largest norm are read at the call: every state of the growing collection answers
            ref = WR.Ref(Q, parts[:i + 1])
            l0 = ctx.f32_filter_stats()[0]
            for r in (ref.kth(3), WR.mixed_radii(ref, i), np.inf):
                got = host.wide_radius_match(qb, r)
                WR.same_lists(got, ref.cut(r), ("after add", i))
                WR.same_lists(mixed.wide_radius_match(qb, r), got, ("host and device adds", i))
            assert _swept(ctx, l0, 6)                               # (scales 0 or 4 apart: the fp16 sweep)
    finally:
        host.close()
        mixed.close()
        qb.close()


def test_a_value_that_is_not_finite_takes_the_all_pairs_path(ctx):
    dim = 161
    Q, T = wide_ref.nonfinite(140, 500, dim, 71)
    images = WR.split_images(T, [100, 129, 271])
    ref = WR.Ref(Q, images)
    qb = ctx.bank(Q)
    with _collection(ctx, images) as c:
        l0 = ctx.f32_filter_stats()[0]
        for r in (ref.kth(5), WR.mixed_radii(ref, 2), np.inf):
            WR.same_lists(c.wide_radius_match(qb, r), ref.cut(r), "nonfinite")
        assert ctx.f32_filter_stats()[0] == l0
        assert np.diff(ref.cut(np.inf)[0]).max() == 498             # nobody lists the NaN row or the row with an infinite value
    qb.close()


@pytest.mark.parametrize("dim", [129, 256])
def test_planted_threshold_pairs_stacked_behind_small_rows(ctx, dim):
    p = F.radius_set(dim)
    small = F.small_rows(70, dim, 3, scale=0.5)                     # an image of small norm in the planted rows' binade, and its padding
    stacked = F.Planted(np.array(p.Q), np.concatenate([small, p.T]).astype(np.float32), [dict(f, t=f["t"] + 70) for f in p.fams])
    r, _ = F.check_threshold(stacked, eps=F.EPS_K14, floor=0.75)
    images = [small, np.array(p.T)]
    ref = WR.Ref(p.Q, images)
    want = ref.cut(r)
    assert want[0][-1] == 9
    qb = ctx.bank(np.array(p.Q))
    with _collection(ctx, images) as c:
        l0 = ctx.f32_filter_stats()[0]
        off, img, idx, dist = c.wide_radius_match(qb, r)
        assert _swept(ctx, l0, 1)
        for f in p.fams:
            row = list(zip(img[off[f["q"]]:off[f["q"] + 1]].tolist(), idx[off[f["q"]]:off[f["q"] + 1]].tolist()))
            assert ((1, f["t"]) in row) == (f["kind"] == "hit"), f
        WR.same_lists((off, img, idx, dist), want, "planted, stacked")
    qb.close()


def test_degenerate_inputs(ctx, std):
    dim, qb, c, ref, Q, _ = std
    q0 = ctx.bank(np.ascontiguousarray(Q[:0]))
    assert q0.kind == _ffi.FM_BANK_F32W
    off, img, idx, dist = c.wide_radius_match(q0, np.inf)                        # nq = 0
    assert off.shape == (1,) and off[0] == 0 and img.size == idx.size == dist.size == 0
    for imgs in ([], [Q[:0], Q[:0], Q[:0]]):                                      # no add has succeeded; empty images only
        with _collection(ctx, imgs) as e:
            for r in (np.inf, np.full(len(Q), np.inf, np.float32)):
                off, img, idx, dist = e.wide_radius_match(qb, r)
                assert off.shape == (len(Q) + 1,) and not off.any() and img.size == idx.size == dist.size == 0
    q0.close()


def test_errors_in_their_order_leave_the_context_working(ctx, std):
    torch = _torch()
    dim, qb, c, ref, Q, images = std
    lib = ctx.lib
    other = fastmatch_amd.Context(0)
    rng = np.random.default_rng(81)
    f32 = ctx.bank(np.ascontiguousarray(Q[:, :128]), float_route=True)
    f32e = ctx.bank(np.ascontiguousarray(Q[:0, :128]), float_route=True)
    binb = ctx.bank_binary(rng.integers(0, 256, (9, 32), dtype=np.uint8))
    w_other = ctx.bank(np.zeros((4, 130 if dim != 130 else 131), np.float32))
    w_other0 = ctx.bank(np.zeros((0, 200), np.float32))
    nq = qb.n
    off = np.zeros(nq + 1, np.int64)
    img, idx, dist = np.zeros(8, np.int32), np.zeros(8, np.int32), np.zeros(8, np.float32)
    d_off = torch.zeros(nq + 1, dtype=torch.int64, device="cuda")
    d_img, d_idx = torch.zeros(8, dtype=torch.int32, device="cuda"), torch.zeros(8, dtype=torch.int32, device="cuda")
    d_dist = torch.zeros(8, dtype=torch.float32, device="cuda")
    d_rad = torch.ones(nq, dtype=torch.float32, device="cuda")
    h_rad = np.ones(nq, np.float32)
    p = lambda a: a.ctypes.data_as(P)                                     # noqa: E731
    dp = lambda t: P(t.data_ptr())                                        # noqa: E731
    NS = P(-1)                                                            # FM_NO_STREAM

    def coll(form, ch, q, cap, o, im, i, d, rad=None):
        if form == "host":
            return lib.fm_collection_wide_radius_match(ctx.handle, ch, q, rad, 3.0, cap, o, im, i, d, None)
        return lib.fm_collection_wide_radius_match_dev(ctx.handle, ch, q, rad, 3.0, cap, o, im, i, d, None, NS)

    def refused(rc, *words):
        assert rc == EINVAL, rc
        msg = lib.fm_last_error(ctx.handle).decode()
        for w in words:
            assert w in msg, msg

    torch.cuda.synchronize()
    with ctx.collection() as cl, ctx.collection() as cbin, ctx.collection() as ce, other.collection() as cf:
        cl.add(np.ascontiguousarray(Q[:50, :128]))                        # an L2 collection
        cbin.add_binary(rng.integers(0, 256, (50, 32), dtype=np.uint8))
        for form, o, im, i, d in (("host", p(off), p(img), p(idx), p(dist)), ("dev", dp(d_off), dp(d_img), dp(d_idx), dp(d_dist))):
            name = "fm_collection_wide_radius_match" + ("_dev" if form == "dev" else "")
            # 1. NULL handles, a foreign context -- in front of everything else: the other arguments are wrong too
            refused(coll(form, None, qb.handle, -1, None, None, None, None), "NULL")
            refused(coll(form, c.handle, None, -1, None, None, None, None), "NULL")
            refused(coll(form, cf.handle, f32.handle, -1, None, None, None, None), "another context")
            # 2. a bank or a collection that is not wide, even an empty bank; the message names the call that serves it
            refused(coll(form, c.handle, f32.handle, -1, None, None, None, None), "wide", "fm_collection_radius_match is the L2 call")
            refused(coll(form, c.handle, f32e.handle, -1, None, None, None, None), "wide", "fm_collection_radius_match")
            refused(coll(form, cl.handle, qb.handle, -1, None, None, None, None), "wide", "fm_collection_radius_match is the L2 call")
            refused(coll(form, c.handle, binb.handle, -1, None, None, None, None), "fm_collection_hamming_radius_match")
            refused(coll(form, cbin.handle, qb.handle, -1, None, None, None, None), "fm_collection_hamming_radius_match")
            refused(coll(form, ce.handle, f32.handle, -1, None, None, None, None), "wide")       # an empty collection, an L2 query
            # 3. widths -- in front of cap
            refused(coll(form, c.handle, w_other.handle, -1, None, None, None, None), "width")
            refused(coll(form, c.handle, w_other0.handle, -1, None, None, None, None), "width")
            # 4. cap < 0 -- in front of offsets; offsets NULL -- in front of the lists; a list NULL with cap > 0
            refused(coll(form, c.handle, qb.handle, -1, None, None, None, None), "cap")
            refused(coll(form, c.handle, qb.handle, 8, None, None, None, None), "offsets")
            refused(coll(form, c.handle, qb.handle, 8, o, None, i, d), "img")
            refused(coll(form, c.handle, qb.handle, 8, o, im, None, d), "idx")
            refused(coll(form, c.handle, qb.handle, 8, o, im, i, None), "dist")
            assert name in lib.fm_last_error(ctx.handle).decode()
            assert coll(form, c.handle, qb.handle, 0, o, None, None, None) == 0          # NULL lists with cap = 0: a counts call
            assert coll(form, ce.handle, qb.handle, 0, o, None, None, None) == 0         # no add has succeeded: valid, all-zero offsets
            assert coll(form, ce.handle, w_other0.handle, 0, o, None, None, None) == 0   # ... which has no width yet
        ctx.sync()
        assert not d_off.cpu().numpy()[:1].any()
        # 5. the device-pointer checks: host memory where device memory is due (checked, never dereferenced)
        refused(coll("dev", c.handle, qb.handle, 8, dp(d_off), dp(d_img), dp(d_idx), dp(d_dist), rad=p(h_rad)), "d_radius")
        refused(coll("dev", c.handle, qb.handle, 8, p(off), dp(d_img), dp(d_idx), dp(d_dist), rad=dp(d_rad)), "d_offsets")
        refused(coll("dev", c.handle, qb.handle, 8, dp(d_off), p(img), dp(d_idx), dp(d_dist)), "d_img")
        refused(coll("dev", c.handle, qb.handle, 8, dp(d_off), dp(d_img), p(idx), dp(d_dist)), "d_idx")
        refused(coll("dev", c.handle, qb.handle, 8, dp(d_off), dp(d_img), dp(d_idx), p(dist)), "d_dist")
        # the L2-named and the Hamming calls keep refusing a wide collection, and say "wide"
        assert lib.fm_collection_radius_match(ctx.handle, c.handle, qb.handle, None, 3.0, 0, p(off), None, None, None, None) == EUNSUPPORTED
        assert "wide" in lib.fm_last_error(ctx.handle).decode()
        assert lib.fm_collection_radius_match_dev(ctx.handle, c.handle, qb.handle, None, 3.0, 0, dp(d_off), None, None, None, None, NS) == EUNSUPPORTED
        assert "wide" in lib.fm_last_error(ctx.handle).decode()
        assert lib.fm_collection_hamming_radius_match(ctx.handle, c.handle, qb.handle, None, 3.0, 0, p(off), None, None, None, None) != 0
    # the context still answers
    WR.same_lists(c.wide_radius_match(qb, ref.kth(2)), ref.cut(ref.kth(2)), "after the refusals")
    for b in (f32, f32e, binb, w_other, w_other0):
        b.close()
    other.close()
