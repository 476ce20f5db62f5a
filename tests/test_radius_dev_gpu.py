"""GPU: radiusMatch with the radii read from and the lists left in device memory -- fm_radius_match_dev,
fm_collection_radius_match_dev, torchmatch.radius_match, torchmatch.Collection.radius_match.

Every result is compared bit for bit with BOTH the oracle lists (tests/radius_coll_ref.py: oracle.bf_knn with k = all rows on
the concatenated images, cut at dist < r_i) and the host forms (Context.radius_match, Collection.radius_match) on the same
banks, on the integer and the float32 route."""
import ctypes

import numpy as np
import pytest

import fastmatch_amd
from fastmatch_amd import _ffi, torchmatch
import radius_coll_ref as RC

pytestmark = pytest.mark.gpu

EINVAL = -1
S_OFF, S_IMG, S_IDX, S_DIST = -7, -77, -78, -79.0          # sentinels


def _torch():
    import torch
    return torch


def _dev(a):
    return _torch().from_numpy(np.array(a, order="C")).cuda()


def _qbank(ctx, Q, route):
    return ctx.bank(Q, float_route=route == "f32")


@pytest.fixture(scope="module", params=RC.ROUTES)
def std(ctx, request):
    """(route, query bank, plain train bank of the stacked real rows, collection, reference) of the standard layout."""
    route = request.param
    Q, images = RC.layout(route)
    qb, tb = _qbank(ctx, Q, route), _qbank(ctx, np.concatenate(images), route)
    c = ctx.collection()
    for im in images:
        c.add(im)
    yield route, qb, tb, c, RC.layout_ref(route)
    c.close()
    tb.close()
    qb.close()


def _call(ctx, qb, target, r, cap, size=None, stream="current", lists=True):
    """One device call into sentinel-filled tensors.  target: a Bank (fm_radius_match_dev) or a Collection.  r: a scalar, a NumPy
    array (uploaded here) or a CUDA tensor.  Returns (n_total, offsets, img or None, idx, dist) as NumPy arrays."""
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
    s = torch.cuda.current_stream().cuda_stream if stream == "current" else stream
    if stream is None:
        torch.cuda.synchronize()                      # FM_NO_STREAM: the caller says the arrays are ready
    p = (lambda t: t.data_ptr()) if lists and size else (lambda t: 0)
    rp = rt.data_ptr() if rt is not None else 0
    if coll:
        n = target.radius_match_dev(qb, rp, r_all, cap, off.data_ptr(), p(img), p(idx), p(dist), consumer_stream=s)
    else:
        n = ctx.radius_match_dev(qb, target, rp, r_all, cap, off.data_ptr(), p(idx), p(dist), consumer_stream=s)
    if stream is None:
        ctx.sync()
    return n, off.cpu().numpy(), (img.cpu().numpy() if coll else None), idx.cpu().numpy(), dist.cpu().numpy()


def _full(ctx, qb, target, r, **kw):
    """Counts call, then fill call: (offsets, [img,] idx, dist)."""
    n0, off0 = _call(ctx, qb, target, r, 0, lists=False, **kw)[:2]
    assert n0 == off0[-1]
    n, off, img, idx, dist = _call(ctx, qb, target, r, n0, **kw)
    assert n == n0 and np.array_equal(off, off0)
    return (off, img, idx, dist) if img is not None else (off, idx, dist)


def _same_pair(got, ref, r, host):
    off, idx, dist = got
    woff, _, _, wdist, wglobal = ref.cut(r)
    assert np.array_equal(off, woff) and np.array_equal(idx, wglobal) and np.array_equal(RC.bits(dist), RC.bits(wdist))
    for g, h in zip(got, host):
        assert g.dtype == h.dtype and np.array_equal(RC.bits(g) if g.dtype == np.float32 else g, RC.bits(h) if h.dtype == np.float32 else h)


def test_device_forms_equal_the_oracle_and_the_host_forms(ctx, std):
    route, qb, tb, c, ref = std
    for r in (ref.kth(4), RC.mixed_radii(ref), np.inf):
        _same_pair(_full(ctx, qb, tb, r), ref, r, ctx.radius_match(qb, tb, r))
        got = _full(ctx, qb, c, r)
        RC.same_lists(got, ref.cut(r), "collection, device form")
        RC.same_lists(got, c.radius_match(qb, r), "collection, device form against the host form")
    for r in (0.0, np.nan, -2.0):                              # no entries: the offsets are still written
        for target in (tb, c):
            n, off = _call(ctx, qb, target, np.float32(r), 0, lists=False)[:2]
            assert n == 0 and not off.any()


def test_radii_from_a_kernel_on_the_current_stream_without_synchronize(ctx, std):
    """d_radius = tau * selfdist computed by torch kernels on a side stream immediately before the call, no synchronize()
    in between; the results are read on the same stream."""
    torch = _torch()
    route, qb, tb, c, ref = std
    sd = ctx.self_dist(qb)
    tau = 1.05
    want_r = (tau * sd).astype(np.float32)
    side = torch.cuda.Stream()
    sd_t = _dev(sd)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        a = torch.ones((1024, 1024), device="cuda")
        for _ in range(8):                                     # work in front of the radii on the stream
            a = (a @ a) * 1e-3
        rad = (tau * sd_t + 0.0 * a[0, 0].double()).float()
        got_c = _full(ctx, qb, c, rad)
        got_p = _full(ctx, qb, tb, rad)
    assert ref.cut(want_r)[0][-1] > ref.nq                     # the query rows' own neighbourhoods: not an empty case
    RC.same_lists(got_c, ref.cut(want_r), "stream, collection")
    _same_pair(got_p, ref, want_r, ctx.radius_match(qb, tb, want_r))
    # FM_NO_STREAM, then ctx.sync()
    got_c = _full(ctx, qb, c, rad, stream=None)
    RC.same_lists(got_c, ref.cut(want_r), "no stream, collection")
    _same_pair(_full(ctx, qb, tb, rad, stream=None), ref, want_r, ctx.radius_match(qb, tb, want_r))


def test_host_pointers_are_refused_and_null_lists_pass_with_cap_0(ctx, std):
    torch = _torch()
    route, qb, tb, c, ref = std
    nq = qb.n
    h_r, h_off, h_idx = np.ones(nq, np.float32), np.zeros(nq + 1, np.int64), np.zeros(64, np.int32)
    d_r = _dev(np.full(nq, ref.kth(2), np.float32))
    d_off = torch.zeros(nq + 1, dtype=torch.int64, device="cuda")
    d_img = torch.zeros(64, dtype=torch.int32, device="cuda")
    d_idx = torch.zeros(64, dtype=torch.int32, device="cuda")
    d_dist = torch.zeros(64, dtype=torch.float32, device="cuda")
    good = dict(r=d_r.data_ptr(), off=d_off.data_ptr(), idx=d_idx.data_ptr())
    for bad in (dict(r=h_r.ctypes.data), dict(off=h_off.ctypes.data), dict(idx=h_idx.ctypes.data)):
        a = dict(good, **bad)
        for call in (lambda: ctx.radius_match_dev(qb, tb, a["r"], 0.0, 64, a["off"], a["idx"], d_dist.data_ptr(), consumer_stream=None),
                     lambda: c.radius_match_dev(qb, a["r"], 0.0, 64, a["off"], d_img.data_ptr(), a["idx"], d_dist.data_ptr(),
                                                consumer_stream=None)):
            with pytest.raises(fastmatch_amd.FastMatchHipError) as e:
                call()
            assert e.value.code == EINVAL and "device memory" in str(e.value)
    # NULL lists with cap = 0 are a counts call; with cap > 0 they are refused
    want = ref.cut(np.float32(ref.kth(2)))[0]
    assert ctx.radius_match_dev(qb, tb, d_r.data_ptr(), 0.0, 0, d_off.data_ptr(), 0, 0, consumer_stream=None) == want[-1]
    ctx.sync()
    assert np.array_equal(d_off.cpu().numpy(), want)
    assert c.radius_match_dev(qb, d_r.data_ptr(), 0.0, 0, d_off.data_ptr(), 0, 0, 0, consumer_stream=None) == want[-1]
    ctx.sync()
    assert np.array_equal(d_off.cpu().numpy(), want)
    with pytest.raises(fastmatch_amd.FastMatchHipError) as e:
        ctx.radius_match_dev(qb, tb, d_r.data_ptr(), 0.0, 8, d_off.data_ptr(), 0, 0, consumer_stream=None)
    assert e.value.code == EINVAL
    with pytest.raises(fastmatch_amd.FastMatchHipError) as e:
        c.radius_match_dev(qb, 0, 1.0, -1, d_off.data_ptr(), 0, 0, 0, consumer_stream=None)
    assert e.value.code == EINVAL


def test_prefix_of_whole_rows_across_chunks(ctx, std):
    """cap below the total: the full offsets and n_total, the rows of the longest prefix that fits, sentinels beyond it --
    with a small workspace, so that (float32 route: final counts per chunk) the row that does not fit sits in a later chunk."""
    route, qb, tb, c, ref = std
    r = RC.mixed_radii(ref, 4)
    woff, wimg, widx, wdist, wglobal = ref.cut(r)
    total, k = int(woff[-1]), ref.nq // 2
    assert woff[k] > 2 * (65536 // 24)                         # ... beyond the second chunk
    old = ctx.get_option("radius_ws_bytes")
    try:
        for ws in (65536, old):
            ctx.set_option("radius_ws_bytes", ws)
            for cap in (total - 1, int(woff[k])):
                m = int(woff[np.searchsorted(woff, cap, side="right") - 1])
                assert 0 < m <= cap and m < total
                for target in (tb, c):
                    n, off, img, idx, dist = _call(ctx, qb, target, r, cap, size=total + 3)
                    assert n == total and np.array_equal(off, woff)
                    assert np.array_equal(idx[:m], (widx if target is c else wglobal)[:m])
                    assert np.array_equal(RC.bits(dist[:m]), RC.bits(wdist[:m]))
                    assert np.all(idx[m:] == S_IDX) and np.all(dist[m:] == S_DIST), "written beyond the prefix"
                    if target is c:
                        assert np.array_equal(img[:m], wimg[:m]) and np.all(img[m:] == S_IMG)
    finally:
        ctx.set_option("radius_ws_bytes", old)


def test_degenerate_device_calls(ctx, std):
    route, qb, tb, c, ref = std
    Q, _ = RC.layout(route)
    q0, t0 = _qbank(ctx, Q[:0], route), _qbank(ctx, Q[:0], route)
    for target in (tb, c):
        n, off = _call(ctx, q0, target, np.inf, 0, lists=False)[:2]             # nq = 0: offsets[0] = 0
        assert n == 0 and off.shape == (1,) and off[0] == 0
    with ctx.collection() as e:
        e.add(Q[:0])
        for target in (t0, e):
            n, off = _call(ctx, qb, target, np.inf, 0, lists=False)[:2]
            assert n == 0 and not off.any()
    q0.close()
    t0.close()


@pytest.mark.parametrize("route", RC.ROUTES)
def test_torchmatch_radius_match(ctx, route):
    torch = _torch()
    Q, images = RC.layout(route)
    ref = RC.layout_ref(route)
    wide = torch.zeros((len(Q), 160), dtype=torch.float32 if route == "f32" else torch.uint8, device="cuda")
    wide[:, 16:144] = _dev(Q)
    q_t = wide[:, 16:144]                                      # a pitched query: a column slice of a wider tensor
    assert not q_t.is_contiguous()
    t_t = _dev(np.concatenate(images))
    qb = _qbank(ctx, Q, route)
    rows = RC.mixed_radii(ref, 5)
    every_second = _dev(np.repeat(rows, 2))[::2]               # a non-contiguous radius tensor
    assert not every_second.is_contiguous()
    with torchmatch.Collection(context=ctx) as tc:
        for im in images:
            tc.add(_dev(im))
        for r, want_r in ((float(ref.kth(4)), ref.kth(4)), (np.float32(np.inf), np.inf), (_dev(rows), rows), (every_second, rows)):
            want = ref.cut(want_r)
            for q in (q_t, qb):
                off, idx, dist = torchmatch.radius_match(q, t_t, r)
                assert off.is_cuda and idx.is_cuda and dist.is_cuda
                assert (off.dtype, idx.dtype, dist.dtype) == (torch.int64, torch.int32, torch.float32)
                assert np.array_equal(off.cpu().numpy(), want[0]) and np.array_equal(idx.cpu().numpy(), want[4])
                assert np.array_equal(RC.bits(dist.cpu().numpy()), RC.bits(want[3]))
                got = tc.radius_match(q, r)
                assert all(x.is_cuda for x in got)
                RC.same_lists(tuple(x.cpu().numpy() for x in got), want, "torchmatch collection")
    qb.close()


def test_torchmatch_fp16_source_equals_the_float32_values_of_the_same_numbers(ctx):
    torch = _torch()
    rng = np.random.default_rng(41)
    halves = [torch.from_numpy(rng.standard_normal((n, 128)).astype(np.float32)).half() for n in (90, 200, 0, 129)]
    q_h = halves[0]
    images = [h.float().numpy() for h in halves[1:]]
    Q = q_h.float().numpy()
    ref = RC.Ref(Q, images)
    r = ref.kth(3)
    rows = _dev(np.nextafter(ref.dist[:, 5], np.float32(np.inf)))
    with torchmatch.Collection(context=ctx) as tc:
        for h in halves[1:]:
            tc.add(h.cuda())
        for rr, want_r in ((float(r), r), (rows, rows.cpu().numpy())):
            want = ref.cut(want_r)
            got = tc.radius_match(q_h.cuda(), rr)
            RC.same_lists(tuple(x.cpu().numpy() for x in got), want, "fp16 source, collection")
            off, idx, dist = torchmatch.radius_match(q_h.cuda(), torch.cat(halves[1:]).cuda(), rr)
            assert np.array_equal(off.cpu().numpy(), want[0]) and np.array_equal(idx.cpu().numpy(), want[4])
            assert np.array_equal(RC.bits(dist.cpu().numpy()), RC.bits(want[3]))
