"""GPU: the stacked knnMatch calls on a WIDE train collection (129 .. 256 values per row) -- fm_collection_wide_knn(_dev),
fm_collection_wide_knn2_ratio(_dev), fm_collection_wide_votes; matchutil.BFMatcher.knnMatchWide and its kin;
torchmatch.Collection.wide_knn / wide_ratio_match / wide_votes (K14 over the stack, wide_stack.hip).

Every result is compared bit for bit -- img, idx, and the distances as uint32 patterns -- with the NumPy reference
(tests/wide_stack_ref.py: the oracle's order-1 chain on the images' rows concatenated, global rows turned into (image, row))
AND with fm_knn / fm_knn2_ratio on one bank of the concatenated rows, under the exact kernel alone ("f32_filter" 0) and under
the fp16 matrix-core filter forced on (2): the 4e6-pair threshold of setting 1 keeps these sizes on the exact kernel.  The
layout is wide_radius_ref.SIZES: padding of 0 / 1 / 63 / 127 rows behind the images, a stage with one real row followed by
seven tiles of padding, an empty image; unit-norm rows put that padding NEARER (1.0) than every real neighbour (about 1.41),
which is the case a sweep that took the stack for a bank fails."""
import ctypes
import functools
from contextlib import closing

import numpy as np
import pytest

import fastmatch_amd
from fastmatch_amd import matchutil
import wide_stack_ref as WS

pytestmark = pytest.mark.gpu

P = ctypes.c_void_p
EINVAL, EUNSUPPORTED = -1, -4
FILTERS = [(0, 0), (2, 0)]
LAYOUTS = {"sizes": WS.SIZES, "empty_ends": WS.SIZES_EMPTY_ENDS}
REAL = sum(WS.SIZES)


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


class _Filter(object):
    """The context with "f32_filter" (and "f32_nsplit") set for a block, restored behind it."""

    def __init__(self, ctx, filt, nsplit=0):
        self.ctx, self.want = ctx, {"f32_filter": filt, "f32_nsplit": nsplit}

    def __enter__(self):
        self.saved = {k: self.ctx.get_option(k) for k in self.want}
        for k, v in self.want.items():
            self.ctx.set_option(k, v)
        return self.ctx

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            self.ctx.set_option(k, v)


def _same(got, want, what, names=("img", "idx", "dist")):
    assert len(got) == len(want) == len(names), what
    for n, g, w in zip(names, got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype, (what, n, g.shape, w.shape, g.dtype, w.dtype)
        if not np.array_equal(WS.bits(g), WS.bits(w)):
            bad = np.nonzero((WS.bits(g) != WS.bits(w)).reshape(len(g), -1).any(1))[0]
            raise AssertionError("%r: %s differs in %d rows, first %d: got %r, want %r" % (what, n, len(bad), bad[0], g[bad[0]], w[bad[0]]))


@functools.lru_cache(maxsize=None)
def _data(kind, layout, nq, dim, seed=0):
    maker = {"unit": WS.unit_images, "clustered": WS.clustered_images}[kind]
    Q, images = maker(nq, LAYOUTS[layout] if isinstance(layout, str) else list(layout), dim, 100 + dim + seed)
    Q.setflags(write=False)
    for im in images:
        im.setflags(write=False)
    return Q, tuple(images)


@functools.lru_cache(maxsize=None)
def _want(kind, layout, nq, dim, k, seed=0):
    """The reference, computed once per (data set, k) and shared by the settings and the tests."""
    Q, images = _data(kind, layout, nq, dim, seed)
    out = WS.knn(Q, images, k)
    for a in out:
        a.setflags(write=False)
    return out


def _check_knn(ctx, Q, images, what, settings=FILTERS, ks=(1, 2), wants=None):
    """fm_collection_wide_knn of one data set at every k and (filter, nsplit) against the reference and against fm_knn on a
    bank of the concatenated rows; returns the number of filtered calls made."""
    qb, c = ctx.bank(Q), _collection(ctx, images)
    T = WS.concat(images, Q.shape[1])
    tb = ctx.bank(T) if len(T) and len(Q) else None
    launches = 0
    try:
        assert c.info()[:2] == (len(images), len(T))
        for k in ks:
            want = wants[k] if wants else WS.knn(Q, images, k)
            if tb is not None:
                g, d = ctx.knn(qb, tb, k)
                im, lo = WS.locate(images, g)
                _same((im.reshape(g.shape), lo.reshape(g.shape), d), want, (what, "fm_knn on the concatenation", k))
            for filt, nsplit in settings:
                with _Filter(ctx, filt, nsplit):
                    l0, f0 = ctx.f32_filter_stats()
                    got = c.wide_knn(qb, k)
                    l1, f1 = ctx.f32_filter_stats()
                _same(got, want, (what, "k", k, "f32_filter", filt, "f32_nsplit", nsplit))
                assert f1 == f0 and (l1 - l0 == 0 if filt == 0 else l1 - l0 <= 1), (what, filt, l1 - l0, f1 - f0)
                launches += l1 - l0
    finally:
        c.close(); qb.close()
        if tb is not None:
            tb.close()
    return launches


def test_a_256_d_collection_matches(ctx):
    """Red without the feature: the parent has no fm_collection_wide_knn."""
    Q, images = _data("clustered", "sizes", 300, 256)
    with _collection(ctx, images) as c, closing(ctx.bank(Q)) as qb:
        _same(c.wide_knn(qb, 2), _want("clustered", "sizes", 300, 256, 2), "k = 2")


PARITY = [(d, lay, nq) for d in WS.FULL_DIMS for lay in sorted(LAYOUTS) for nq in WS.NQS]


@pytest.mark.parametrize("dim,layout,nq", PARITY, ids=["%d-%s-%d" % p for p in PARITY])
def test_padding_nearer_than_every_real_row(ctx, dim, layout, nq):
    """Unit-norm rows: a zero (padding) row lies at 1.0 from every query row, every real neighbour at about 1.41.  No -1 appears,
    no padding index is returned -- every (img, idx) names a real row -- and the lists are the reference's."""
    Q, images = _data("unit", layout, nq, dim)
    wants = {k: _want("unit", layout, nq, dim, k) for k in (1, 2)}
    img, idx, dist = wants[2]
    sizes = np.array(LAYOUTS[layout])
    assert (img >= 0).all() and (idx >= 0).all() and (idx < sizes[img]).all() and (dist > 1.0).all()
    launches = _check_knn(ctx, Q, images, ("unit", dim, layout, nq), wants=wants)
    assert launches == (2 if nq else 0)                 # "f32_filter" 2 did take the filter, at k = 1 and at k = 2
    # clustered rows (every query row a near copy of a train row) on the same layout
    Qc, imc = _data("clustered", layout, nq, dim)
    _check_knn(ctx, Qc, imc, ("clustered", dim, layout, nq), wants={k: _want("clustered", layout, nq, dim, k) for k in (1, 2)})


@pytest.mark.parametrize("dim", WS.SMALL_DIMS)
def test_one_small_shape_at_every_k_step_boundary(ctx, dim):
    sizes = (130, 0, 1, 65)
    Q, images = _data("unit", sizes, 129, dim)
    assert _check_knn(ctx, Q, images, ("small", dim), wants={k: _want("unit", sizes, 129, dim, k) for k in (1, 2)}) == 2


@pytest.mark.parametrize("dim", WS.FULL_DIMS)
def test_split_boundaries_inside_an_image_on_a_skipped_tile_and_an_all_padding_split(ctx, dim):
    """The stack of SIZES is 15 stages = 120 tiles.  The 1-row image is stage 4: tile 32 holds its row, tiles 33 .. 39 are
    padding.  "f32_nsplit" 7: 18 tiles per split, boundaries at tiles 18 (inside the 300-row image), 36 (a skipped tile), 54 ...;
    40: 3 tiles per split, so split 11 = tiles 33 .. 35 and split 12 = tiles 36 .. 38 hold padding only -- no record, no bound."""
    first = np.concatenate([[0], np.cumsum([(n + 127) // 128 * 128 for n in WS.SIZES])])
    assert first[-1] == 1920 and first[3] == 512 and WS.SIZES[3] == 1 and first[4] == 640
    for nsplit, per in ((7, 18), (40, 3)):
        assert -(-120 // nsplit) == per
    assert 0 < 18 * 16 < 300 and 33 <= 36 <= 39 and 33 <= 3 * 11 and 3 * 12 + 2 <= 39
    for kind in ("unit", "clustered"):
        Q, images = _data(kind, "sizes", 300, dim)
        wants = {k: _want(kind, "sizes", 300, dim, k) for k in (1, 2)}
        assert _check_knn(ctx, Q, images, ("splits", kind, dim), settings=[(2, 7), (2, 40), (2, 120), (0, 0)], wants=wants) == 6


def test_ties_go_to_the_earlier_image_then_the_earlier_row(ctx):
    for dim in WS.FULL_DIMS:
        Q, images = WS.tied_images(dim, 5)
        want = WS.knn(Q, images, 2)
        assert (want[2][:10] == 0).all() and (want[0][:10] == 1).all() and (want[1][:10, 0] < want[1][:10, 1]).all()
        assert _check_knn(ctx, Q, images, ("ties", dim), wants={1: WS.knn(Q, images, 1), 2: want}) == 2


def test_fewer_than_k_real_rows(ctx):
    dim = 129
    Q = _data("unit", "sizes", 127, dim)[0]
    one = np.ascontiguousarray(Q[5:6] * np.float32(0.5))
    for images in ([], [Q[:0]], [Q[:0], Q[:0], Q[:0]], [one], [Q[:0], one, Q[:0]], [one, Q[:0], one]):
        real = sum(len(im) for im in images)
        for k in (1, 2):
            want = WS.knn(Q, images, k)
            assert (want[0] >= 0).sum() == len(Q) * min(k, real)
        _check_knn(ctx, Q, images, ("few", len(images), real))
        if images:
            _check_knn(ctx, Q[:0], images, ("few, nq = 0", len(images), real))


@pytest.mark.parametrize("factor", [1000.0, 100.0])
def test_an_add_that_rewrites_the_stack_scale_between_two_calls(ctx, factor):
    """An image 1000 times larger lowers the stack's scale by 9 or 10 binary orders -- its fp16 plane is rewritten, and the
    query's scale now lies more than 8 from it: the exact kernel answers.  100 times (6 or 7 orders): the filter still runs, on
    the rewritten plane, with the scale and the largest norm it reads at the call."""
    dim = 192
    Q, images = WS.clustered_images(150, [130, 70, 0, 200, 200], dim, 61)
    images[3] = (images[3] * np.float32(factor)).astype(np.float32)
    with closing(ctx.bank(Q)) as qb, ctx.collection() as c:
        for im in images[:3]:
            c.add_wide(im)
        for filt in (0, 2):
            with _Filter(ctx, filt):
                _same(c.wide_knn(qb, 2), WS.knn(Q, images[:3], 2), ("before", filt))
        c.add_wide(images[3])
        c.add_wide(images[4])
        for filt in (0, 2):
            with _Filter(ctx, filt):
                l0 = ctx.f32_filter_stats()[0]
                _same(c.wide_knn(qb, 2), WS.knn(Q, images, 2), ("after", filt))
                _same(c.wide_knn(qb, 1), WS.knn(Q, images, 1), ("after, k = 1", filt))
                assert ctx.f32_filter_stats()[0] - l0 == (2 if filt and factor == 100.0 else 0)


def test_what_the_filter_cannot_take_goes_to_the_exact_kernel(ctx):
    dim = 256
    Q, images = _data("clustered", "sizes", 129, dim)
    Q, images = Q.copy(), [im.copy() for im in images]

    def run(Q, images, what):
        n = _check_knn(ctx, Q, images, what, settings=[(2, 0)])
        assert n == 0, (what, n)                     # "f32_filter" 2 and still no filtered call
        want = WS.knn(Q, images, 2)
        assert not np.isnan(want[2]).any()
        return want

    # a query whose scale exponent lies more than 8 from the stack's
    run((Q * np.float32(2.0 ** -12)).astype(np.float32), images, "scales 12 apart")
    run((Q * np.float32(2.0 ** 12)).astype(np.float32), images, "scales 12 apart, the other way")
    # a NaN and a +inf in one image: the rows that hold them are never listed
    bad = [im.copy() for im in images]
    bad[6][10, 3] = np.nan
    bad[6][20, dim - 1] = np.inf
    bad[6][30] = Q[0]                                # (a row next to them is found)
    want = run(Q, bad, "NaN / inf in an image")
    hit = (want[0] == 6) & ((want[1] == 10) | (want[1] == 20))
    assert not hit.any() and want[0][0, 0] == 6 and want[1][0, 0] == 30
    # a NaN in a query row: that row's lists are empty, the others unchanged
    Qn = Q.copy()
    Qn[7, 100] = np.nan
    want = run(Qn, images, "NaN in a query row")
    assert (want[0][7] == -1).all() and np.isinf(want[2][7]).all() and (want[0][8] >= 0).all()


def test_the_list_overflow_falls_back_to_the_exact_kernel(ctx):
    """600 x 2100 = 1.26 million pairs inside the margin against 2^20 records, the copies spread over two images: the exact
    kernel redoes the call, and the fallback is counted -- which is what keeps this case from passing without exercising it."""
    Q, images, fewer = WS.overflow_images()
    with closing(ctx.bank(Q)) as qb, _collection(ctx, images) as c, _collection(ctx, fewer) as cf:
        for k in (1, 2):
            with _Filter(ctx, 2):
                l0, f0 = ctx.f32_filter_stats()
                got = c.wide_knn(qb, k)
                l1, f1 = ctx.f32_filter_stats()
            assert (l1 - l0, f1 - f0) == (1, 1), k
            _same(got, WS.knn(Q, images, k), ("overflow", k))
        with _Filter(ctx, 2):
            l0, f0 = ctx.f32_filter_stats()
            got = cf.wide_knn(qb, 2)
            l1, f1 = ctx.f32_filter_stats()
        assert (l1 - l0, f1 - f0) == (1, 0)              # a filtered call without overflow: one launch, no fallback
        _same(got, WS.knn(Q, fewer, 2), "no overflow")


# ---- the ratio test and the votes --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=WS.FULL_DIMS)
def std(ctx, request):
    """(dim, Q, images, query bank, collection, bank of the concatenation) of the standard layout with clustered rows, some of
    them duplicated so that d1 == 0 and d0 == d1 occur; every test leaves the collection unchanged."""
    dim = request.param
    Q, images = WS.clustered_images(300, WS.SIZES, dim, 70 + dim)
    images[6][5] = images[0][7]                          # a row present in two images: d0 == d1 for a query on it
    Q[3] = images[0][7]                                  # ... exactly: 0 / 0
    Q[4] = images[2][9]                                  # an exact copy with a distinct second neighbour: ratio 0
    qb, c, tb = ctx.bank(Q), _collection(ctx, images), ctx.bank(WS.concat(images, dim))
    yield dim, Q, images, qb, c, tb
    for x in (tb, c, qb):
        x.close()


def _ratio_raw(ctx, c, qb, tau, cap, name="fm_collection_wide_knn2_ratio"):
    n = max(cap, 1) + 3
    qidx, img, tidx = np.full(n, -7, np.int32), np.full(n, -7, np.int32), np.full(n, -7, np.int32)
    dist, ratio = np.full(n, -7, np.float32), np.full(n, -7, np.float64)
    nacc = ctypes.c_int64(-5)
    rc = getattr(ctx.lib, name)(ctx.handle, c.handle, qb.handle, float(tau), cap, _ptr(qidx), _ptr(img), _ptr(tidx), _ptr(dist), _ptr(ratio),
                                ctypes.byref(nacc))
    assert rc == 0, ctx.lib.fm_last_error(ctx.handle)
    return int(nacc.value), (qidx, img, tidx, dist, ratio)


@pytest.mark.parametrize("tau", [0.6, 0.8, 1.0])
def test_knn2_ratio(ctx, std, tau):
    dim, Q, images, qb, c, tb = std
    want = WS.ratio_match(Q, images, tau)
    count = len(want[0])
    assert 0 < count < len(Q) and 3 not in want[0] and (4 in want[0])
    names = ("qidx", "img", "tidx", "dist", "ratio")
    # fm_knn2_ratio on the bank of the concatenated rows
    bq, bt, bd, br = ctx.knn2_ratio(qb, tb, tau)
    bi, bl = WS.locate(images, bt)
    _same((bq, bi, bl, bd, br), want, ("fm_knn2_ratio on the concatenation", tau), names)
    for filt in (0, 2):
        with _Filter(ctx, filt):
            _same(c.wide_knn2_ratio(qb, tau), want, ("ratio", tau, filt), names)
            for cap in (0, count // 2, count, len(Q)):                   # cap 0, cap < count, cap >= count
                nacc, cols = _ratio_raw(ctx, c, qb, tau, cap)
                m = min(cap, count)
                assert nacc == count, (cap, nacc)                        # the full count, whatever cap
                _same(tuple(a[:m] for a in cols), tuple(w[:m] for w in want), ("ratio cap", cap, filt), names)
                assert all((a[m:] == -7).all() for a in cols), "written beyond min(count, cap)"


def test_votes(ctx, std):
    dim, Q, images, qb, c, tb = std
    each = c.wide_knn2_each(qb)
    for tau in (0.6, 0.9):
        w0, w1 = WS.votes(Q, images, tau, 0), WS.votes(Q, images, tau, 1)
        # (an image's own second neighbour is no nearer than the collection's: a row that passes mode 0 passes mode 1 there)
        assert w0.sum() > 0 and (w1 >= w0).all() and w0[1] == w1[1] == 0
        assert np.array_equal(WS.votes_from_each(each[0], each[1], tau), w1)
        for filt in (0, 2):
            with _Filter(ctx, filt):
                for mode, want in ((0, w0), (1, w1)):
                    got = c.wide_votes(qb, tau, mode)
                    assert got.dtype == np.int64 and np.array_equal(got, want), (tau, filt, mode, got, want)
    # nq = 0, empty images only, no image
    with closing(ctx.bank(Q[:0])) as q0:
        assert c.wide_votes(q0, 0.8, 0).tolist() == c.wide_votes(q0, 0.8, 1).tolist() == [0] * len(images)
    with _collection(ctx, [Q[:0], Q[:0]]) as e, ctx.collection() as none:
        for mode in (0, 1):
            assert e.wide_votes(qb, 0.8, mode).tolist() == [0, 0] and none.wide_votes(qb, 0.8, mode).shape == (0,)


# ---- the device forms, torchmatch, matchutil ---------------------------------------------------------------------------------
def test_device_forms_and_torchmatch_equal_the_host_forms(ctx, std):
    torch = _torch()
    dim, Q, images, qb, c, tb = std
    side = torch.cuda.Stream()
    for k in (1, 2):
        host = c.wide_knn(qb, k)
        for stream in ("current", side, None):
            with torch.cuda.stream(side if stream is side else torch.cuda.current_stream()):
                img = torch.full((qb.n, k), -7, dtype=torch.int32, device="cuda")
                idx = torch.full((qb.n, k), -7, dtype=torch.int32, device="cuda")
                dist = torch.full((qb.n, k), -7.0, dtype=torch.float32, device="cuda")
                s = torch.cuda.current_stream().cuda_stream if stream is not None else None
                if stream is None:
                    torch.cuda.synchronize()
                c.wide_knn_dev(qb, k, img.data_ptr(), idx.data_ptr(), dist.data_ptr(), consumer_stream=s)
                if stream is None:
                    ctx.sync()
                got = (img.cpu().numpy(), idx.cpu().numpy(), dist.cpu().numpy())
            _same(got, host, ("knn_dev", k, "side" if stream is side else stream))
    tau = 0.8
    host = c.wide_knn2_ratio(qb, tau)
    count = len(host[0])
    for cap, stream in ((len(Q), "current"), (count // 2, side), (0, "current")):
        with torch.cuda.stream(side if stream is side else torch.cuda.current_stream()):
            rows = torch.full((max(cap, 1), 4), -7, dtype=torch.int32, device="cuda")
            cnt = torch.full((1,), -7, dtype=torch.int64, device="cuda")
            n = c.wide_knn2_ratio_dev(qb, tau, rows.data_ptr() if cap else 0, cnt.data_ptr(), cap, want_count=True,
                                      consumer_stream=torch.cuda.current_stream().cuda_stream)
            r, m = rows.cpu().numpy(), min(cap, count)
            assert n == count and int(cnt.cpu()[0]) == m
        _same((r[:m, 0], r[:m, 1], r[:m, 2], np.ascontiguousarray(r[:m, 3]).view(np.float32)), tuple(h[:m] for h in host[:4]),
              ("ratio_dev", cap), ("qidx", "img", "tidx", "dist"))
        assert (r[m:] == -7).all()
    # torchmatch: a float32 tensor and a bank as the query
    from fastmatch_amd import torchmatch
    with torchmatch.Collection(context=ctx) as tc:
        for im in images:
            tc.add_wide(_dev(im))
        for q in (_dev(Q), qb):
            for k in (1, 2):
                got = tc.wide_knn(q, k)
                assert all(x.is_cuda for x in got) and [x.dtype for x in got] == [torch.int32, torch.int32, torch.float32]
                _same(tuple(x.cpu().numpy() for x in got), c.wide_knn(qb, k), ("torchmatch wide_knn", k))
            with torch.cuda.stream(side):
                got = tc.wide_ratio_match(q, tau)
                assert all(x.is_cuda for x in got)
                _same(tuple(x.cpu().numpy() for x in got), host[:4], "torchmatch wide_ratio_match", ("qidx", "img", "tidx", "dist"))
            for mode in (0, 1):
                v = tc.wide_votes(q, tau, mode)
                assert v.is_cuda and v.dtype == torch.int64 and np.array_equal(v.cpu().numpy(), c.wide_votes(qb, tau, mode))
        with pytest.raises(ValueError, match="wide collection"):
            tc.knn(_dev(Q), 2)


def test_matchutil_methods(ctx, std):
    dim, Q, images, qb, c, tb = std
    m = matchutil.BFMatcher(matchutil.NORM_L2)
    m.add_wide(list(images))
    for k in (1, 2):
        want = WS.knn(Q, images, k)
        _same(m.knnMatchWide_arrays(Q, k), want, ("knnMatchWide_arrays", k))
        lists = m.knnMatchWide(Q.astype(np.float64), k)
        assert len(lists) == len(Q) and all(len(row) == k for row in lists)
        assert [[(d.queryIdx, d.imgIdx, d.trainIdx) for d in row] for row in lists] == \
            [[(i, int(want[0][i, j]), int(want[1][i, j])) for j in range(k)] for i in range(len(Q))]
        assert all(np.float32(d.distance) == want[2][i, j] for i, row in enumerate(lists) for j, d in enumerate(row))
    _same(m.ratioMatchWide_arrays(Q, 0.8), WS.ratio_match(Q, images, 0.8), "ratioMatchWide_arrays", ("qidx", "img", "tidx", "dist", "ratio"))
    for mode in (0, 1):
        assert np.array_equal(m.votesWide(Q, 0.8, mode), WS.votes(Q, images, 0.8, mode))
    with pytest.raises(ValueError, match="wide"):
        m.knnMatch(Q, k=2)                               # the L2-named method keeps refusing
    m.clear()


def test_accounting_in_fm_stats(ctx, std):
    torch = _torch()
    dim, Q, images, qb, c, tb = std
    nq = len(Q)

    def grown(call):
        before = ctx.stats()
        call()
        after = ctx.stats()
        return after["calls"] - before["calls"], after["pairs"] - before["pairs"]

    assert grown(lambda: c.wide_knn(qb, 2)) == (1, nq * REAL)
    assert grown(lambda: c.wide_knn(qb, 1)) == (1, nq * REAL)
    assert grown(lambda: c.wide_knn2_ratio(qb, 0.8)) == (1, nq * REAL)
    assert grown(lambda: c.wide_votes(qb, 0.8, 0)) == (1, nq * REAL)
    assert grown(lambda: c.wide_votes(qb, 0.8, 1)) == (1, nq * REAL)
    img = torch.zeros((nq, 2), dtype=torch.int32, device="cuda")
    dist = torch.zeros((nq, 2), dtype=torch.float32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    assert grown(lambda: c.wide_knn_dev(qb, 2, img.data_ptr(), img.data_ptr(), dist.data_ptr(), consumer_stream=s))[1] == 0
    assert grown(lambda: c.wide_knn2_ratio_dev(qb, 0.8, 0, cnt.data_ptr(), 0, want_count=True, consumer_stream=s))[1] == 0
    torch.cuda.synchronize()


# ---- errors ------------------------------------------------------------------------------------------------------------------
def test_errors_in_their_order_leave_the_context_working(ctx, std):
    torch = _torch()
    dim, Q, images, qb, c, tb = std
    lib = ctx.lib
    other = fastmatch_amd.Context(0)
    rng = np.random.default_rng(81)
    f32 = ctx.bank(np.ascontiguousarray(Q[:, :128]), float_route=True)
    f32e = ctx.bank(np.ascontiguousarray(Q[:0, :128]), float_route=True)
    binb = ctx.bank_binary(rng.integers(0, 256, (9, 32), dtype=np.uint8))
    w_other = ctx.bank(np.zeros((4, 130 if dim != 130 else 131), np.float32))
    w_other0 = ctx.bank(np.zeros((0, 200), np.float32))
    nq = qb.n
    img, idx, dist = np.zeros((nq, 2), np.int32), np.zeros((nq, 2), np.int32), np.zeros((nq, 2), np.float32)
    ratio, votes, nacc = np.zeros(nq, np.float64), np.zeros(len(images), np.int64), ctypes.c_int64(0)
    d_img = torch.zeros((nq, 2), dtype=torch.int32, device="cuda")
    d_idx = torch.zeros((nq, 2), dtype=torch.int32, device="cuda")
    d_dist = torch.zeros((nq, 2), dtype=torch.float32, device="cuda")
    d_cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    dp = lambda t: P(t.data_ptr())                                        # noqa: E731
    NS = P(-1)                                                            # FM_NO_STREAM
    H = ctx.handle

    # every call with "everything behind the collection and the query wrong": k = 0 / mode = 7 / cap = -1, outputs NULL
    calls = {
        "fm_collection_wide_knn": lambda ch, q: lib.fm_collection_wide_knn(H, ch, q, 0, None, None, None),
        "fm_collection_wide_knn_dev": lambda ch, q: lib.fm_collection_wide_knn_dev(H, ch, q, 0, None, None, None, NS),
        "fm_collection_wide_knn2_ratio": lambda ch, q: lib.fm_collection_wide_knn2_ratio(H, ch, q, 0.8, -1, None, None, None, None, None, None),
        "fm_collection_wide_knn2_ratio_dev": lambda ch, q: lib.fm_collection_wide_knn2_ratio_dev(H, ch, q, 0.8, -1, None, None, None, NS),
        "fm_collection_wide_votes": lambda ch, q: lib.fm_collection_wide_votes(H, ch, q, 0.8, 7, None),
    }
    l2 = {"fm_collection_wide_knn": "fm_collection_knn", "fm_collection_wide_knn_dev": "fm_collection_knn_dev",
          "fm_collection_wide_knn2_ratio": "fm_collection_knn2_ratio", "fm_collection_wide_knn2_ratio_dev": "fm_collection_knn2_ratio_dev",
          "fm_collection_wide_votes": "fm_collection_votes"}

    def refused(rc, *words, code=EINVAL):
        assert rc == code, rc
        msg = lib.fm_last_error(H).decode()
        for w in words:
            assert w in msg, msg

    torch.cuda.synchronize()
    with ctx.collection() as cl, ctx.collection() as cbin, ctx.collection() as ce, other.collection() as cf:
        cl.add(np.ascontiguousarray(Q[:50, :128]))                        # an L2 collection
        cbin.add_binary(rng.integers(0, 256, (50, 32), dtype=np.uint8))
        for name, call in calls.items():
            # 1. NULL handles, a foreign context -- in front of everything else
            refused(call(None, qb.handle), "NULL")
            refused(call(c.handle, None), "NULL")
            refused(call(cf.handle, f32.handle), "another context")
            # 2. a query that is not wide, even an empty one; a non-empty collection that is not; the message names the call that serves it
            for ch, q in ((c.handle, f32.handle), (c.handle, f32e.handle), (cl.handle, qb.handle), (c.handle, binb.handle),
                          (cbin.handle, qb.handle), (ce.handle, f32.handle)):
                refused(call(ch, q), name + ":", "wide", l2[name] + " is the call that serves")
            # 3. widths -- in front of k / mode / cap
            refused(call(c.handle, w_other.handle), "width")
            refused(call(c.handle, w_other0.handle), "width")
        # 4. k, the mode -- in front of the output pointers
        for name, args in (("fm_collection_wide_knn", ()), ("fm_collection_wide_knn_dev", (NS,))):
            fn = getattr(lib, name)
            refused(fn(H, c.handle, qb.handle, 0, None, None, None, *args), "k must be at least 1")
            refused(fn(H, c.handle, qb.handle, -2, None, None, None, *args), "k must be at least 1")
            refused(fn(H, c.handle, qb.handle, 3, None, None, None, *args), "k >= 3", code=EUNSUPPORTED)
            refused(fn(H, c.handle, qb.handle, 8, None, None, None, *args), "k >= 3", code=EUNSUPPORTED)
        refused(lib.fm_collection_wide_votes(H, c.handle, qb.handle, 0.8, 2, None), "mode")
        refused(lib.fm_collection_wide_votes(H, c.handle, qb.handle, 0.8, -1, None), "mode")
        # 5. the output pointers: the host forms check NULL with nq > 0 ...
        for trio in ((None, _ptr(idx), _ptr(dist)), (_ptr(img), None, _ptr(dist)), (_ptr(img), _ptr(idx), None)):
            refused(lib.fm_collection_wide_knn(H, c.handle, qb.handle, 2, *trio), "fm_collection_wide_knn: output pointer is NULL")
        refused(lib.fm_collection_wide_votes(H, c.handle, qb.handle, 0.8, 0, None), "votes is NULL")
        refused(lib.fm_collection_wide_knn2_ratio(H, c.handle, qb.handle, 0.8, -1, _ptr(img), _ptr(img), _ptr(idx), _ptr(dist), _ptr(ratio),
                                                  ctypes.byref(nacc)), "bad output arguments")
        refused(lib.fm_collection_wide_knn2_ratio(H, c.handle, qb.handle, 0.8, 4, _ptr(img), None, _ptr(idx), _ptr(dist), _ptr(ratio),
                                                  ctypes.byref(nacc)), "bad output arguments")
        with closing(ctx.bank(Q[:0])) as q0:                                      # nq = 0: NULL outputs are fine
            assert lib.fm_collection_wide_knn(H, c.handle, q0.handle, 2, None, None, None) == 0
            assert lib.fm_collection_wide_knn_dev(H, c.handle, q0.handle, 2, None, None, None, NS) == 0
            assert lib.fm_collection_wide_knn2_ratio(H, c.handle, q0.handle, 0.8, 0, None, None, None, None, None, None) == 0
        # ... the _dev forms use fm_collection_knn_dev's / fm_collection_knn2_ratio_dev's pointer checks
        refused(lib.fm_collection_wide_knn_dev(H, c.handle, qb.handle, 2, None, dp(d_idx), dp(d_dist), NS), "output pointer is NULL")
        refused(lib.fm_collection_wide_knn_dev(H, c.handle, qb.handle, 2, _ptr(img), dp(d_idx), dp(d_dist), NS), "d_img")
        refused(lib.fm_collection_wide_knn_dev(H, c.handle, qb.handle, 2, dp(d_img), _ptr(idx), dp(d_dist), NS), "d_idx")
        refused(lib.fm_collection_wide_knn_dev(H, c.handle, qb.handle, 2, dp(d_img), dp(d_idx), _ptr(dist), NS), "d_dist")
        refused(lib.fm_collection_wide_knn2_ratio_dev(H, c.handle, qb.handle, 0.8, 4, dp(d_img), None, None, NS), "bad output arguments")
        refused(lib.fm_collection_wide_knn2_ratio_dev(H, c.handle, qb.handle, 0.8, 4, None, dp(d_cnt), None, NS), "bad output arguments")
        refused(lib.fm_collection_wide_knn2_ratio_dev(H, c.handle, qb.handle, 0.8, 4, dp(d_img), _ptr(votes), None, NS), "d_count")
        refused(lib.fm_collection_wide_knn2_ratio_dev(H, c.handle, qb.handle, 0.8, 4, _ptr(img), dp(d_cnt), None, NS), "d_rows")
        # a collection on which no add has succeeded is valid (and has no width yet)
        for q in (qb, w_other):
            got = ce.wide_knn(q, 2)
            assert (got[0] == -1).all() and (got[1] == -1).all() and np.isinf(got[2]).all()
            assert len(ce.wide_knn2_ratio(q, 0.8)[0]) == 0 and ce.wide_votes(q, 0.8).shape == (0,)
        # the L2-named calls keep refusing a wide collection, and a wide query; their message says "wide"
        for rc in (lib.fm_collection_knn(H, c.handle, qb.handle, 2, _ptr(img), _ptr(idx), _ptr(dist)),
                   lib.fm_collection_knn_dev(H, c.handle, qb.handle, 2, dp(d_img), dp(d_idx), dp(d_dist), NS),
                   lib.fm_collection_knn2_ratio(H, c.handle, qb.handle, 0.8, 4, _ptr(img), _ptr(img), _ptr(idx), _ptr(dist), _ptr(ratio),
                                                ctypes.byref(nacc)),
                   lib.fm_collection_knn2_ratio_dev(H, c.handle, qb.handle, 0.8, 4, dp(d_img), dp(d_cnt), None, NS),
                   lib.fm_collection_votes(H, c.handle, qb.handle, 0.8, 0, _ptr(votes)),
                   lib.fm_collection_votes(H, c.handle, qb.handle, 0.8, 1, _ptr(votes))):
            refused(rc, "wide", "fm_collection_wide_knn(_dev)", code=EUNSUPPORTED)
        assert lib.fm_collection_knn(H, cl.handle, qb.handle, 2, _ptr(img), _ptr(idx), _ptr(dist)) != 0      # a wide query, an L2 collection
        assert "wide" in lib.fm_last_error(H).decode()
    # the context still answers
    _same(c.wide_knn(qb, 2), WS.knn(Q, images, 2), "after the refusals")
    for b in (f32, f32e, binb, w_other, w_other0):
        b.close()
    other.close()


# ---- fuzz --------------------------------------------------------------------------------------------------------------------
FUZZ_SIZES = [0, 0, 1, 5, 64, 127, 128, 129, 200, 256, 300]
FUZZ_DIMS = [129, 160, 161, 192, 193, 224, 255, 256]


@pytest.mark.parametrize("group", range(6))
def test_fuzz(ctx, group):
    """Six seeds per case: random image counts and sizes (0 and multiples of 128 among them), nq, dim, k, filter setting and
    split count; knn, the ratio test and the votes against the reference."""
    for seed in range(6 * group, 6 * group + 6):
        rng = np.random.default_rng(1000 + seed)
        sizes = [int(rng.choice(FUZZ_SIZES)) for _ in range(int(rng.integers(1, 7)))]
        nq, dim, k = int(rng.choice([1, 17, 128, 150])), int(rng.choice(FUZZ_DIMS)), int(rng.integers(1, 3))
        filt, nsplit, tau = int(rng.integers(0, 3)), int(rng.choice([0, 2, 5, 9])), float(rng.choice([0.7, 0.95]))
        Q, images = WS.clustered_images(nq, sizes, dim, 2000 + seed)
        what = ("fuzz", seed, sizes, nq, dim, k, filt, nsplit)
        with closing(ctx.bank(Q)) as qb, _collection(ctx, images) as c, _Filter(ctx, filt, nsplit):
            _same(c.wide_knn(qb, k), WS.knn(Q, images, k), what)
            _same(c.wide_knn2_ratio(qb, tau), WS.ratio_match(Q, images, tau), what, ("qidx", "img", "tidx", "dist", "ratio"))
            mode = seed & 1
            assert np.array_equal(c.wide_votes(qb, tau, mode), WS.votes(Q, images, tau, mode)), what
