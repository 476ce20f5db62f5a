"""GPU: knnMatch under a mask on wide float banks (fm_wide_knn_masked, fm_wide_knn_masked_dev; wide_masked.hip).  Every result
is compared bit for bit, idx and dist, with the oracle's order-1 chain over each query row's permitted train rows
(tests/wide_masked_ref.py), under the masked exact kernel alone ("f32_filter" 0) and under the masked fp16 matrix-core filter
forced on (2): the 4e6-pair threshold of setting 1 keeps these sizes on the exact kernel."""
import functools
import os
import sys

import numpy as np
import pytest

from fastmatch_amd import _ffi, matchutil

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wide_masked_ref as WM    # noqa: E402
import wide_ref                 # noqa: E402

pytestmark = pytest.mark.gpu

FILTERS = [0, 2]
KS = [1, 2]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.kind == "f" else a


def _same(got, want, what):
    assert len(got) == len(want) == 2, what
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, i, g.shape, w.shape)
        if not np.array_equal(_bits(g), _bits(w)):
            bad = np.nonzero((_bits(g) != _bits(w)).reshape(len(g), -1).any(1))[0]
            raise AssertionError("%r: %s differs in %d rows, first %d: got %r, want %r"
                                 % (what, ("idx", "dist")[i], len(bad), bad[0], g[bad[0]], w[bad[0]]))


@functools.lru_cache(maxsize=None)
def _data(regime, nq, nt, dim, seed=7):
    Q, T = WM.data(regime, nq, nt, dim, seed)
    Q.setflags(write=False)
    T.setflags(write=False)
    return Q, T


@functools.lru_cache(maxsize=None)
def _mask(name, nq, nt, k, seed=5):
    m = WM.MASKS[name](nq, nt, k, seed)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def _want(regime, nq, nt, dim, mask_name, k):
    """The reference, computed once per (data set, mask, k) and shared by the filter settings."""
    Q, T = _data(regime, nq, nt, dim)
    return WM.knn(Q, T, _mask(mask_name, nq, nt, k), k)


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


def _masked(ctx, qb, tb, m, k):
    with ctx.mask(qb.n, tb.n) as mk:
        return ctx.wide_knn_masked(qb, tb, mk.set(m), k)


def _check_masks(ctx, regime, nq, nt, dim, masks, settings):
    """Every mask x k x (filter, nsplit) of one data set against the reference; returns the filtered calls that were made."""
    Q, T = _data(regime, nq, nt, dim)
    qb, tb = ctx.bank(Q), ctx.bank(T)
    launches = 0
    try:
        assert qb.kind == tb.kind == _ffi.FM_BANK_F32W and qb.dim == dim
        for name in masks:
            for k in KS:
                want = _want(regime, nq, nt, dim, name, k)
                for filt, nsplit in settings:
                    with _Filter(ctx, filt, nsplit):
                        l0 = ctx.f32_filter_stats()[0]
                        got = _masked(ctx, qb, tb, _mask(name, nq, nt, k), k)
                        grown = ctx.f32_filter_stats()[0] - l0
                    _same(got, want, (regime, dim, (nq, nt), name, "k", k, "f32_filter", filt, "f32_nsplit", nsplit))
                    assert grown == 0 if filt == 0 else grown <= 1
                    launches += grown
                if name == "ones" and nq:
                    # an all-ones mask reproduces fm_knn bit for bit
                    _same(got, ctx.knn(qb, tb, k), (regime, dim, (nq, nt), "ones against fm_knn", k))
    finally:
        qb.close(); tb.close()
    return launches


def test_a_masked_256_d_pair_matches(ctx):
    """Red without the feature: the parent has no fm_wide_knn_masked."""
    Q, T = _data("clustered", 300, 257, 256)
    m = _mask("half", 300, 257, 2)
    qb, tb = ctx.bank(Q), ctx.bank(T)
    try:
        _same(_masked(ctx, qb, tb, m, 2), _want("clustered", 300, 257, 256, "half", 2), "k = 2")
    finally:
        qb.close(); tb.close()


PARITY = [(d, s) for d in WM.DIMS for s in WM.SHAPES]


@pytest.mark.parametrize("dim,shape", PARITY, ids=["%d-%dx%d" % (d, s[0], s[1]) for d, s in PARITY])
def test_parity_with_the_reference(ctx, dim, shape):
    launches = _check_masks(ctx, "clustered", shape[0], shape[1], dim, sorted(WM.MASKS), [(0, 0), (2, 0)])
    if shape[0] and shape[1]:
        assert launches > 0                     # "f32_filter" 2 did take the filter


@pytest.mark.parametrize("mask_name", sorted(WM.MASKS))
@pytest.mark.parametrize("dim", [129, 256])
def test_large_shape_and_split_boundaries(ctx, dim, mask_name):
    """1000 x 4099: 65 mask words per row, the last one partial; with "f32_nsplit" 3 the filter's splits start at tiles 0, 86 and
    172 -- inside a group of four tiles, so a split's first mask word is used from its middle."""
    nq, nt = WM.LARGE
    assert _check_masks(ctx, "clustered", nq, nt, dim, [mask_name], [(0, 0), (2, 0), (2, 3)]) == 4


@pytest.mark.parametrize("regime", WM.REGIMES)
def test_data_regimes(ctx, regime):
    nq, nt, dim = 300, 257, 161
    launches = _check_masks(ctx, regime, nq, nt, dim, ["ones", "half", "sparse", "band"], [(0, 0), (2, 0)])
    assert (launches > 0) == (regime in wide_ref.FILTERED)          # a value that is not finite: the exact kernel, always
    Q, T = _data(regime, nq, nt, dim)
    if regime == "copies":
        # ties go to the lowest PERMITTED index: forbid the first two copies, the next two take their places
        vals, counts = np.unique(np.asarray(T)[:, 0], return_counts=True)
        rows = np.nonzero(np.asarray(T)[:, 0] == vals[counts.argmax()])[0]
        assert len(rows) >= 200
        m = np.ones((nq, nt), np.uint8)
        m[:, rows[:2]] = 0
        qb, tb = ctx.bank(Q), ctx.bank(T)
        try:
            for filt in FILTERS:
                with _Filter(ctx, filt):
                    idx, dist = _masked(ctx, qb, tb, m, 2)
                _same((idx, dist), WM.knn(Q, T, m, 2), ("copies, two forbidden", filt))
                assert (idx[:nq // 2, 0] == rows[2]).all() and (idx[:nq // 2, 1] == rows[3]).all()
        finally:
            qb.close(); tb.close()
    if regime == "nonfinite":
        qb, tb = ctx.bank(Q), ctx.bank(T)
        try:
            idx, dist = _masked(ctx, qb, tb, np.ones((nq, nt), np.uint8), 2)
            assert (idx[nq // 2] == -1).all() and np.isinf(dist[nq // 2]).all()          # a NaN row matches nothing
            assert not np.isin(idx, [nt // 2, nt // 3]).any() and np.isfinite(dist[idx >= 0]).all()
        finally:
            qb.close(); tb.close()


@pytest.mark.parametrize("dim", [129, 256])
def test_a_forbidden_exact_copy_does_not_enter_the_bound(ctx, dim):
    """Every query row has an exact copy of itself in the train bank, forbidden.  Its score is the row's maximum: in a bound it
    would shut the permitted neighbours out.  It must not be listed and the neighbours behind it must all be found."""
    nq, nt = 300, 1100
    Q, T, mask, rows = WM.planted(nq, nt, dim, 9)
    qb, tb = ctx.bank(Q), ctx.bank(T)
    try:
        for k in KS:
            want = WM.knn(Q, T, mask, k)
            assert (want[0] >= 0).all() and (want[1] > 0).all()
            for filt in FILTERS:
                with _Filter(ctx, filt):
                    l0 = ctx.f32_filter_stats()[0]
                    idx, dist = _masked(ctx, qb, tb, mask, k)
                    assert ctx.f32_filter_stats()[0] - l0 == (1 if filt else 0)
                _same((idx, dist), want, ("planted", dim, k, filt))
                assert not (idx == rows[:, None]).any()
        # with the copy permitted it is the first neighbour, at distance 0
        idx, dist = _masked(ctx, qb, tb, np.ones((nq, nt), np.uint8), 1)
        assert (idx[:, 0] == rows).all() and (dist == 0).all()
    finally:
        qb.close(); tb.close()


def test_the_list_overflow_falls_back_to_the_masked_exact_kernel(ctx):
    """600 x 1890 = 1.13 million permitted pairs inside the margin against 2^20 records: the masked exact kernel redoes the call,
    and the fallback is counted -- which is what keeps this case from passing without exercising it."""
    Q, T, mask = WM.overflow_cluster()
    qb, tb = ctx.bank(Q), ctx.bank(T)
    try:
        for k in KS:
            with _Filter(ctx, 2):
                l0, f0 = ctx.f32_filter_stats()
                got = _masked(ctx, qb, tb, mask, k)
                l1, f1 = ctx.f32_filter_stats()
            assert (l1 - l0, f1 - f0) == (1, 1), k
            _same(got, WM.knn(Q, T, mask, k), ("overflow", k))
        # the same call with half of the copies forbidden fits the list: no fallback
        fewer = mask.copy()
        fewer[:, np.nonzero((T == T[np.nonzero(mask[0] == 0)[0][0]]).all(1))[0][::2]] = 0
        with _Filter(ctx, 2):
            l0, f0 = ctx.f32_filter_stats()
            got = _masked(ctx, qb, tb, fewer, 2)
            l1, f1 = ctx.f32_filter_stats()
        assert (l1 - l0, f1 - f0) == (1, 0)
        _same(got, WM.knn(Q, T, fewer, 2), "no overflow")
    finally:
        qb.close(); tb.close()


# ---- device form, torchmatch, matchutil --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [129, 256])
def test_device_form_and_torchmatch(ctx, dim):
    import torch
    from fastmatch_amd import torchmatch
    nq, nt = 300, 257
    Q, T = _data("clustered", nq, nt, dim)
    tq, tt = torch.from_numpy(np.array(Q)).cuda(), torch.from_numpy(np.array(T)).cuda()
    sources = {"float32": (tq, tt), "float16": (tq.half(), tt.half()), "bfloat16": (tq.bfloat16(), tt.bfloat16())}
    m = _mask("half", nq, nt, 2)
    dm = torch.from_numpy(np.array(m)).cuda()
    wide_m = torch.zeros((nq, nt + 19), dtype=torch.uint8, device="cuda")
    wide_m[:, 7:7 + nt] = dm
    for filt in FILTERS:
        with _Filter(ctx, filt):
            for name, (dq, dt) in sources.items():
                hq, ht = dq.float().cpu().numpy(), dt.float().cpu().numpy()          # the values the device bank holds, exactly
                hqb, htb = ctx.bank(hq), ctx.bank(ht)
                dqb, dtb = torchmatch.bank(dq, context=ctx), torchmatch.bank(dt, context=ctx)
                try:
                    for k in KS:
                        want = _masked(ctx, hqb, htb, m, k)
                        _same(want, WM.knn(hq, ht, m, k), (name, filt, k, "host form against the reference"))
                        for what, mask in (("uint8", dm), ("bool", dm.bool()), ("pitched", wide_m[:, 7:7 + nt])):
                            idx, dist = torchmatch.wide_knn_masked(dq, dt, k, mask)
                            assert idx.is_cuda and dist.is_cuda and idx.dtype == torch.int32 and dist.dtype == torch.float32
                            _same((idx.cpu().numpy(), dist.cpu().numpy()), want, (name, filt, k, what, "torchmatch"))
                        with ctx.mask(nq, nt) as mk:                                  # resident banks and a resident Mask
                            mk.set(m)
                            idx, dist = torchmatch.wide_knn_masked(dqb, dtb, k, mk)
                            _same((idx.cpu().numpy(), dist.cpu().numpy()), want, (name, filt, k, "resident"))
                            # the raw device form
                            d_idx = torch.full((nq, k), -7, dtype=torch.int32, device="cuda")
                            d_dist = torch.full((nq, k), -7.0, dtype=torch.float32, device="cuda")
                            ctx.wide_knn_masked_dev(dqb, dtb, mk, k, d_idx.data_ptr(), d_dist.data_ptr(),
                                                    consumer_stream=torch.cuda.current_stream().cuda_stream)
                            _same((d_idx.cpu().numpy(), d_dist.cpu().numpy()), want, (name, filt, k, "_dev"))
                finally:
                    for b in (hqb, htb, dqb, dtb):
                        b.close()
    # empty operands
    for eq, et in ((0, 5), (5, 0)):
        idx, dist = torchmatch.wide_knn_masked(tq[:eq], tt[:et], 2, torch.ones((eq, et), dtype=torch.bool, device="cuda"))
        assert tuple(idx.shape) == (eq, 2) and (idx.cpu().numpy() == -1).all() and np.isinf(dist.cpu().numpy()).all()


def test_matchutil_takes_a_masked_wide_pair(ctx):
    Q, T = _data("clustered", 300, 257, 256)
    m = _mask("sparse", 300, 257, 2)
    opts = {"context": ctx}
    for k in KS:
        want = _want("clustered", 300, 257, 256, "sparse", 2)
        want = (want[0][:, :k], want[1][:, :k])
        _same(matchutil.wide_bf_match_masked_arrays(Q, T, m, k=k, options=opts), want, ("arrays", k))
        _same(matchutil.wide_bf_match_masked_arrays(Q.astype(np.float64), T, m.astype(bool), k=k, options=opts), want, ("float64 / bool", k))
    qb, tb = ctx.bank(Q), ctx.bank(T)
    try:
        with ctx.mask(300, 257) as mk:
            mk.set(m)
            _same(matchutil.wide_bf_match_masked_arrays(qb, tb, mk, k=2, options=opts), want, "resident")
    finally:
        qb.close(); tb.close()
    lists = matchutil.wide_bf_match_masked(Q, T, m, k=2, options=opts)
    assert [[x.trainIdx for x in row] for row in lists] == [[j for j in row if j >= 0] for row in want[0].tolist()]
    assert any(len(row) < 2 for row in lists)


def test_accounting(ctx):
    """The host form is accounted like fm_knn_masked (pairs = nq * real train rows); the device form is not."""
    import torch
    Q, T = _data("clustered", 127, 129, 200)
    qb, tb = ctx.bank(Q), ctx.bank(T)
    try:
        with ctx.mask(127, 129) as mk:
            mk.set_all(True)
            ctx.reset_stats()
            ctx.wide_knn_masked(qb, tb, mk, 2)
            s = ctx.stats()
            assert (s["calls"], s["kernel_launches"], s["pairs"]) == (1, 1, 127 * 129)
            d_idx = torch.empty((127, 2), dtype=torch.int32, device="cuda")
            d_dist = torch.empty((127, 2), dtype=torch.float32, device="cuda")
            ctx.wide_knn_masked_dev(qb, tb, mk, 2, d_idx.data_ptr(), d_dist.data_ptr(), consumer_stream=torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            s = ctx.stats()
            assert (s["calls"], s["kernel_launches"], s["pairs"]) == (1, 1, 127 * 129)
    finally:
        qb.close(); tb.close()


# ---- errors ------------------------------------------------------------------------------------------------------------------
def test_error_order(ctx):
    import torch
    import fastmatch_amd
    rng = np.random.default_rng(3)
    W = rng.standard_normal((40, 256)).astype(np.float32)
    qb, tb = ctx.bank(W), ctx.bank(W[:30])
    w200 = ctx.bank(W[:30, :200])
    f128, f128e = ctx.bank(W[:30, :128]), ctx.bank(np.zeros((0, 128), np.float32))
    u8 = ctx.bank(np.zeros((30, 128), np.uint8))
    binb = ctx.bank_binary(np.zeros((30, 32), np.uint8))
    n = qb.n
    i2, f2 = np.zeros((n, 2), np.int32), np.zeros((n, 2), np.float32)
    d_idx = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
    d_dist = torch.zeros((n, 2), dtype=torch.float32, device="cuda")
    p = lambda a: a.ctypes.data                                 # noqa: E731
    EINVAL, EUNSUPPORTED = -1, -4
    other = fastmatch_amd.Context(0)

    def host(q, t, m, k, idx=i2, dist=f2):
        return ctx.lib.fm_wide_knn_masked(ctx.handle, q, t, m, k, p(idx) if idx is not None else None, p(dist) if dist is not None else None)

    def dev(q, t, m, k, idx=d_idx, dist=d_dist):
        return ctx.lib.fm_wide_knn_masked_dev(ctx.handle, q, t, m, k, idx.data_ptr() if idx is not None else None,
                                              dist.data_ptr() if dist is not None else None, None)

    def err():
        return ctx.lib.fm_last_error(ctx.handle).decode()

    try:
        with ctx.mask(n, 30) as mk, ctx.mask(n, 29) as m29, ctx.mask(n - 1, 30) as mq, other.mask(n, 30) as mo, ctx.mask(n, 0) as m0:
            mk.set_all(True)
            for call in (host, dev):
                # (1) NULL handles -- before everything else, a bad k included
                assert ctx.lib.fm_wide_knn_masked(None, qb.handle, tb.handle, mk.handle, 2, p(i2), p(f2)) == EINVAL
                assert call(None, tb.handle, mk.handle, 0) == EINVAL and "bank is NULL" in err()
                assert call(qb.handle, None, mk.handle, 0) == EINVAL and "bank is NULL" in err()
                assert call(qb.handle, tb.handle, None, 0) == EINVAL and "mask is NULL" in err()
                # (2) the kinds, even of an empty bank, before k; the message names the call that serves them
                for bad in (f128, f128e, u8, binb):
                    assert call(qb.handle, bad.handle, mk.handle, 0) == EINVAL and "fm_knn_masked" in err() and "FM_BANK_F32W" in err()
                    assert call(bad.handle, tb.handle, mk.handle, 9) == EINVAL and "fm_knn_masked" in err()
                assert call(qb.handle, w200.handle, mk.handle, 0) == EINVAL and "dim mismatch" in err()
                # (3) k, before the mask checks
                assert call(qb.handle, tb.handle, m29.handle, 0) == EINVAL and "k must be at least 1" in err()
                assert call(qb.handle, tb.handle, m29.handle, -1) == EINVAL and "k must be at least 1" in err()
                for k in (3, 8, 9):
                    assert call(qb.handle, tb.handle, m29.handle, k) == EUNSUPPORTED and "k >= 3" in err()
                # (4) the mask, before the output pointers
                assert call(qb.handle, tb.handle, mo.handle, 2, None, None) == EINVAL and "another context" in err()
                assert call(qb.handle, tb.handle, mq.handle, 2, None, None) == EINVAL and "query rows" in err()
                assert call(qb.handle, tb.handle, m29.handle, 2, None, None) == EINVAL and "train rows" in err()
                assert call(qb.handle, tb.handle, m0.handle, 2, None, None) == EINVAL and "train rows" in err()
                # (5) the output pointers
                assert call(qb.handle, tb.handle, mk.handle, 2, None, None) == EINVAL and "output pointer is NULL" in err()
            with ctx.collection() as col:
                col.add(W[:30, :128])
                with col.mask(n) as cm:
                    for call in (host, dev):
                        assert call(qb.handle, tb.handle, cm.handle, 2, None, None) == EINVAL and "collection" in err()
            # the device form: fm_knn_dev's pointer checks -- host memory is refused
            assert ctx.lib.fm_wide_knn_masked_dev(ctx.handle, qb.handle, tb.handle, mk.handle, 2, p(i2), p(f2), None) == EINVAL
            assert "d_idx" in err()
            # valid: nq = 0 needs no output, nt = 0 gives -1 / +inf
            with ctx.mask(0, 30) as me:
                qe = ctx.bank(np.zeros((0, 256), np.float32))
                assert host(qe.handle, tb.handle, me.handle, 2, None, None) == 0 and dev(qe.handle, tb.handle, me.handle, 1, None, None) == 0
                qe.close()
            te = ctx.bank(np.zeros((0, 256), np.float32))
            assert host(qb.handle, te.handle, m0.handle, 2) == 0 and (i2 == -1).all() and np.isinf(f2).all()
            te.close()
            # fm_knn_masked keeps refusing wide banks, and says "wide"
            assert ctx.lib.fm_knn_masked(ctx.handle, qb.handle, tb.handle, mk.handle, 2, p(i2), p(f2)) == EUNSUPPORTED and "wide" in err()
    finally:
        for b in (qb, tb, w200, f128, f128e, u8, binb):
            b.close()
        other.close()


# ---- fuzz --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(40))
def test_fuzz(ctx, seed):
    rng = np.random.default_rng(1000 + seed)
    dim = int(rng.integers(129, 257))
    nq, nt = int(rng.integers(1, 301)), int(rng.integers(1, 1501))
    k = int(rng.integers(1, 3))
    density = float(rng.choice([0.002, 0.02, 0.3, 0.9, 1.0]))
    regime = str(rng.choice(["clustered", "gaussian", "spread", "integers"]))
    Q, T = wide_ref.REGIMES[regime](nq, nt, dim, 2000 + seed) if nt > 1 else wide_ref.gaussian(nq, nt, dim, 2000 + seed)
    m = (rng.random((nq, nt)) < density).astype(np.uint8)
    want = WM.knn(Q, T, m, k)
    qb, tb = ctx.bank(Q), ctx.bank(T)
    try:
        for filt, nsplit in ((0, 0), (2, 0), (2, int(rng.integers(1, 6)))):
            with _Filter(ctx, filt, nsplit):
                _same(_masked(ctx, qb, tb, m, k), want, (seed, regime, dim, nq, nt, k, density, filt, nsplit))
    finally:
        qb.close(); tb.close()
