"""GPU: wide float banks (FM_BANK_F32W, 129 .. 256 values per row; wide_f32.hip).  Every result is compared bit for bit with
the oracle's order-1 chain (tests/wide_ref.py), under the exact kernel alone ("f32_filter" 0) and under the fp16 matrix-core
filter forced on (2): the default rule would keep most of these sizes off the filter."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

import fastmatch_amd
from fastmatch_amd import _ffi, matchutil

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wide_ref as ref          # noqa: E402

pytestmark = pytest.mark.gpu

FILTERS = [0, 2]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same(got, want, what):
    got = got if isinstance(got, tuple) else (got,)
    want = want if isinstance(want, tuple) else (want,)
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape, (what, i, g.shape, w.shape)
        assert np.array_equal(_bits(g), _bits(w)), (what, i)


@functools.lru_cache(maxsize=None)
def _data(regime, nq, nt, dim, seed=7):
    if nq == 0 or nt == 0:
        rng = np.random.default_rng(seed)
        Q, T = rng.standard_normal((nq, dim)).astype(np.float32), rng.standard_normal((nt, dim)).astype(np.float32)
    elif nt == 1 and regime in ("clustered", "copies", "dup_queries"):
        Q, T = ref.gaussian(nq, nt, dim, seed)
    else:
        Q, T = ref.REGIMES[regime](nq, nt, dim, seed)
    Q.setflags(write=False)
    T.setflags(write=False)
    return Q, T


@functools.lru_cache(maxsize=None)
def _want(regime, nq, nt, dim, seed=7):
    """The reference of every served call, computed once per data set."""
    Q, T = _data(regime, nq, nt, dim, seed)
    out = {"knn2": ref.knn(Q, T, 2), "knn1": ref.knn(Q, T, 1), "xcheck1": ref.xcheck1(Q, T),
           "ratio0.8": ref.ratio_match(Q, T, 0.8), "ratioinf": ref.ratio_match(Q, T, np.inf),
           "mutual0": ref.mutual_ratio(Q, T, 0.8, False), "mutual1": ref.mutual_ratio(Q, T, 0.8, True)}
    return out


def _check_all(c, qb, tb, want, what):
    _same(c.knn2(qb, tb), want["knn2"], (what, "knn2"))
    _same(c.knn(qb, tb, 1), want["knn1"], (what, "knn k=1"))
    _same(c.xcheck1(qb, tb), want["xcheck1"], (what, "xcheck1"))
    _same(c.knn2_ratio(qb, tb, 0.8), want["ratio0.8"], (what, "knn2_ratio 0.8"))
    _same(c.knn2_ratio(qb, tb, np.inf), want["ratioinf"], (what, "knn2_ratio inf"))
    _same(c.mutual_ratio(qb, tb, 0.8, False), want["mutual0"], (what, "mutual_ratio"))
    _same(c.mutual_ratio(qb, tb, 0.8, True), want["mutual1"], (what, "mutual_ratio symmetric"))


@pytest.fixture(params=FILTERS, ids=["exact", "filter"])
def fctx(request, ctx):
    old = ctx.get_option("f32_filter")
    ctx.set_option("f32_filter", request.param)
    yield request.param, ctx
    ctx.set_option("f32_filter", old)


def test_a_256_d_bank_is_created_and_matches(ctx):
    """Red without the feature: the parent refuses dim > 128."""
    Q, T = _data("clustered", 300, 300, 256)
    qb, tb = ctx.bank(Q), ctx.bank(T)
    try:
        assert (qb.n, qb.dim, qb.kind) == (300, 256, _ffi.FM_BANK_F32W) and tb.kind == 4
        _same(ctx.knn2(qb, tb), ref.knn(Q, T, 2), "knn2")
        _same(ctx.xcheck1(qb, tb), ref.xcheck1(Q, T), "xcheck1")
    finally:
        qb.close(); tb.close()
    # n = 0 is a wide bank too, fm_bank_create_f32_route makes the same kind, integer values do not change it
    for b in (ctx.bank(np.zeros((0, 200), np.float32)), ctx.bank(np.ones((3, 129), np.float32), float_route=True),
              ctx.bank(np.arange(2 * 256).reshape(2, 256) % 256)):
        assert b.kind == _ffi.FM_BANK_F32W and b.dim in (200, 129, 256)
        b.close()


PARITY = [(d, s) for d in ref.DIMS for s in ref.SHAPES if s not in ref.LARGE or d in (129, 256)]


@pytest.mark.parametrize("dim,shape", PARITY, ids=["%d-%dx%d" % (d, s[0], s[1]) for d, s in PARITY])
def test_parity_with_the_oracle(fctx, dim, shape):
    mode, c = fctx
    Q, T = _data("clustered", shape[0], shape[1], dim)
    qb, tb = c.bank(Q), c.bank(T)
    try:
        assert qb.kind == tb.kind == _ffi.FM_BANK_F32W and qb.dim == dim
        _check_all(c, qb, tb, _want("clustered", shape[0], shape[1], dim), (mode, dim, shape))
    finally:
        qb.close(); tb.close()


@pytest.mark.parametrize("shape,dim", [((300, 257), 161), ((1000, 4099), 256)], ids=["300x257-161", "1000x4099-256"])
@pytest.mark.parametrize("regime", sorted(ref.REGIMES))
def test_data_regimes(fctx, regime, shape, dim):
    mode, c = fctx
    Q, T = _data(regime, shape[0], shape[1], dim)
    want = _want(regime, shape[0], shape[1], dim)
    qb, tb = c.bank(Q), c.bank(T)
    try:
        assert qb.kind == tb.kind == _ffi.FM_BANK_F32W              # integer-valued rows included
        before = c.f32_filter_stats()
        _check_all(c, qb, tb, want, (mode, regime, shape))
        after = c.f32_filter_stats()
        if mode == 0 or regime not in ref.FILTERED:
            assert after[0] == before[0]                             # the exact kernel alone (a value that is not finite: always)
        else:
            assert after[0] > before[0]
        if regime == "copies":
            # the lowest index of the copies wins first and second place
            vals, counts = np.unique(np.asarray(T)[:, 0], return_counts=True)
            rows = np.nonzero(np.asarray(T)[:, 0] == vals[counts.argmax()])[0]
            idx = c.knn2(qb, tb)[0][:shape[0] // 2]
            assert len(rows) >= 256 and (idx[:, 0] == rows[0]).all() and (idx[:, 1] == rows[1]).all()
        if regime == "dup_queries":
            tidx = c.xcheck1(qb, tb)[0]
            assert (tidx[0::3] >= 0).any() and (tidx[1::3] == -1).all()      # of two equal query rows the lower index is elected
    finally:
        qb.close(); tb.close()


@pytest.mark.parametrize("shape", [(300, 257), (1000, 4099), (4099, 1000)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("dim", [129, 160, 256])
def test_clustered_set_never_falls_back(ctx, dim, shape):
    """A fallback must not hide a broken filter: on the clustered set (tests/test_wide_host.py asserts its margin census) the
    filter answers every sweep itself."""
    old = ctx.get_option("f32_filter")
    ctx.set_option("f32_filter", 2)
    Q, T = _data("clustered", shape[0], shape[1], dim)
    want = _want("clustered", shape[0], shape[1], dim)
    qb, tb = ctx.bank(Q), ctx.bank(T)
    try:
        l0, f0 = ctx.f32_filter_stats()
        _same(ctx.knn2(qb, tb), want["knn2"], "knn2")
        _same(ctx.xcheck1(qb, tb), want["xcheck1"], "xcheck1")
        _same(ctx.knn(qb, tb, 1), want["knn1"], "knn1")
        l1, f1 = ctx.f32_filter_stats()
        assert l1 - l0 == 3 and f1 - f0 == 0, (l1 - l0, f1 - f0)
    finally:
        ctx.set_option("f32_filter", old)
        qb.close(); tb.close()


def test_the_list_overflow_falls_back_to_the_exact_kernel(ctx):
    """More records than the list holds: 2100 identical train rows are all inside every query row's margin, 600 query rows
    make 1.26M records against a capacity of 2^20; the exact kernel redoes the call and the fallback is counted."""
    rng = np.random.default_rng(11)
    T = np.repeat(rng.standard_normal((1, 192)).astype(np.float32), 2100, axis=0)
    Q = (T[:600] + 1e-3 * rng.standard_normal((600, 192))).astype(np.float32)
    old = ctx.get_option("f32_filter")
    ctx.set_option("f32_filter", 2)
    qb, tb = ctx.bank(Q), ctx.bank(T)
    try:
        l0, f0 = ctx.f32_filter_stats()
        idx, dist = ctx.knn2(qb, tb)
        l1, f1 = ctx.f32_filter_stats()
        assert (l1 - l0, f1 - f0) == (1, 1)
        _same((idx, dist), ref.knn(Q, T, 2), "knn2")
        assert (idx == [0, 1]).all()
    finally:
        ctx.set_option("f32_filter", old)
        qb.close(); tb.close()


def test_the_overflow_is_sticky_past_2_32_records(ctx):
    """Two banks of 65536 identical rows: every one of the 2^32 pairs is inside the margin, so a sweep would reserve 2^32
    record slots -- a 32-bit count would be back at 0 and the rescoring would see an empty list.  The count is 64-bit and a
    wave stops recording once the list is full: the call falls back and every row gets (0, 1) at distance 0."""
    Z = np.zeros((65536, 129), np.float32)
    old = ctx.get_option("f32_filter")
    ctx.set_option("f32_filter", 1)                     # the default rule: 2^32 pairs are far above 4e6
    qb, tb = ctx.bank(Z), ctx.bank(Z)
    try:
        l0, f0 = ctx.f32_filter_stats()
        idx, dist = ctx.knn2(qb, tb)
        l1, f1 = ctx.f32_filter_stats()
        assert (l1 - l0, f1 - f0) == (1, 1)
        assert (idx == [0, 1]).all() and (dist == 0).all()
        tidx, d1 = ctx.xcheck1(qb, tb)
        assert tidx[0] == 0 and (tidx[1:] == -1).all() and d1[0] == 0     # every train row elects query row 0
    finally:
        ctx.set_option("f32_filter", old)
        qb.close(); tb.close()


@pytest.mark.parametrize("shape,dim", [((300, 257), 192), ((1000, 4099), 129)], ids=["300x257-192", "1000x4099-129"])
def test_option_invariance(ctx, shape, dim):
    Q, T = _data("gaussian", shape[0], shape[1], dim)
    want = _want("gaussian", shape[0], shape[1], dim)
    qb, tb = ctx.bank(Q), ctx.bank(T)
    saved = {k: ctx.get_option(k) for k in ("f32_filter", "f32_nsplit", "nsplit")}
    try:
        for filt, fsplit, nsplit in [(0, 0, 0), (0, 0, 1), (0, 0, 3), (1, 0, 0), (2, 0, 0), (2, 1, 0), (2, 3, 0), (2, 7, 2), (2, 1000, 0)]:
            ctx.set_option("f32_filter", filt)
            ctx.set_option("f32_nsplit", fsplit)
            ctx.set_option("nsplit", nsplit)
            l0 = ctx.f32_filter_stats()[0]
            _same(ctx.knn2(qb, tb), want["knn2"], (filt, fsplit, nsplit, "knn2"))
            _same(ctx.xcheck1(qb, tb), want["xcheck1"], (filt, fsplit, nsplit, "xcheck1"))
            _same(ctx.mutual_ratio(qb, tb, 0.8, True), want["mutual1"], (filt, fsplit, nsplit, "mutual"))
            grown = ctx.f32_filter_stats()[0] - l0
            # "f32_filter" 1: the filter from nq * nt >= 4e6 on -- 1000 x 4099 is above, 300 x 257 below
            assert (grown > 0) == (filt == 2 or (filt == 1 and shape[0] * shape[1] >= 4e6)), (filt, grown)
    finally:
        for k, v in saved.items():
            ctx.set_option(k, v)
        qb.close(); tb.close()


def test_banks_of_different_scales(fctx):
    """The two banks' powers of two differ: the filter rescales (up to 2^8), beyond that the exact kernel answers."""
    mode, c = fctx
    Q, T = _data("gaussian", 300, 257, 200)
    for f in (2.0 ** -7, 3.0, 2.0 ** 12):
        Qs = (np.asarray(Q) * np.float32(f)).astype(np.float32)
        qb, tb = c.bank(Qs), c.bank(T)
        try:
            _same(c.knn2(qb, tb), ref.knn(Qs, T, 2), ("knn2", f))
            _same(c.xcheck1(qb, tb), ref.xcheck1(Qs, T), ("xcheck1", f))
        finally:
            qb.close(); tb.close()


# ---- device sources and device results ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [129, 256])
def test_device_banks_and_device_forms(fctx, dim):
    import torch
    from fastmatch_amd import torchmatch
    mode, c = fctx
    Q, T = _data("gaussian", 300, 257, dim)
    tq, tt = torch.from_numpy(np.array(Q)).cuda(), torch.from_numpy(np.array(T)).cuda()
    wide_q = torch.zeros((300, dim + 37), dtype=torch.float32, device="cuda")
    wide_q[:, 5:5 + dim] = tq
    sources = {"float32": (tq, tt), "float16": (tq.half(), tt.half()), "bfloat16": (tq.bfloat16(), tt.bfloat16()),
               "pitched": (wide_q[:, 5:5 + dim], tt)}
    for name, (dq, dt) in sources.items():
        hq, ht = dq.float().cpu().numpy(), dt.float().cpu().numpy()          # the values the device bank holds, exactly
        hqb, htb = c.bank(hq), c.bank(ht)
        dqb, dtb = torchmatch.bank(dq, context=c), torchmatch.bank(dt, context=c)
        try:
            assert (dqb.n, dqb.dim, dqb.kind) == (300, dim, _ffi.FM_BANK_F32W)
            want = {"knn2": c.knn2(hqb, htb), "xcheck1": c.xcheck1(hqb, htb), "ratio": c.knn2_ratio(hqb, htb, 0.9),
                    "mutual": c.mutual_ratio(hqb, htb, 0.9, True)}
            _same(want["knn2"], ref.knn(hq, ht, 2), (name, "host bank against the oracle"))
            # the device-created bank answers as the host-created one
            _same(c.knn2(dqb, dtb), want["knn2"], (name, "knn2"))
            _same(c.xcheck1(dqb, dtb), want["xcheck1"], (name, "xcheck1"))
            _same(c.mutual_ratio(dqb, dtb, 0.9, True), want["mutual"], (name, "mutual"))
            # each device form equals its host form
            for k in (1, 2):
                idx, dist = torchmatch.knn(dq, dt, k)
                _same((idx.cpu().numpy(), dist.cpu().numpy()), (want["knn2"][0][:, :k], want["knn2"][1][:, :k]), (name, "knn_dev", k))
            tidx, dist = torchmatch.mutual_nn(dqb, dtb)
            _same((tidx.cpu().numpy(), dist.cpu().numpy()), want["xcheck1"], (name, "xcheck1_dev"))
            got = torchmatch.ratio_match(dq, dtb, 0.9)
            _same(tuple(x.cpu().numpy() for x in got), want["ratio"][:3], (name, "knn2_ratio_dev"))
            got = torchmatch.mutual_ratio_match(dqb, dt, 0.9, symmetric=True)
            _same(tuple(x.cpu().numpy() for x in got), want["mutual"][:3], (name, "mutual_ratio_dev"))
        finally:
            for b in (hqb, htb, dqb, dtb):
                b.close()


def test_matchutil_takes_a_256_d_pair(ctx):
    Q, T = _data("clustered", 300, 257, 256)
    want = _want("clustered", 300, 257, 256)
    opts = {"context": ctx}
    _same(matchutil.bf_match_arrays(Q, T, k=2, options=opts), want["knn2"], "bf_match k=2")
    _same(matchutil.bf_match_arrays(Q, T, k=1, options=opts), want["knn1"], "bf_match k=1")
    _same(matchutil.bf_match_arrays(Q, T, k=1, options=dict(opts, crossCheck=True)), want["xcheck1"], "crossCheck")
    _same(matchutil.ratio_match_arrays(Q, T, 0.8, options=opts), want["ratio0.8"], "ratio_match_arrays")
    _same(matchutil.mutual_ratio_match_arrays(Q, T, 0.8, True, options=opts), want["mutual1"], "mutual_ratio_match_arrays")
    lists = matchutil.bf_match(Q[:5], T, k=2, options=opts)
    assert [[m.trainIdx for m in row] for row in lists] == want["knn2"][0][:5].tolist()


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def _rc(ctx, fn, *args):
    return getattr(ctx.lib, fn)(ctx.handle, *args)


def test_refusals(ctx):
    import torch
    rng = np.random.default_rng(3)
    W = rng.standard_normal((40, 256)).astype(np.float32)
    qb, tb = ctx.bank(W), ctx.bank(W[:30])
    w200, we = ctx.bank(W[:, :200]), ctx.bank(np.zeros((0, 256), np.float32))
    f128 = ctx.bank(W[:, :128])
    f128e = ctx.bank(np.zeros((0, 128), np.float32))
    n = qb.n
    i32, f32, f64, u8 = np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros(n, np.float64), np.zeros(n, np.uint8)
    cnt = ctypes.c_int64(0)
    d_rows = torch.zeros(3 * n, dtype=torch.int32, device="cuda")
    d_cnt = torch.zeros(2 * n, dtype=torch.int64, device="cuda")
    P = ctypes.c_void_p
    p = lambda a: a.ctypes.data                                 # noqa: E731
    E = -4                                                      # FM_EUNSUPPORTED

    def refused(rc, what):
        assert rc == E, (what, rc)
        assert "wide" in ctx.lib.fm_last_error(ctx.handle).decode(), what

    try:
        offs = np.zeros(n + 1, np.int64)
        i3, f3 = np.zeros((n, 3), np.int32), np.zeros((n, 3), np.float32)
        refused(_rc(ctx, "fm_knn", qb.handle, tb.handle, 3, p(i3), p(f3)), "fm_knn k = 3")
        refused(_rc(ctx, "fm_knn_dev", qb.handle, tb.handle, 3, d_rows.data_ptr(), d_rows.data_ptr(), None), "fm_knn_dev k = 3")
        refused(_rc(ctx, "fm_radius_match", qb.handle, tb.handle, None, 5.0, 0, p(offs), None, None, ctypes.byref(cnt)), "fm_radius_match")
        refused(_rc(ctx, "fm_radius_match_dev", qb.handle, tb.handle, None, 5.0, 0, d_cnt.data_ptr(), None, None, ctypes.byref(cnt), None),
                "fm_radius_match_dev")
        refused(_rc(ctx, "fm_self_dist", qb.handle, p(f64)), "fm_self_dist")
        refused(_rc(ctx, "fm_self_dist_batch", 1, (P * 1)(qb.handle), None), "fm_self_dist_batch")
        refused(_rc(ctx, "fm_bank_set_selfdist", qb.handle, p(f64)), "fm_bank_set_selfdist")
        refused(_rc(ctx, "fm_match_ratio", qb.handle, tb.handle, 0.8, p(i32), p(f32), p(f64), p(u8), ctypes.byref(cnt)), "fm_match_ratio")
        refused(_rc(ctx, "fm_match_accepted", qb.handle, tb.handle, 0.8, n, p(i32), p(i32), p(f32), p(f64), ctypes.byref(cnt)), "fm_match_accepted")
        refused(_rc(ctx, "fm_match_accepted_async", qb.handle, tb.handle, 0.8, n, p(i32), p(i32), p(f32), p(f64), p(offs)), "fm_match_accepted_async")
        refused(_rc(ctx, "fm_match_accepted_dev", qb.handle, tb.handle, 0.8, n, d_rows.data_ptr(), d_cnt.data_ptr(), None), "fm_match_accepted_dev")
        refused(_rc(ctx, "fm_match_accepted_dev_async", qb.handle, tb.handle, 0.8, n, d_rows.data_ptr(), d_cnt.data_ptr(), None, P(-1)),
                "fm_match_accepted_dev_async")
        pq, pt = (P * 1)(qb.handle), (P * 1)(tb.handle)
        outs = [(P * 1)(p(a)) for a in (i32, i32, f32, f64, offs)]
        refused(_rc(ctx, "fm_match_accepted_batch", 1, pq, pt, 0.8, n, *outs), "fm_match_accepted_batch")
        refused(_rc(ctx, "fm_match_accepted_dev_batch", 1, pq, pt, 0.8, n, d_rows.data_ptr(), d_cnt.data_ptr(), None, P(-1)), "fm_match_accepted_dev_batch")
        keys = np.zeros(n, np.uint64)
        refused(_rc(ctx, "fm_xcheck1_keys", qb.handle, tb.handle, 0, p(keys)), "fm_xcheck1_keys")
        refused(_rc(ctx, "fm_xcheck1_keys_dev", qb.handle, tb.handle, 0, d_cnt.data_ptr()), "fm_xcheck1_keys_dev")
        qo, to = np.array([0, 2], np.int64), np.array([0, 2], np.int64)
        refused(_rc(ctx, "fm_xcheck1_batched", qb.handle, p(np.arange(2, dtype=np.int32)), p(qo), tb.handle, p(to), 1, p(i32), p(f32), None),
                "fm_xcheck1_batched")
        with ctx.mask(qb.n, tb.n) as mk:
            mk.set_all(True)
            i2, f2 = np.zeros((n, 2), np.int32), np.zeros((n, 2), np.float32)
            refused(_rc(ctx, "fm_knn_masked", qb.handle, tb.handle, mk.handle, 2, p(i2), p(f2)), "fm_knn_masked")
            refused(_rc(ctx, "fm_knn_masked_dev", qb.handle, tb.handle, mk.handle, 2, d_rows.data_ptr(), d_rows.data_ptr(), None), "fm_knn_masked_dev")
        B = np.zeros((10, 256), np.uint8)
        refused(_rc(ctx, "fm_bank_refill_u8_async", qb.handle, p(B), 10), "fm_bank_refill_u8_async")
        first = ctypes.c_int64(0)
        refused(_rc(ctx, "fm_bank_append_u8", qb.handle, p(B), 1, ctypes.byref(first)), "fm_bank_append_u8")
        refused(_rc(ctx, "fm_bank_append_f32", qb.handle, p(W), 1, ctypes.byref(first)), "fm_bank_append_f32")
        desc = _ffi.fm_expand_desc()
        desc.query, desc.target = qb.handle, tb.handle
        ex = P()
        refused(_rc(ctx, "fm_expand_create", ctypes.byref(desc), ctypes.byref(ex)), "fm_expand_create")

        # every fm_collection_* call: the adds, and a wide query bank against an empty and a filled collection
        def coll_refused(call, what):
            with pytest.raises(_ffi.FastMatchHipError, match="wide") as ei:
                call()
            assert ei.value.code == E, what

        for filled in (False, True):
            with ctx.collection() as col:
                if filled:
                    col.add(W[:, :128])
                coll_refused(lambda: col.add(W), "add")
                coll_refused(lambda: col.add_from_device(d_rows.data_ptr(), _ffi.FM_DT_F16, 4, 200), "add_from_device")
                assert col.info()[0] == (1 if filled else 0)
                coll_refused(lambda: col.knn(qb, 2), "knn")
                coll_refused(lambda: col.knn2_ratio(qb, 0.8), "knn2_ratio")
                coll_refused(lambda: col.knn2_each(qb), "knn2_each")
                coll_refused(lambda: col.votes(qb, 0.8), "votes")
                coll_refused(lambda: col.radius_match(qb, 1.0), "radius_match")
                coll_refused(lambda: col.match_accepted_each(qb, 0.8), "match_accepted_each")
                coll_refused(lambda: col.xcheck1_each(qb), "xcheck1_each")
                coll_refused(lambda: col.mutual_ratio_each(qb, 0.8), "mutual_ratio_each")
                dr, dc = d_rows.data_ptr(), d_cnt.data_ptr()
                with col.mask(qb.n) as cm:
                    coll_refused(lambda: col.knn_masked(qb, cm, 2), "knn_masked")
                    coll_refused(lambda: col.knn_masked_dev(qb, cm, 1, dr, dr, dr), "knn_masked_dev")
                # the device forms (valid device pointers: the refusal is the query bank's)
                coll_refused(lambda: col.knn_dev(qb, 1, dr, dr, dr), "knn_dev")
                coll_refused(lambda: col.knn2_ratio_dev(qb, 0.8, dr, dc, 1), "knn2_ratio_dev")
                coll_refused(lambda: col.radius_match_dev(qb, 0, 1.0, 0, dc, 0, 0, 0), "radius_match_dev")
                coll_refused(lambda: col.match_accepted_each_dev(qb, 0.8, dr, dc, 1), "match_accepted_each_dev")
                coll_refused(lambda: col.xcheck1_each_dev(qb, float("inf"), dr, dc, 1), "xcheck1_each_dev")
                coll_refused(lambda: col.mutual_ratio_each_dev(qb, 0.8, False, dr, dc, 1), "mutual_ratio_each_dev")

        # pairing: another kind or another dim is FM_EINVAL, an empty bank on either side included
        idx2, d2 = np.zeros((n, 2), np.int32), np.zeros((n, 2), np.float32)
        for a, b in ((qb, f128), (f128, qb), (qb, f128e), (f128e, qb), (we, f128), (w200, qb), (qb, w200), (we, w200), (w200, we)):
            for fn in ("fm_knn2", "fm_knn"):
                args = (2,) if fn == "fm_knn" else ()
                assert _rc(ctx, fn, a.handle, b.handle, *args, p(idx2), p(d2)) == -1, fn
            assert _rc(ctx, "fm_xcheck1", a.handle, b.handle, p(i32), p(f32)) == -1
            assert _rc(ctx, "fm_knn2_ratio", a.handle, b.handle, 0.8, n, p(i32), p(i32), p(f32), p(f64), ctypes.byref(cnt)) == -1
            assert _rc(ctx, "fm_mutual_ratio", a.handle, b.handle, 0.8, 0, n, p(i32), p(i32), p(f32), p(f64), ctypes.byref(cnt)) == -1
        # widths
        h = P()
        Z = np.zeros((4, 257), np.float32)
        assert _rc(ctx, "fm_bank_create_f32", p(Z), 4, 257, ctypes.byref(h)) == E and h.value is None
        assert _rc(ctx, "fm_bank_create_f32_route", p(Z), 4, 257, ctypes.byref(h)) == E
        assert _rc(ctx, "fm_bank_create_u8", p(B), 4, 200, ctypes.byref(h)) == E
        assert _rc(ctx, "fm_bank_create_dev", d_rows.data_ptr(), _ffi.FM_DT_F32, 0, 257, 0, 0, None, ctypes.byref(h)) == E
        assert _rc(ctx, "fm_bank_create_dev", d_rows.data_ptr(), _ffi.FM_DT_U8, 0, 200, 0, 0, None, ctypes.byref(h)) == E
        # the context still answers: a 128-D call, and the wide banks themselves
        _same(ctx.knn2(f128, f128), ref.knn(W[:, :128], W[:, :128], 2), "128-D knn2 after the refusals")
        _same(ctx.knn2(qb, tb), ref.knn(W, W[:30], 2), "wide knn2 after the refusals")
        _same(ctx.knn2(we, tb), ref.knn(W[:0], W[:30], 2), "an empty query bank")
        _same(ctx.knn2(qb, we), ref.knn(W, W[:0], 2), "an empty train bank")
    finally:
        for b in (qb, tb, w200, we, f128, f128e):
            b.close()


def test_bank_cycles_give_the_memory_back():
    c = fastmatch_amd.Context(0)
    rng = np.random.default_rng(5)
    W = rng.standard_normal((700, 256)).astype(np.float32)

    def cycle(k):
        c.set_option("f32_filter", 2 if k % 2 else 0)
        qb, tb = c.bank(W[: 300 + k % 100, : 129 + k % 128]), c.bank(W[: 600 + k % 100, : 129 + k % 128])
        c.knn2(qb, tb)
        if k % 10 == 0:
            c.xcheck1(qb, tb)
            c.mutual_ratio(qb, tb, 0.9, True)
        qb.close(); tb.close()
    for k in range(20):
        cycle(k)
    c.sync()
    base = c.mem_info()[0]
    for k in range(200):
        cycle(k)
    c.sync()
    after = c.mem_info()[0]
    assert base - after <= (4 << 20), (base, after)
    c.close()
