"""GPU: Fast-Match's self-distance test on wide float descriptors (FM_BANK_F32W, 129 .. 256 values per row) --
fm_wide_self_dist(_batch), fm_wide_set_selfdist, fm_wide_match_ratio, fm_wide_match_accepted(_dev),
fm_collection_wide_match_accepted_each(_dev) and the Python layers on top -- against the NumPy reference
(tests/wide_fast_ref.py over tests/wide_ref.py, the oracle's order-1 chain).  Every comparison is exact: integers, float32
and float64 bit patterns (NaNs by position); there is no tolerance anywhere.  Every test runs under the exact kernel alone
("f32_filter" 0) and under the fp16 matrix-core filter forced on (2) unless it says otherwise.

Shapes follow the self sweep's geometry: the filter's tile is 16 reduced rows, a wave owns two blocks of 16 output rows and a
workgroup 128, the exact kernel steps over 64 x 64 rows; the sizes put the diagonal in every lane group of a tile, in the last
partial tile and, with "f32_nsplit", in different splits."""
import ctypes
import functools

import numpy as np
import pytest

import fastmatch_amd
import wide_fast_ref as WF
import wide_ref as ref
from fastmatch_amd import _ffi, matchutil

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -4
INF = float("inf")
FILTERS = [0, 2]
SIZES = [0, 1, 2, 3, 17, 127, 128, 129, 300, 640, 1000]
TAUS = [0.0, 0.6, 0.8, 1.0, INF]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


@pytest.fixture(params=FILTERS, ids=["exact", "filter"])
def fctx(request, ctx):
    old = ctx.get_option("f32_filter")
    ctx.set_option("f32_filter", request.param)
    yield request.param, ctx
    ctx.set_option("f32_filter", old)


@functools.lru_cache(maxsize=None)
def _bank_rows(n, dim, seed=7):
    """One bank of n rows: unit-norm rows on a 16-D subspace plus noise (wide_ref.clustered's train side)."""
    X = ref.clustered(1, n, dim, seed)[1] if n else np.zeros((0, dim), np.float32)
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def _self_ref(n, dim, seed=7):
    sd = WF.self_dist(_bank_rows(n, dim, seed))
    sd.setflags(write=False)
    return sd


def _check_self(c, X, want, what, second=True):
    """fm_wide_self_dist of a bank of X against `want`; returns what the call added to fm_f32_filter_stats."""
    b = c.bank(X)
    try:
        assert b.kind == _ffi.FM_BANK_F32W
        l0, f0 = c.f32_filter_stats()
        got = c.wide_self_dist(b)
        l1, f1 = c.f32_filter_stats()
        assert got.dtype == np.float64 and _same(got, want), (what, np.nonzero(_bits(got) != _bits(want))[0][:8])
        if second and len(X) >= 2:
            # a bank whose values are all finite: the second column of fm_knn2(b, b), the value only
            assert _same(got, c.knn2(b, b)[1][:, 1].astype(np.float64)), what
    finally:
        b.close()
    return l1 - l0, f1 - f0


# ---- self distances ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [129, 160, 256])
def test_self_dist_sizes(fctx, dim):
    mode, c = fctx
    for n in SIZES + ([4099] if dim in (129, 256) else []):
        want = _self_ref(n, dim)
        if n == 1:
            assert want[0] == np.inf
        _check_self(c, _bank_rows(n, dim), want, (mode, dim, n))


@pytest.mark.parametrize("nsplit", [1, 3, 7])
def test_self_dist_splits(ctx, nsplit):
    """1000 rows are 63 tiles (64 with the padding); under 1, 3 and 7 splits the diagonal tiles of the eight workgroups fall
    into different splits, and most splits of a workgroup hold no diagonal at all."""
    saved = {k: ctx.get_option(k) for k in ("f32_filter", "f32_nsplit")}
    ctx.set_option("f32_filter", 2)
    ctx.set_option("f32_nsplit", nsplit)
    try:
        for dim in (129, 256):
            assert _check_self(ctx, _bank_rows(1000, dim), _self_ref(1000, dim), (nsplit, dim), second=False) == (1, 0)
    finally:
        for k, v in saved.items():
            ctx.set_option(k, v)


@pytest.mark.parametrize("n,dim", [(300, 161), (1000, 256)], ids=["300-161", "1000-256"])
@pytest.mark.parametrize("regime", sorted(ref.REGIMES))
def test_self_dist_regimes(fctx, regime, n, dim):
    """The query array of every regime of tests/wide_ref.py (for `copies` the train array too: that is where the exact copies
    are)."""
    mode, c = fctx
    Q, T = ref.REGIMES[regime](n, n, dim, 7)
    finite = regime in ref.FILTERED
    want = WF.self_dist(Q)
    grown = _check_self(c, Q, want, (mode, regime, n, dim), second=finite)
    # the exact kernel alone under "f32_filter" 0 and for a bank with a value that is not finite; else one filter launch
    assert grown[0] == (1 if mode == 2 and finite else 0), grown
    if regime == "copies":
        wt = WF.self_dist(T)
        vals, counts = np.unique(np.asarray(T)[:, 0], return_counts=True)
        rows = np.nonzero(np.asarray(T)[:, 0] == vals[counts.argmax()])[0]
        assert len(rows) >= 256 and (wt[rows] == 0.0).all() and (wt > 0).any()       # the copies give 0
        _check_self(c, T, wt, (mode, regime, "train side"))
    if regime == "dup_queries":
        assert (want[1::3] == 0.0).all() and (want[0::3][:len(want[1::3])] == 0.0).all() and (want[2::3] > 0).all()
    if regime == "nonfinite":
        # the NaN row and the row with an infinite value give +inf, and neither becomes anyone's minimum
        bad = np.zeros(n, bool)
        bad[[n // 3, n // 2]] = True
        assert np.isinf(want[bad]).all() and np.isfinite(want[~bad]).all()
        clean = WF.self_dist(np.asarray(Q)[~bad])
        assert _same(want[~bad], clean)


def test_the_filter_really_ran(ctx):
    """n = 640, dim 256, "f32_filter" 2, clustered: one filter launch, no fallback.  A condition, not a hope: the record list
    holds at least 2^20 slots (include/fastmatch_hip.h, K14; plan_wide_filter: max(256 n, 2^20)).  Even if every one of the
    640^2 pairs were recorded and consecutive 64-slot chunks were filled only just over half on average -- the worst
    wide_push allows: a chunk is closed when the next push does not fit, and together the two exceed 64 -- the slots used
    stay below 2 * 409 600 plus one open chunk of 64 per wave, and 5 workgroups x 1 split x 4 waves make 20 waves."""
    n, waves = 640, (640 // 128) * 1 * 4
    assert 2 * n * n + 64 * waves < 1 << 20
    old = ctx.get_option("f32_filter")
    ctx.set_option("f32_filter", 2)
    try:
        assert _check_self(ctx, _bank_rows(n, 256), _self_ref(n, 256), "640", second=False) == (1, 0)
    finally:
        ctx.set_option("f32_filter", old)


def test_the_list_overflow_falls_back_to_the_exact_self_kernel(ctx):
    """2100 exact copies of one row plus 500 other rows, dim 256: all 2100 * 2099 copy pairs lie at distance 0 -- their fp16
    scores are equal, so every one of them reaches every bound -- and must be recorded; 4.4e6 > 2^20 slots, so the list
    overflows, the exact SELF kernel redoes the sweep and the fallback is counted."""
    assert 2100 * 2099 > 1 << 20 and 256 * 2600 < 1 << 20
    rng = np.random.default_rng(11)
    X = np.concatenate([np.repeat(rng.standard_normal((1, 256)).astype(np.float32), 2100, axis=0),
                        rng.standard_normal((500, 256)).astype(np.float32)])
    X = X[rng.permutation(len(X))]
    want = WF.self_dist(X)
    assert (want == 0).sum() == 2100
    old = ctx.get_option("f32_filter")
    ctx.set_option("f32_filter", 2)
    try:
        assert _check_self(ctx, X, want, "overflow", second=False) == (1, 1)
    finally:
        ctx.set_option("f32_filter", old)


def test_batched_self_dist_and_stats(fctx):
    """Banks of mixed sizes and dims, one of them empty, in one call: the returned values, the attached ones (through a
    match), a bank listed twice; fm_stats counts n * n pairs per self sweep and nq * nt per match."""
    mode, c = fctx
    shapes = [(300, 256), (1, 129), (130, 160), (0, 256), (640, 129)]
    mats = [_bank_rows(n, d, seed=20 + i) for i, (n, d) in enumerate(shapes)]
    banks = [c.bank(m) for m in mats]
    fresh = [c.bank(m) for m in mats]
    tb = c.bank(_bank_rows(257, 256, seed=3))
    try:
        c.sync()
        c.reset_stats()
        outs = c.wide_self_dist_batch(banks)
        assert c.stats()["pairs"] == sum(n * n for n, _ in shapes)
        assert len(outs) == len(shapes) and all(_same(o, WF.self_dist(m)) for o, m in zip(outs, mats))
        assert all(_same(c.wide_self_dist(b), o) for b, o in zip(banks, outs))
        # the enqueue-only form: nothing comes back, the values are attached on the device
        assert c.wide_self_dist_batch(fresh, want_host=False) is None
        c.sync()
        c.reset_stats()
        got = c.wide_match_ratio(fresh[0], tb, 0.9)
        assert c.stats()["pairs"] == 300 * 257
        rt, rd, rr, rp = WF.match_ratio(mats[0], _bank_rows(257, 256, seed=3), outs[0], 0.9)
        assert _same(got[0], rt) and _same(got[1], rd) and WF.same_f64(got[2], rr) and np.array_equal(got[3], rp) and got[4] == rp.sum()
        hs = (ctypes.c_void_p * 2)(banks[0].handle, banks[0].handle)
        assert c.lib.fm_wide_self_dist_batch(c.handle, 2, hs, None) == EINVAL
        assert "listed twice" in c.lib.fm_last_error(c.handle).decode()
    finally:
        for b in banks + fresh + [tb]:
            b.close()


# ---- bank pairs ------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (2, 2), (1, 300), (129, 127), (300, 257), (1000, 4099)]


@functools.lru_cache(maxsize=None)
def _pair(nq, nt, dim):
    """wide_ref.clustered's pair -- every query row a near copy of a train row, so small ratios exist -- with, from 129 query
    rows on, two exact duplicates inside the query bank: one whose train row is at d > 0 (d / 0 = +inf) and one whose train
    row is an exact copy (0 / 0 = NaN).  Of two equal query rows every train row elects the lower one."""
    Q, T = ref.clustered(nq, nt, dim, 7) if nt > 1 else ref.gaussian(nq, nt, dim, 7)
    Q, T = np.array(Q), np.array(T)
    if nq >= 129:
        Q[17] = Q[4]
        T[5] = Q[4]
        T[5, 0] += np.float32(1e-3)   # ... train row 5 elects query row 4 at d > 0
        Q[30] = Q[8]
        T[9] = Q[8]
    sd = WF.self_dist(Q)
    tidx, dist = ref.xcheck1(Q, T)
    for a in (Q, T, sd, tidx, dist):
        a.setflags(write=False)
    return Q, T, sd, tidx, dist


def _ratio_ref(nq, nt, dim, tau, sd=None):
    Q, T, sd0, tidx, dist = _pair(nq, nt, dim)
    sd = sd0 if sd is None else sd
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = dist.astype(np.float64) / sd
    ratio[tidx < 0] = np.nan
    with np.errstate(invalid="ignore"):
        passed = (tidx >= 0) & (ratio < tau)
    return tidx, dist, ratio, passed


def _accepted_raw(c, qb, tb, tau, cap):
    out = tuple(np.full(max(cap, 1), -9, dt) for dt in (np.int32, np.int32, np.float32, np.float64))
    n = ctypes.c_int64(-1)
    rc = c.lib.fm_wide_match_accepted(c.handle, qb.handle, tb.handle, float(tau), cap, *[_ffi._ptr(a) for a in out], ctypes.byref(n))
    assert rc == 0, c.lib.fm_last_error(c.handle).decode()
    return out, n.value


@pytest.mark.parametrize("dim", [129, 256])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_match_calls(fctx, shape, dim):
    import torch
    mode, c = fctx
    nq, nt = shape
    Q, T, sd, xt, xd = _pair(nq, nt, dim)
    tb = c.bank(T)
    banks = []
    try:
        for source in ("batch", "set"):
            qb = c.bank(Q)
            banks.append(qb)
            if source == "batch":
                assert c.wide_self_dist_batch([qb], want_host=False) is None      # enqueue only, then the match call
            else:
                qb.set_wide_selfdist(sd)                                          # the reference's values
            some_pass = some_fail = False
            for tau in TAUS:
                rt, rd, rr, rp = _ratio_ref(nq, nt, dim, tau)
                assert _same(rt, xt)
                tidx, dist, ratio, passed, npass = c.wide_match_ratio(qb, tb, tau)
                assert _same(tidx, rt) and _same(dist, rd) and WF.same_f64(ratio, rr) and np.array_equal(passed, rp) and npass == rp.sum(), (source, tau)
                aq = np.nonzero(rp)[0].astype(np.int32)
                at, ad, ar = rt[aq], rd[aq], rr[aq]
                m = len(aq)
                some_pass |= m > 0
                some_fail |= bool(((rt >= 0) & ~rp).any())
                host = None
                for cap in (0, m // 2, nq):
                    out, full = _accepted_raw(c, qb, tb, tau, cap)
                    k = min(cap, m)
                    assert full == m, (source, tau, cap, full, m)                 # the FULL count, whatever the capacity
                    assert _same(out[0][:k], aq[:k]) and _same(out[1][:k], at[:k]) and _same(out[2][:k], ad[:k]) and _same(out[3][:k], ar[:k])
                    assert (out[0][k:] == -9).all()
                    host = out
                    rows = torch.full((max(cap, 1), 3), -9, dtype=torch.int32, device="cuda")
                    cnt = torch.full((1,), -9, dtype=torch.int64, device="cuda")
                    torch.cuda.synchronize()
                    assert c.wide_match_accepted_dev(qb, tb, tau, rows.data_ptr(), cnt.data_ptr(), cap) == m
                    r = rows.cpu().numpy()
                    assert int(cnt.item()) == k
                    # the _dev rows equal the host form's, the distance bits included
                    assert _same(r[:k, 0], host[0][:k]) and _same(r[:k, 1], host[1][:k]) and _same(r[:k, 2].view(np.float32), host[2][:k])
                    assert (r[k:] == -9).all()
            if nq == 1:                                            # a bank of one query row: selfdist +inf, the ratio is 0
                assert sd[0] == np.inf and _ratio_ref(nq, nt, dim, 1.0)[2][0] == 0.0 and _ratio_ref(nq, nt, dim, 1.0)[3][0]
            assert some_pass and (some_fail or nq < 129), (some_pass, some_fail)
        if nq >= 129:
            # a query row with a duplicate is never accepted: d / 0 = +inf and 0 / 0 = NaN, at tau = +inf too
            rt, rd, rr, rp = _ratio_ref(nq, nt, dim, INF)
            assert sd[4] == 0 and sd[17] == 0 and sd[8] == 0 and sd[30] == 0 and not rp[[4, 17, 8, 30]].any()
            assert rt[8] == 9 and rd[8] == 0 and np.isnan(rr[8])                  # 0 / 0
            assert rt[4] == 5 and rd[4] > 0 and rr[4] == np.inf and rt[17] == -1  # d / 0; of two equal rows the lower is elected
    finally:
        for b in banks + [tb]:
            b.close()


def test_caller_self_distances_are_honoured(fctx):
    mode, c = fctx
    Q, T, sd, _, _ = _pair(300, 257, 256)
    qb, tb = c.bank(Q), c.bank(T)
    try:
        mine = np.linspace(0.01, 3.0, len(Q))
        mine[3], mine[9] = 0.0, np.inf
        qb.set_wide_selfdist(mine)
        rt, rd, rr, rp = _ratio_ref(300, 257, 256, 0.9, mine)
        tidx, dist, ratio, passed, npass = c.wide_match_ratio(qb, tb, 0.9)
        assert _same(tidx, rt) and WF.same_f64(ratio, rr) and np.array_equal(passed, rp) and npass == rp.sum()
        c.wide_self_dist_batch([qb], want_host=False)         # ... and computed ones replace them
        assert WF.same_f64(c.wide_match_ratio(qb, tb, 0.9)[2], _ratio_ref(300, 257, 256, 0.9)[2])
    finally:
        qb.close(); tb.close()


# ---- collections -----------------------------------------------------------------------------------------------------------
IMAGE_ROWS = [0, 1, 130, 257, 600]


@functools.lru_cache(maxsize=None)
def _coll_data(dim):
    Q, T = ref.clustered(300, sum(IMAGE_ROWS), dim, 13)
    Q = np.array(Q)
    Q[17] = Q[4]
    images, at = [], 0
    for n in IMAGE_ROWS:
        images.append(np.ascontiguousarray(T[at:at + n]))
        at += n
    sd = WF.self_dist(Q)
    want = {tau: WF.fast_match_each(Q, images, tau, sd) for tau in (0.6, INF)}
    return Q, images, sd, want


def _same_rows(got, want):
    return all(_same(g, w) if g.dtype != np.float64 else WF.same_f64(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("device_adds", [False, True], ids=["host-adds", "device-adds"])
@pytest.mark.parametrize("dim", [192, 256])
def test_collection_forms(fctx, dim, device_adds):
    import torch
    mode, c = fctx
    Q, images, sd, want = _coll_data(dim)
    ni = len(images)
    saved = c.get_option("coll_ws_bytes")
    qb = c.bank(Q)
    img_banks = [c.bank(im) for im in images]
    keep = []
    try:
        c.wide_self_dist_batch([qb], want_host=False)
        with c.collection() as col:
            for im in images:
                if device_adds:
                    t = torch.from_numpy(im).cuda()
                    keep.append(t)
                    torch.cuda.synchronize()
                    col.add_wide_from_device(t.data_ptr() if len(im) else 0, _ffi.FM_DT_F32, len(im), dim)
                else:
                    col.add_wide(im)
            assert col.info()[0] == ni and col.info()[3] == _ffi.FM_BANK_F32W
            # the budget of one chunk: 25 bytes per (image, query row) and 4 per block of 256 query rows; room for two images
            # makes three chunks of the five
            per = 300 * 25 + 2 * 4
            for budget in (0, 2 * per + 100):
                c.set_option("coll_ws_bytes", budget)
                chunks = 1 if budget == 0 else -(-ni // (budget // per))
                assert chunks in (1, 3)
                for tau in (0.6, INF):
                    l0, f0 = c.f32_filter_stats()
                    got = col.wide_match_accepted_each(qb, tau)
                    l1, f1 = c.f32_filter_stats()
                    # one filter launch (with its rescoring and its guarded exact launch) per chunk of images, none redone
                    assert (l1 - l0, f1 - f0) == ((chunks if mode == 2 else 0), 0), (budget, l1 - l0, f1 - f0)
                    assert len(got) == ni
                    for i in range(ni):
                        assert _same_rows(got[i], want[tau][i]), (budget, tau, i)
                        # every slot equals fm_wide_match_accepted(q, B_i)
                        assert _same_rows(got[i], c.wide_match_accepted(qb, img_banks[i], tau)), (budget, tau, i)
                    assert len(got[0][0]) == 0 and sum(len(g[0]) for g in got) > 0          # the empty image keeps its slot
                # cap below the counts: the full counts, the first rows
                full = [len(w[0]) for w in want[INF]]
                cap = max(full) // 2
                got = col.wide_match_accepted_each(qb, INF, cap=cap)
                assert [len(g[0]) for g in got] == [min(f, cap) for f in full]
                assert all(_same_rows(g, tuple(a[:cap] for a in w)) for g, w in zip(got, want[INF]))
                # the device form, with a consumer stream
                s = torch.cuda.Stream()
                with torch.cuda.stream(s):
                    rows = torch.full((ni, 300, 3), -9, dtype=torch.int32, device="cuda")
                    counts = torch.full((ni,), -9, dtype=torch.int64, device="cuda")
                    h = np.full(ni, -9, np.int64)
                    col.wide_match_accepted_each_dev(qb, 0.6, rows.data_ptr(), counts.data_ptr(), 300, h_counts=h, consumer_stream=s.cuda_stream)
                    r, k = rows.cpu().numpy(), counts.cpu().numpy()
                assert h.tolist() == k.tolist() == [len(w[0]) for w in want[0.6]]
                for i in range(ni):
                    w = want[0.6][i]
                    m = len(w[0])
                    assert _same(r[i, :m, 0], w[0]) and _same(r[i, :m, 1], w[1]) and _same(r[i, :m, 2].view(np.float32), w[2])
                    assert (r[i, m:] == -9).all()
        # an empty collection gives all zero counts: no image, and images without rows
        with c.collection() as col:
            assert col.wide_match_accepted_each(qb, 0.8) == []
            col.add_wide(np.zeros((0, dim), np.float32))
            col.add_wide(np.zeros((0, dim), np.float32))
            got = col.wide_match_accepted_each(qb, INF)
            assert [len(g[0]) for g in got] == [0, 0]
    finally:
        c.set_option("coll_ws_bytes", saved)
        for b in img_banks + [qb]:
            b.close()


# ---- errors ----------------------------------------------------------------------------------------------------------------
def test_errors_in_the_documented_order(ctx):
    import torch
    rng = np.random.default_rng(3)
    W = rng.standard_normal((40, 256)).astype(np.float32)
    qb, tb, w200 = ctx.bank(W), ctx.bank(W[:30]), ctx.bank(W[:, :200])
    f128 = ctx.bank(W[:, :128])
    bq = ctx.bank_binary(rng.integers(0, 256, (40, 32), dtype=np.uint8))
    empty = ctx.bank(np.zeros((0, 256), np.float32))
    other = fastmatch_amd.Context(0)
    n = qb.n
    i32, f32, f64, u8 = np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros(n, np.float64), np.zeros(n, np.uint8)
    cnt = ctypes.c_int64(0)
    d_rows = torch.zeros(3 * n * 4, dtype=torch.int32, device="cuda")
    d_cnt = torch.zeros(8, dtype=torch.int64, device="cuda")
    P = ctypes.c_void_p
    p = lambda a: a.ctypes.data                                 # noqa: E731
    L, H = ctx.lib, ctx.handle

    def err(rc, code, *words):
        msg = L.fm_last_error(H).decode()
        assert rc == code, (rc, msg)
        for w in words:
            assert w in msg, (w, msg)

    ratio_args = (0.8, p(i32), p(f32), p(f64), p(u8), ctypes.byref(cnt))
    acc_args = (0.8, n, p(i32), p(i32), p(f32), p(f64), ctypes.byref(cnt))
    dev_args = (0.8, n, d_rows.data_ptr(), d_cnt.data_ptr(), None)
    try:
        with ctx.collection() as wcol, ctx.collection() as ncol, ctx.collection() as bcol, other.collection() as ocol:
            wcol.add_wide(W[:30])
            ncol.add(W[:, :128])
            bcol.add_binary(rng.integers(0, 256, (20, 32), dtype=np.uint8))
            ocol.add_wide(W[:30])
            counts = np.zeros(4, np.int64)
            each_args = (0.8, n, p(i32), p(i32), p(f32), p(f64), p(counts))
            each_dev = (0.8, n, d_rows.data_ptr(), d_cnt.data_ptr(), None, None)
            # 1. NULL handles, a collection of another context
            err(L.fm_wide_self_dist(H, None, p(f64)), EINVAL, "NULL")
            err(L.fm_wide_self_dist_batch(H, 1, (P * 1)(None), None), EINVAL, "NULL")
            err(L.fm_wide_set_selfdist(H, None, p(f64)), EINVAL, "NULL")
            err(L.fm_wide_match_ratio(H, None, tb.handle, *ratio_args), EINVAL, "NULL")
            err(L.fm_wide_match_accepted(H, qb.handle, None, *acc_args), EINVAL, "NULL")
            err(L.fm_wide_match_accepted_dev(H, None, None, *dev_args), EINVAL, "NULL")
            err(L.fm_collection_wide_match_accepted_each(H, None, qb.handle, *each_args), EINVAL)
            err(L.fm_collection_wide_match_accepted_each(H, wcol.handle, None, *each_args), EINVAL, "NULL")
            err(L.fm_collection_wide_match_accepted_each(H, ocol.handle, qb.handle, *each_args), EINVAL)
            err(L.fm_collection_wide_match_accepted_each_dev(H, ocol.handle, qb.handle, *each_dev), EINVAL)
            # 2. a bank or a collection that is not wide: the message names the L2 / the Hamming call that serves it
            err(L.fm_wide_self_dist(H, f128.handle, p(f64)), EINVAL, "fm_self_dist is the L2 call")
            err(L.fm_wide_self_dist(H, bq.handle, p(f64)), EINVAL, "fm_hamming_self_dist is the Hamming call")
            err(L.fm_wide_self_dist_batch(H, 2, (P * 2)(qb.handle, f128.handle), None), EINVAL, "fm_self_dist_batch is the L2 call")
            err(L.fm_wide_set_selfdist(H, f128.handle, p(f64)), EINVAL, "fm_bank_set_selfdist is the L2 call")
            err(L.fm_wide_match_ratio(H, f128.handle, f128.handle, *ratio_args), EINVAL, "fm_match_ratio is the L2 call")
            err(L.fm_wide_match_ratio(H, qb.handle, f128.handle, *ratio_args), EINVAL, "fm_match_ratio is the L2 call")
            err(L.fm_wide_match_accepted(H, bq.handle, bq.handle, *acc_args), EINVAL, "fm_hamming_match_accepted is the Hamming call")
            err(L.fm_wide_match_accepted_dev(H, f128.handle, tb.handle, *dev_args), EINVAL, "fm_match_accepted_dev is the L2 call")
            err(L.fm_collection_wide_match_accepted_each(H, ncol.handle, qb.handle, *each_args), EINVAL, "fm_collection_match_accepted_each is the L2 call")
            err(L.fm_collection_wide_match_accepted_each(H, wcol.handle, f128.handle, *each_args), EINVAL, "fm_collection_match_accepted_each is the L2 call")
            err(L.fm_collection_wide_match_accepted_each_dev(H, bcol.handle, bq.handle, *each_dev), EINVAL,
                "fm_collection_hamming_match_accepted_each_dev is the Hamming call")
            # 3. dims that differ
            err(L.fm_wide_match_ratio(H, w200.handle, tb.handle, *ratio_args), EINVAL, "mismatch")
            err(L.fm_wide_match_accepted(H, qb.handle, w200.handle, *acc_args), EINVAL, "mismatch")
            err(L.fm_wide_match_accepted_dev(H, w200.handle, tb.handle, *dev_args), EINVAL, "mismatch")
            err(L.fm_collection_wide_match_accepted_each(H, wcol.handle, w200.handle, *each_args), EINVAL, "width")
            # 4. a query bank with rows but without self distances (before cap and the outputs are looked at)
            err(L.fm_wide_match_ratio(H, qb.handle, tb.handle, 0.8, None, None, None, None, None), EINVAL, "no self distances")
            err(L.fm_wide_match_accepted(H, qb.handle, tb.handle, 0.8, -1, None, None, None, None, None), EINVAL, "no self distances")
            err(L.fm_wide_match_accepted_dev(H, qb.handle, tb.handle, 0.8, -1, None, None, None), EINVAL, "no self distances")
            err(L.fm_collection_wide_match_accepted_each(H, wcol.handle, qb.handle, 0.8, -1, None, None, None, None, None), EINVAL, "no self distances")
            err(L.fm_collection_wide_match_accepted_each_dev(H, wcol.handle, qb.handle, 0.8, -1, None, None, None, None), EINVAL, "no self distances")
            # 5. cap < 0 and NULL outputs as in the L2 forms
            err(L.fm_wide_set_selfdist(H, qb.handle, None), EINVAL, "NULL")
            err(L.fm_wide_self_dist(H, qb.handle, None), EINVAL, "NULL")
            assert L.fm_wide_self_dist_batch(H, 1, (P * 1)(qb.handle), None) == 0
            qb.has_selfdist = True
            err(L.fm_wide_match_accepted(H, qb.handle, tb.handle, 0.8, -1, p(i32), p(i32), p(f32), p(f64), ctypes.byref(cnt)), EINVAL, "cap < 0")
            err(L.fm_wide_match_accepted_dev(H, qb.handle, tb.handle, 0.8, -1, d_rows.data_ptr(), d_cnt.data_ptr(), None), EINVAL, "cap < 0")
            err(L.fm_wide_match_ratio(H, qb.handle, tb.handle, 0.8, None, p(f32), None, None, ctypes.byref(cnt)), EINVAL, "NULL")
            err(L.fm_wide_match_accepted(H, qb.handle, tb.handle, 0.8, n, None, p(i32), p(f32), p(f64), ctypes.byref(cnt)), EINVAL, "NULL")
            err(L.fm_wide_match_accepted_dev(H, qb.handle, tb.handle, 0.8, n, None, d_cnt.data_ptr(), None), EINVAL, "NULL")
            err(L.fm_collection_wide_match_accepted_each(H, wcol.handle, qb.handle, 0.8, -1, *each_args[2:]), EINVAL, "cap < 0")
            err(L.fm_collection_wide_match_accepted_each(H, wcol.handle, qb.handle, 0.8, n, None, None, None, None, each_args[-1]), EINVAL, "NULL")
            err(L.fm_collection_wide_match_accepted_each_dev(H, wcol.handle, qb.handle, 0.8, n, None, None, None, None), EINVAL, "NULL")
            # empty banks and empty collections are valid
            assert L.fm_wide_self_dist(H, empty.handle, None) == 0
            assert L.fm_wide_set_selfdist(H, empty.handle, None) == 0
            assert L.fm_wide_match_ratio(H, empty.handle, tb.handle, 0.8, None, None, None, None, ctypes.byref(cnt)) == 0 and cnt.value == 0
            assert L.fm_wide_match_accepted(H, qb.handle, empty.handle, *acc_args) == 0 and cnt.value == 0
            with ctx.collection() as ecol:
                assert L.fm_collection_wide_match_accepted_each(H, ecol.handle, qb.handle, *each_args) == 0
                assert L.fm_collection_wide_match_accepted_each(H, ecol.handle, f128.handle, *each_args) == EINVAL     # (the query's kind still counts)
            # the L2-named calls keep refusing a wide bank, with "wide" in the message
            err(L.fm_self_dist(H, qb.handle, p(f64)), EUNSUPPORTED, "wide")
            err(L.fm_match_ratio(H, qb.handle, tb.handle, *ratio_args), EUNSUPPORTED, "wide")
        # the context still answers a wide fm_knn2 and a 128-D fm_self_dist
        got = ctx.knn2(qb, tb)
        want = ref.knn(W, W[:30], 2)
        assert _same(got[0], want[0]) and _same(got[1], want[1])
        sd128 = ctx.self_dist(f128)
        k2 = ref.knn(W[:, :128], W[:, :128], 2)[1][:, 1].astype(np.float64)
        assert _same(sd128, k2)
        assert _same(ctx.wide_self_dist(qb), WF.self_dist(W))
    finally:
        for b in (qb, tb, w200, f128, bq, empty):
            b.close()
        other.close()


# ---- memory ----------------------------------------------------------------------------------------------------------------
def test_cycles_give_the_memory_back():
    c = fastmatch_amd.Context(0)
    rng = np.random.default_rng(5)
    W = rng.standard_normal((700, 256)).astype(np.float32)

    def cycle(k):
        c.set_option("f32_filter", 2 if k % 2 else 0)
        dim = 129 + k % 128
        qb, tb = c.bank(W[: 300 + k % 100, :dim]), c.bank(W[: 600 + k % 100, :dim])
        if k % 3 == 0:
            c.wide_self_dist(qb)
        c.wide_self_dist_batch([qb], want_host=False)
        c.wide_match_accepted(qb, tb, 0.9)
        if k % 10 == 0:
            c.wide_match_ratio(qb, tb, 0.9)
            with c.collection() as col:
                col.add_wide(W[:200, :dim])
                col.add_wide(W[200:450, :dim])
                col.wide_match_accepted_each(qb, 0.9)
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


# ---- Python layers ---------------------------------------------------------------------------------------------------------
def test_matchutil(fctx):
    mode, c = fctx
    Q, T, sd, _, _ = _pair(300, 257, 256)
    want = WF.fast_match(Q, T, 0.8, sd)
    assert len(want[0]) > 0
    opts = {"context": c}
    got = matchutil.wide_fast_match_arrays(Q, T, 0.8, options=opts)
    assert _same_rows(got, want)
    got64 = matchutil.wide_fast_match_arrays(np.asarray(Q, np.float64), np.asarray(T, np.float64), 0.8, options=opts)
    assert _same_rows(got64, want)
    lst = matchutil.wide_fast_match(Q, T, 0.8, options=opts)
    assert [(m.queryIdx, m.trainIdx) for m in lst] == list(zip(want[0].tolist(), want[1].tolist()))
    # a resident query bank that carries self distances of its own is taken at its word
    qb = c.bank(Q)
    try:
        mine = np.full(len(Q), 1e9)
        qb.set_wide_selfdist(mine)
        g = matchutil.wide_fast_match_arrays(qb, T, 0.8, options=opts)
        assert _same_rows(g, WF.fast_match(Q, T, 0.8, mine))
    finally:
        qb.close()
    images = [np.ascontiguousarray(T[:100]), np.ascontiguousarray(T[100:101]), np.ascontiguousarray(T[101:])]
    m = matchutil.BFMatcher(options=opts)
    m.add_wide(images)
    each = m.wideFastMatchEach_arrays(Q, 0.8)
    ref_each = WF.fast_match_each(Q, images, 0.8, sd)
    assert len(each) == 3 and all(_same_rows(g, w) for g, w in zip(each, ref_each))
    lists = m.wideFastMatchEach(Q, 0.8)
    assert [[(d.queryIdx, d.trainIdx, d.imgIdx) for d in l] for l in lists] == \
        [[(int(q), int(t), i) for q, t in zip(w[0], w[1])] for i, w in enumerate(ref_each)]


@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16"])
def test_torchmatch(fctx, dtype):
    import torch
    from fastmatch_amd import torchmatch
    mode, c = fctx
    Q, T, _, _, _ = _pair(300, 257, 256)
    dt = getattr(torch, dtype)
    # integer-free scaling keeps half in range; the reference runs on the widened values
    tq, tt = torch.from_numpy(np.array(Q)).cuda().to(dt), torch.from_numpy(np.array(T)).cuda().to(dt)
    hq, ht = tq.float().cpu().numpy(), tt.float().cpu().numpy()
    sd = WF.self_dist(hq)
    want = WF.fast_match(hq, ht, 0.8, sd)
    qb, tb = torchmatch.bank(tq, context=c), torchmatch.bank(tt, context=c)
    try:
        rows, count = torchmatch.wide_fast_match(qb, tb, 0.8)
        r = rows.cpu().numpy()
        assert int(count.item()) == len(want[0]) == len(r)
        assert _same(r[:, 0], want[0]) and _same(r[:, 1], want[1]) and _same(r[:, 2].view(np.float32), want[2])
        images = [tt[:100], tt[100:101], tt[101:]]
        ref_each = WF.fast_match_each(hq, [ht[:100], ht[100:101], ht[101:]], 0.8, sd)
        with torchmatch.Collection(context=c) as col:
            for im in images:
                col.add_wide(im)
            rows, counts = col.wide_fast_match_each(qb, 0.8)
            r, k = rows.cpu().numpy(), counts.cpu().numpy()
            assert r.shape == (3, 300, 3) and k.tolist() == [len(w[0]) for w in ref_each]
            for i, w in enumerate(ref_each):
                m = len(w[0])
                assert _same(r[i, :m, 0], w[0]) and _same(r[i, :m, 1], w[1]) and _same(r[i, :m, 2].view(np.float32), w[2])
            # a tensor query: its bank and its self distances are made for the call
            rows2, counts2 = col.wide_fast_match_each(tq, 0.8)
            assert torch.equal(counts2, counts) and all(torch.equal(rows2[i, :int(k[i])], rows[i, :int(k[i])]) for i in range(3))
    finally:
        qb.close(); tb.close()
        c.sync()                                                       # (the collection calls only enqueue: nothing stays pending)
    if dtype == "float32":
        rows, count = torchmatch.wide_fast_match(tq, tt, 0.8)          # tensors in, banks made for the call
        assert int(count.item()) == len(want[0]) and _same(rows.cpu().numpy()[:, 1], want[1])
