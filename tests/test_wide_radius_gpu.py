"""GPU: radiusMatch on wide float banks (FM_BANK_F32W, 129 .. 256 values per row) -- fm_wide_radius_match,
fm_wide_radius_match_dev, matchutil.wide_radius_match(_arrays), torchmatch.wide_radius_match.

Every result is compared bit for bit with the reference (tests/wide_radius_ref.py: oracle.bf_knn with k = all rows and the
float32 fma chain, cut at dist < r_i): the offsets, the train indices, the distances as uint32 bit patterns.  The planted
threshold pairs (tests/f16_margin_ref.py) sit at 0.78 of the sweep's margin: a sweep that loses fp16 products, takes a smaller
constant or the wrong norm bound drops them."""
import ctypes

import numpy as np
import pytest

import fastmatch_amd
from fastmatch_amd import _ffi, matchutil
import f16_margin_ref as F
import wide_radius_ref as WR
import wide_ref

pytestmark = pytest.mark.gpu

P = ctypes.c_void_p
EINVAL, EUNSUPPORTED = -1, -4


def _ptr(a):
    return a.ctypes.data_as(P)


def _check(ctx, qb, tb, ref, r, what):
    WR.same_pair(ctx.wide_radius_match(qb, tb, r), ref.cut(r), what)


def _swept(ctx, l0, calls):
    """fm_f32_filter_stats counts one launch per C call that ran the fp16 sweep; a Python call is a counts call and, when
    there are entries, a fill call."""
    return calls <= ctx.f32_filter_stats()[0] - l0 <= 2 * calls


# ---- every K-step count, every shape ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", WR.DIMS)
def test_every_dim_and_shape(ctx, dim):
    shapes = WR.SHAPES if dim in (129, 256) else WR.SMALL
    for nq, nt in shapes:
        Q, T = wide_ref.clustered(max(nq, 1), max(nt, 2), dim, 100 + dim)
        Q, T = np.ascontiguousarray(Q[:nq]), np.ascontiguousarray(T[:nt])
        ref = WR.Ref(Q, [T])
        qb, tb = ctx.bank(Q), ctx.bank(T)
        try:
            assert qb.kind == tb.kind == _ffi.FM_BANK_F32W
            if nq == 0 or nt == 0:
                for r in (np.inf, np.full(nq, np.inf, np.float32)):
                    off, idx, dist = ctx.wide_radius_match(qb, tb, r)
                    assert off.shape == (nq + 1,) and not off.any() and idx.size == dist.size == 0
                continue
            l0 = ctx.f32_filter_stats()[0]
            r = ref.kth(min(4, nt - 1))
            _check(ctx, qb, tb, ref, r, (dim, nq, nt, "scalar"))
            _check(ctx, qb, tb, ref, WR.mixed_radii(ref, dim), (dim, nq, nt, "per row"))
            _check(ctx, qb, tb, ref, np.inf, (dim, nq, nt, "inf"))
            assert np.array_equal(np.diff(ctx.wide_radius_match(qb, tb, np.inf)[0]), np.full(nq, nt))
            assert _swept(ctx, l0, 4)                              # the fp16 sweep ran in every one of the four calls
            for r in (0.0, -1.0, np.nan, -np.inf):
                off, idx, dist = ctx.wide_radius_match(qb, tb, np.float32(r))
                assert not off.any() and idx.size == dist.size == 0
        finally:
            qb.close()
            tb.close()


# ---- the data regimes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [129, 256])
@pytest.mark.parametrize("regime", ["clustered", "gaussian", "spread", "integers", "copies", "nonfinite"])
def test_regimes(ctx, regime, dim):
    nq, nt = 300, 1100          # a partial last 64-row stage (1088 .. 1099), three workgroups of query rows, two splits
    Q, T = wide_ref.REGIMES[regime](nq, nt, dim, 7)
    ref = WR.Ref(Q, [T])
    qb, tb = ctx.bank(Q), ctx.bank(T)
    try:
        rows = WR.mixed_radii(ref, 2)
        even = np.arange(0, nq, 2)
        assert np.isnan(rows).any() and np.isinf(rows).any() and (rows == 0).any() and (rows < 0).any()
        l0 = ctx.f32_filter_stats()[0]
        for r, what in ((ref.kth(8), "scalar"), (rows, "per row"), (np.inf, "inf")):
            _check(ctx, qb, tb, ref, r, (regime, dim, what))
        grown = ctx.f32_filter_stats()[0] - l0
        if regime == "nonfinite":
            assert grown == 0                                       # a value that is not finite: the all-pairs path
            off = ref.cut(np.inf)[0]
            assert off[nq // 2 + 1] == off[nq // 2] and np.diff(off).max() == nt - 2    # the NaN row lists nothing; nobody lists a NaN or inf row
        else:
            assert 3 <= grown <= 6
        # a radius EXACTLY equal to one of the row's distances excludes that entry, the float32 after it includes it
        off = ref.cut(rows)[0]
        up = np.where(np.isfinite(rows) & (rows > 0) & (rows < 1e38), np.nextafter(rows, np.float32(np.inf)), rows).astype(np.float32)
        off_up = ref.cut(up)[0]
        assert (np.diff(off_up)[even] > np.diff(off)[even]).sum() > nq // 4
        _check(ctx, qb, tb, ref, up, (regime, dim, "the float32 after"))
        # one row lists every train row with a finite distance: the long-segment sort tier (> 2048 keys needs more rows: below)
        assert np.diff(off)[3] >= nt - 2
    finally:
        qb.close()
        tb.close()


def test_a_list_beyond_2048_keys(ctx):
    """The third sort tier (rocPRIM's segmented sort): rows whose lists hold more than 2048 entries, next to short ones."""
    dim = 224
    Q, T = wide_ref.gaussian(5, 2300, dim, 11)
    ref = WR.Ref(Q, [T])
    qb, tb = ctx.bank(Q), ctx.bank(T)
    try:
        r = np.array([np.inf, ref.dist[1, 20], 3.0e38, ref.dist[3, 2100], 0.0], np.float32)
        want = ref.cut(r)
        assert np.diff(want[0]).tolist()[0] == 2300 and np.diff(want[0])[2] == 2300 and 2048 < np.diff(want[0])[3] < 2300
        _check(ctx, qb, tb, ref, r, "long lists")
        _check(ctx, qb, tb, ref, np.inf, "every list long")
    finally:
        qb.close()
        tb.close()


# ---- planted pairs on the threshold ------------------------------------------------------------------------------------------
def _planted_rows_present(p, got, r):
    off, idx, dist = got
    for f in p.fams:
        row = idx[off[f["q"]]:off[f["q"] + 1]]
        if f["kind"] == "hit":
            assert f["t"] in row, ("a planted hit is missing", f)
        else:
            assert f["t"] not in row, ("a mirror pair was listed", f)


@pytest.mark.parametrize("dim", [129, 256])
def test_planted_threshold_pairs(ctx, dim):
    p = F.radius_set(dim)
    r, fractions = F.check_threshold(p, eps=F.EPS_K14, floor=0.75)
    ref = WR.Ref(p.Q, [p.T])
    want = ref.cut(r)
    assert want[0][-1] == 9                                         # the nine planted hits and nothing else
    qb, tb = ctx.bank(np.array(p.Q)), ctx.bank(np.array(p.T))
    try:
        l0 = ctx.f32_filter_stats()[0]
        got = ctx.wide_radius_match(qb, tb, r)
        assert _swept(ctx, l0, 1)                                   # ... through the fp16 sweep
        _planted_rows_present(p, got, r)
        WR.same_pair(got, want, ("planted", dim))
        rows = np.full(len(p.Q), r, np.float32)
        WR.same_pair(ctx.wide_radius_match(qb, tb, rows), want, ("planted, per row", dim))
        # a query bank whose scale exponent differs by 3: one more query row of magnitude 8 * 1.25
        rng = np.random.default_rng(5)
        Q8 = np.concatenate([p.Q, (10.0 * rng.choice([-1.0, 1.0], (1, dim))).astype(np.float32)])
        assert F.kscale(Q8) == F.kscale(p.T) - 3
        ref8 = WR.Ref(Q8, [p.T])
        q8 = ctx.bank(Q8)
        try:
            l0 = ctx.f32_filter_stats()[0]
            got8 = ctx.wide_radius_match(q8, tb, r)
            assert _swept(ctx, l0, 1)
            _planted_rows_present(p, got8, r)
            WR.same_pair(got8, ref8.cut(r), ("planted, scales 3 apart", dim))
            assert got8[0][-1] == 9
        finally:
            q8.close()
    finally:
        qb.close()
        tb.close()


def test_scales_more_than_8_apart_take_the_all_pairs_path(ctx):
    dim = 193
    Q, T = wide_ref.clustered(129, 127, dim, 21)
    dk = F.kscale(Q) - F.kscale(T)                                  # (0 or +-1: the two largest magnitudes may lie in neighbouring binades)
    Qs = np.ldexp(Q, -(10 - dk)).astype(np.float32)                 # exact: the query bank's exponent is 10 above the train bank's
    assert F.kscale(Qs) - F.kscale(T) == 10
    ref = WR.Ref(Qs, [T])
    qb, tb = ctx.bank(Qs), ctx.bank(T)
    try:
        l0 = ctx.f32_filter_stats()[0]
        for r in (ref.kth(5), WR.mixed_radii(ref, 3), np.inf):
            _check(ctx, qb, tb, ref, r, "scales 10 apart")
        assert ctx.f32_filter_stats()[0] == l0                      # no fp16 sweep
        # the other way round, and 8 apart (still swept)
        ref_r = WR.Ref(T, [Qs])
        _check(ctx, tb, qb, ref_r, ref_r.kth(5), "scales -10 apart")
        assert ctx.f32_filter_stats()[0] == l0
        Q8 = np.ldexp(Q, -(8 - dk)).astype(np.float32)
        assert F.kscale(Q8) - F.kscale(T) == 8
        q8 = ctx.bank(Q8)
        try:
            ref8 = WR.Ref(Q8, [T])
            _check(ctx, q8, tb, ref8, ref8.kth(5), "scales 8 apart")
            _check(ctx, q8, tb, ref8, WR.mixed_radii(ref8, 4), "scales 8 apart, per row")
            assert _swept(ctx, l0, 2)
        finally:
            q8.close()
    finally:
        qb.close()
        tb.close()


# ---- cap, chunks, options -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def std(ctx):
    """(query bank, train bank, reference, Q, T) of the 300 x 1100 clustered set at 161 values (6 K steps)."""
    Q, T = wide_ref.clustered(300, 1100, 161, 31)
    qb, tb = ctx.bank(Q), ctx.bank(T)
    yield qb, tb, WR.Ref(Q, [T]), Q, T
    qb.close()
    tb.close()


def _raw(ctx, qb, tb, r, cap, size, with_lists=True, fn="fm_wide_radius_match"):
    """The C call with sentinel-filled arrays of `size` entries: (rc, offsets, idx, dist, n_total)."""
    off = np.full((qb.n if qb is not None else 0) + 1, -7, np.int64)
    idx = np.full(size, -78, np.int32)
    dist = np.full(size, -79.0, np.float32)
    tot = ctypes.c_int64(-1)
    rows = None if np.ndim(r) == 0 else np.ascontiguousarray(r, np.float32)
    rc = getattr(ctx.lib, fn)(ctx.handle, qb.handle if qb is not None else None, tb.handle if tb is not None else None,
                              _ptr(rows) if rows is not None else None, float(np.float32(r)) if rows is None else 0.0, cap,
                              _ptr(off), _ptr(idx) if with_lists else None, _ptr(dist) if with_lists else None, ctypes.byref(tot))
    return rc, off, idx, dist, tot.value


def test_cap_counts_only_and_the_prefix_of_whole_rows(ctx, std):
    qb, tb, ref, _, _ = std
    r = WR.mixed_radii(ref, 4)
    woff, _, _, wdist, widx = ref.cut(r)
    total = int(woff[-1])
    rc, off, _, _, tot = _raw(ctx, qb, tb, r, 0, 1, with_lists=False)           # counts only, NULL lists
    assert rc == 0 and np.array_equal(off, woff) and tot == total
    k = ref.nq // 2 + int(np.argmax(np.diff(woff)[ref.nq // 2:] > 1))    # a row of at least two entries, past the middle
    assert 0 < woff[k] < total and woff[k + 1] - woff[k] > 1
    old = ctx.get_option("radius_ws_bytes")
    try:
        for ws in (old, 65536):                                                  # 65536: 2730 candidates (24 B each) per chunk
            ctx.set_option("radius_ws_bytes", ws)
            for cap in (total - 1, int(woff[k]) + 1, int(woff[k]), total):       # woff[k] + 1 cuts inside row k
                rc, off, idx, dist, tot = _raw(ctx, qb, tb, r, cap, total + 5)
                assert rc == 0 and np.array_equal(off, woff) and tot == total
                m = int(woff[np.searchsorted(woff, cap, side="right") - 1])      # the longest prefix of whole rows within cap
                assert m <= cap and (cap < total) == (m < total)
                assert np.array_equal(idx[:m], widx[:m]) and np.array_equal(WR.bits(dist[:m]), WR.bits(wdist[:m]))
                assert np.all(idx[m:] == -78) and np.all(dist[m:] == -79.0), "written beyond the prefix"
    finally:
        ctx.set_option("radius_ws_bytes", old)


def test_many_chunks_and_options_give_the_same_bits(ctx, std):
    qb, tb, ref, _, _ = std
    radii = (ref.kth(4), WR.mixed_radii(ref, 3), np.inf)
    assert ref.cut(np.inf)[0][-1] == 300 * 1100 > 100 * (65536 // 24)
    saved = {k: ctx.get_option(k) for k in ("radius_ws_bytes", "f32_filter", "f32_nsplit", "nsplit")}
    try:
        for opts in ({"radius_ws_bytes": 65536}, {"f32_filter": 0}, {"f32_filter": 2, "f32_nsplit": 3}, {"nsplit": 5, "radius_ws_bytes": 1 << 20}):
            for k, v in opts.items():
                ctx.set_option(k, v)
            l0 = ctx.f32_filter_stats()[0]
            for r in radii:
                _check(ctx, qb, tb, ref, r, opts)
            assert _swept(ctx, l0, 3)                             # no option switches the sweep
            for k, v in saved.items():
                ctx.set_option(k, v)
    finally:
        for k, v in saved.items():
            ctx.set_option(k, v)


def test_accounted_in_the_stats(ctx, std):
    qb, tb, ref, _, _ = std
    before = ctx.stats()
    assert _raw(ctx, qb, tb, np.float32(ref.kth(2)), 0, 1, with_lists=False)[0] == 0
    after = ctx.stats()
    assert after["calls"] - before["calls"] == 1 and after["pairs"] - before["pairs"] == 300 * 1100


# ---- errors, in the header's order ------------------------------------------------------------------------------------------
def test_refusals_with_their_codes_leave_the_context_working(ctx, std):
    qb, tb, ref, Q, T = std
    rng = np.random.default_rng(37)

    def still_answers():
        _check(ctx, qb, tb, ref, ref.kth(2), "after a refusal")

    def refused(call, code, *words):
        with pytest.raises(fastmatch_amd.FastMatchHipError) as e:
            call()
        assert e.value.code == code, e.value
        for w in words:
            assert w in str(e.value), (w, str(e.value))
        still_answers()

    # 1. NULL handles
    assert _raw(ctx, None, tb, 1.0, 0, 1, fn="fm_wide_radius_match")[0] == EINVAL
    assert _raw(ctx, qb, None, 1.0, 0, 1)[0] == EINVAL
    still_answers()
    # 2. a bank that is not wide, even an empty one; the message names the call that serves it
    f32 = ctx.bank(np.ascontiguousarray(Q[:, :128]), float_route=True)
    f32_0 = ctx.bank(np.ascontiguousarray(Q[:0, :128]), float_route=True)
    binb = ctx.bank_binary(rng.integers(0, 256, (9, 32), dtype=np.uint8))
    narrow = ctx.bank(np.ones((4, 200), np.float32))               # wide banks of another dim (std: 161)
    narrow0 = ctx.bank(np.zeros((0, 200), np.float32))
    try:
        assert narrow.kind == narrow0.kind == _ffi.FM_BANK_F32W
        refused(lambda: ctx.wide_radius_match(f32, tb, 1.0), EINVAL, "fm_radius_match is the L2 call")
        refused(lambda: ctx.wide_radius_match(qb, f32, 1.0), EINVAL, "fm_radius_match is the L2 call")
        refused(lambda: ctx.wide_radius_match(f32_0, tb, 1.0), EINVAL, "fm_radius_match")
        refused(lambda: ctx.wide_radius_match(f32, f32, 1.0), EINVAL, "wide")
        refused(lambda: ctx.wide_radius_match(binb, tb, 1.0), EINVAL, "fm_hamming_radius_match")
        refused(lambda: ctx.wide_radius_match(binb, binb, 40.0), EINVAL, "fm_hamming_radius_match")
        # (the kind comes before the dims: a float32 bank of another width is refused for its kind)
        # 3. dims that differ, also for an empty bank
        refused(lambda: ctx.wide_radius_match(narrow, tb, 1.0), EINVAL, "dim mismatch")
        refused(lambda: ctx.wide_radius_match(qb, narrow0, 1.0), EINVAL, "dim mismatch")
        # ... and before cap: both wrong gives the dim message
        with pytest.raises(fastmatch_amd.FastMatchHipError) as e:
            ctx._check(_raw(ctx, narrow, tb, 1.0, -1, 1)[0])
        assert "dim mismatch" in str(e.value)
        # the L2-named and the Hamming calls keep refusing wide banks
        refused(lambda: ctx.radius_match(qb, tb, 1.0), EUNSUPPORTED, "wide")
        refused(lambda: ctx.hamming_radius_match(qb, tb, 1.0), EINVAL)
    finally:
        for b in (f32, f32_0, binb, narrow, narrow0):
            b.close()
    # 4. cap < 0, NULL offsets, NULL lists with cap > 0
    assert _raw(ctx, qb, tb, np.inf, -1, 4)[0] == EINVAL
    still_answers()
    assert _raw(ctx, qb, tb, np.inf, 8, 8, with_lists=False)[0] == EINVAL
    still_answers()
    tot = ctypes.c_int64(-1)
    assert ctx.lib.fm_wide_radius_match(ctx.handle, qb.handle, tb.handle, None, 1.0, 0, None, None, None, ctypes.byref(tot)) == EINVAL
    still_answers()
    # n_total may be NULL
    off = np.full(qb.n + 1, -7, np.int64)
    assert ctx.lib.fm_wide_radius_match(ctx.handle, qb.handle, tb.handle, None, float(ref.kth(2)), 0, _ptr(off), None, None, None) == 0
    assert np.array_equal(off, ref.cut(ref.kth(2))[0])


# ---- device forms -----------------------------------------------------------------------------------------------------------
def _torch():
    import torch
    return torch


def _dev(a):
    return _torch().from_numpy(np.array(a, order="C")).cuda()


def _dev_call(ctx, qb, tb, r, cap, size=None, stream="current", lists=True, want_total=True):
    torch = _torch()
    size = cap if size is None else size
    off = torch.full((qb.n + 1,), -7, dtype=torch.int64, device="cuda")
    idx = torch.full((size,), -78, dtype=torch.int32, device="cuda")
    dist = torch.full((size,), -79.0, dtype=torch.float32, device="cuda")
    if isinstance(r, torch.Tensor):
        rt, r_all = r, 0.0
    elif np.ndim(r) == 0:
        rt, r_all = None, float(np.float32(r))
    else:
        rt, r_all = _dev(np.asarray(r, np.float32)), 0.0
    s = torch.cuda.current_stream().cuda_stream if stream == "current" else stream
    if stream is None:
        torch.cuda.synchronize()
    p = (lambda t: t.data_ptr()) if lists and size else (lambda t: 0)
    n = ctx.wide_radius_match_dev(qb, tb, rt.data_ptr() if rt is not None else 0, r_all, cap, off.data_ptr(), p(idx), p(dist),
                                  want_total=want_total, consumer_stream=s)
    if stream is None:
        ctx.sync()
    return n, off.cpu().numpy(), idx.cpu().numpy(), dist.cpu().numpy()


def test_device_form_equals_the_reference_and_the_host_form(ctx, std):
    torch = _torch()
    qb, tb, ref, _, _ = std
    rows = WR.mixed_radii(ref, 6)
    for r in (ref.kth(4), rows, np.inf):
        want = ref.cut(r)
        n0, off0, _, _ = _dev_call(ctx, qb, tb, r, 0, lists=False)
        assert n0 == want[0][-1] and np.array_equal(off0, want[0])
        for stream in ("current", None):
            n, off, idx, dist = _dev_call(ctx, qb, tb, r, n0, stream=stream)
            assert n == n0
            WR.same_pair((off, idx, dist), want, ("device form", stream))
        host = ctx.wide_radius_match(qb, tb, r)
        assert np.array_equal(host[0], off) and np.array_equal(host[1], idx) and np.array_equal(WR.bits(host[2]), WR.bits(dist))
    # device radii read in place, from a kernel on the current stream without a synchronize; n_total NULL
    d_rows = _dev(rows)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        rad = d_rows * 1.0 + 0.0
        want = ref.cut(rows)
        total = int(want[0][-1])
        n, off, idx, dist = _dev_call(ctx, qb, tb, rad, total, want_total=False)
        assert n is None
        WR.same_pair((off, idx, dist), want, "device radii, n_total NULL")
    # a cap that cuts inside a row, with several chunks: the prefix of whole rows, sentinels beyond it
    old = ctx.get_option("radius_ws_bytes")
    try:
        ctx.set_option("radius_ws_bytes", 65536)
        k = ref.nq // 2 + int(np.argmax(np.diff(want[0])[ref.nq // 2:] > 1))
        cap = int(want[0][k]) + 1
        n, off, idx, dist = _dev_call(ctx, qb, tb, rows, cap, size=total + 3)
        m = int(want[0][k])
        assert want[0][k + 1] > cap
        assert n == total and np.array_equal(off, want[0]) and 0 < m < cap
        assert np.array_equal(idx[:m], want[4][:m]) and np.array_equal(WR.bits(dist[:m]), WR.bits(want[3][:m]))
        assert np.all(idx[m:] == -78) and np.all(dist[m:] == -79.0), "written beyond the prefix"
    finally:
        ctx.set_option("radius_ws_bytes", old)
    # degenerate radii still write the offsets; stats are not touched by the device form
    before = ctx.stats()
    for r in (0.0, np.nan, -2.0):
        n, off, _, _ = _dev_call(ctx, qb, tb, np.float32(r), 0, lists=False)
        assert n == 0 and not off.any()
    assert _dev_call(ctx, qb, tb, ref.kth(2), 0, lists=False)[0] == ref.cut(ref.kth(2))[0][-1]
    assert ctx.stats()["calls"] == before["calls"] and ctx.stats()["pairs"] == before["pairs"]


def test_device_form_pointer_checks(ctx, std):
    torch = _torch()
    qb, tb, ref, Q, _ = std
    nq = qb.n
    h_r, h_off, h_idx = np.ones(nq, np.float32), np.zeros(nq + 1, np.int64), np.zeros(64, np.int32)
    d_r = _dev(np.full(nq, ref.kth(2), np.float32))
    d_off = torch.zeros(nq + 1, dtype=torch.int64, device="cuda")
    d_idx = torch.zeros(64, dtype=torch.int32, device="cuda")
    d_dist = torch.zeros(64, dtype=torch.float32, device="cuda")
    good = dict(r=d_r.data_ptr(), off=d_off.data_ptr(), idx=d_idx.data_ptr())
    for bad in (dict(r=h_r.ctypes.data), dict(off=h_off.ctypes.data), dict(idx=h_idx.ctypes.data)):
        a = dict(good, **bad)
        with pytest.raises(fastmatch_amd.FastMatchHipError) as e:
            ctx.wide_radius_match_dev(qb, tb, a["r"], 0.0, 64, a["off"], a["idx"], d_dist.data_ptr(), consumer_stream=None)
        assert e.value.code == EINVAL and "device memory" in str(e.value)
    # the host forms' errors come first: a bank of another kind with a host pointer is refused for its kind
    f32 = ctx.bank(np.ascontiguousarray(Q[:, :128]), float_route=True)
    try:
        with pytest.raises(fastmatch_amd.FastMatchHipError) as e:
            ctx.wide_radius_match_dev(f32, tb, h_r.ctypes.data, 0.0, 64, h_off.ctypes.data, 0, 0, consumer_stream=None)
        assert e.value.code == EINVAL and "fm_radius_match is the L2 call" in str(e.value)
    finally:
        f32.close()
    with pytest.raises(fastmatch_amd.FastMatchHipError) as e:
        ctx.wide_radius_match_dev(qb, tb, d_r.data_ptr(), 0.0, 8, d_off.data_ptr(), 0, 0, consumer_stream=None)
    assert e.value.code == EINVAL
    want = ref.cut(np.float32(ref.kth(2)))[0]
    assert ctx.wide_radius_match_dev(qb, tb, d_r.data_ptr(), 0.0, 0, d_off.data_ptr(), 0, 0, consumer_stream=None) == want[-1]
    ctx.sync()
    assert np.array_equal(d_off.cpu().numpy(), want)


# ---- matchutil and torchmatch -------------------------------------------------------------------------------------------------
def test_through_matchutil_and_torchmatch(ctx, std):
    torch = _torch()
    from fastmatch_amd import torchmatch
    qb, tb, ref, Q, T = std
    r = ref.kth(4)
    want = ref.cut(r)
    rows = WR.mixed_radii(ref, 8)
    opts = {"context": ctx}
    WR.same_pair(matchutil.wide_radius_match_arrays(Q, T, r, options=opts), want, "matchutil arrays")
    WR.same_pair(matchutil.wide_radius_match_arrays(qb, T.astype(np.float64), rows, options=opts), ref.cut(rows), "matchutil bank + float64")
    lists = matchutil.wide_radius_match(Q, tb, r, options=opts)
    assert len(lists) == 300 and [len(x) for x in lists] == np.diff(want[0]).tolist()
    flat = [m for x in lists for m in x]
    assert [m.trainIdx for m in flat] == want[4].tolist() and [m.queryIdx for m in flat] == np.repeat(np.arange(300), np.diff(want[0])).tolist()
    assert np.array_equal(WR.bits(np.array([m.distance for m in flat], np.float32)), WR.bits(want[3]))
    # torchmatch: float32 tensors and banks, a scalar and a device radius tensor
    for q, t, rr, w in ((_dev(Q), _dev(T), float(r), want), (qb, _dev(T), _dev(rows), ref.cut(rows)), (_dev(Q), tb, np.float32(np.inf), ref.cut(np.inf))):
        off, idx, dist = torchmatch.wide_radius_match(q, t, rr)
        assert off.is_cuda and idx.is_cuda and dist.is_cuda
        assert (off.dtype, idx.dtype, dist.dtype) == (torch.int64, torch.int32, torch.float32)
        WR.same_pair((off.cpu().numpy(), idx.cpu().numpy(), dist.cpu().numpy()), w, "torchmatch")
    # one float16 and one bfloat16 tensor pair: the banks of their widened values
    rng = np.random.default_rng(43)
    for dt in (torch.float16, torch.bfloat16):
        q_h = torch.from_numpy(rng.standard_normal((90, 200)).astype(np.float32)).to(dt)
        t_h = torch.from_numpy(rng.standard_normal((260, 200)).astype(np.float32)).to(dt)
        ref_h = WR.Ref(q_h.float().numpy(), [t_h.float().numpy()])
        for rr, want_r in ((float(ref_h.kth(3)), ref_h.kth(3)), (_dev(WR.mixed_radii(ref_h, 9)), WR.mixed_radii(ref_h, 9))):
            off, idx, dist = torchmatch.wide_radius_match(q_h.cuda(), t_h.cuda(), rr)
            WR.same_pair((off.cpu().numpy(), idx.cpu().numpy(), dist.cpu().numpy()), ref_h.cut(want_r), ("torchmatch", dt))
