"""GPU: radiusMatch (K10, fm_radius_match) -- cv2.BFMatcher(NORM_L2).radiusMatch with compactResult False.

Row i's list holds every train row with dist(i, j) < r_i (strict, float32), ascending by (distance bits, train index);
dist is the value fm_knn2 returns.  The reference lists come from the oracle's k-NN (oracle.bf_knn, k_cap columns) cut at
r, with the k_cap-th column checked to be >= r so that the cut list is complete."""
import ctypes

import numpy as np
import pytest

import fastmatch_amd
import oracle
from fastmatch_amd import matchutil, synth, _ffi
from kat import far_banks, row_with_sumsq

pytestmark = pytest.mark.gpu


def _radii(r, nq):
    return np.broadcast_to(np.asarray(r, dtype=np.float32), (nq,)).copy()


def _ref(Q, T, r, k_cap=None):
    """Reference lists [(idx, dist)] per query row from the oracle's k-NN lists."""
    nq, nt = len(Q), len(T)
    rr = _radii(r, nq)
    if nq == 0 or nt == 0:
        return [(np.zeros(0, np.int32), np.zeros(0, np.float32)) for _ in range(nq)]
    k = nt if k_cap is None else min(k_cap, nt)
    idx, dist = oracle.bf_knn(Q, T, k, order=1)
    if k < nt:
        live = rr > 0
        assert np.all(dist[live, -1] >= rr[live]), "k_cap too small: a reference list may be cut short"
    out = []
    for i in range(nq):
        m = dist[i] < rr[i]
        out.append((idx[i][m], dist[i][m]))
    return out


def _check(res, ref):
    off, idx, dist = res
    assert off.dtype == np.int64 and off.shape == (len(ref) + 1,) and off[0] == 0
    assert off[-1] == idx.shape[0] == dist.shape[0]
    for i, (ri, rd) in enumerate(ref):
        a, b = off[i], off[i + 1]
        assert np.array_equal(idx[a:b], ri), "row %d: %s != %s" % (i, idx[a:b][:10], ri[:10])
        assert np.array_equal(dist[a:b].view(np.uint32), rd.astype(np.float32).view(np.uint32)), "row %d distances" % i


def _both(ctx, Q, T, r, k_cap=None):
    qb, tb = ctx.bank(Q), ctx.bank(T)
    try:
        _check(ctx.radius_match(qb, tb, r), _ref(Q, T, r, k_cap))
    finally:
        qb.close()
        tb.close()


def _floaty(U, rng):
    """Non-integer float32 rows (RootSIFT-like values)."""
    return (U.astype(np.float32) / 512.0 + rng.random(U.shape, dtype=np.float32) * 1e-3).astype(np.float32)


@pytest.mark.parametrize("route", ["i8", "f32"])
def test_planted_pairs_scalar_and_per_row_radius(ctx, route):
    rng = np.random.default_rng(3)
    Q, T, _ = synth.planted_pair(300, 700, seed=11)
    if route == "f32":
        Q, T = _floaty(Q, rng), _floaty(T, rng)
        r, rows = np.float32(0.75), rng.uniform(0.2, 0.85, 300).astype(np.float32)
    else:
        r, rows = np.float32(380.0), rng.uniform(100.0, 420.0, 300).astype(np.float32)
    _both(ctx, Q, T, r)
    _both(ctx, Q, T, rows)


@pytest.mark.parametrize("route", ["i8", "f32"])
def test_duplicate_train_rows_tie_in_ascending_index(ctx, route):
    rng = np.random.default_rng(5)
    base = synth.synth_sift(40, rng)
    T = base[rng.permutation(np.repeat(np.arange(40), 5))]
    Q = np.concatenate([base[:20], synth.synth_sift(10, rng)])
    if route == "f32":
        Q, T = Q.astype(np.float32) / 7.0, T.astype(np.float32) / 7.0
        r = np.float32(60.0)
    else:
        r = np.float32(420.0)
    _both(ctx, Q, T, r)


def test_far_banks_in_the_float32_root_tie_range(ctx):
    rng = np.random.default_rng(7)
    Q, T = far_banks(70, 300, rng)
    idx, dist = oracle.bf_knn(Q, T, 300)
    for r in (np.median(dist), dist[0, 3], dist[5, 40], np.nextafter(dist[1, 10], np.float32(np.inf))):
        _both(ctx, Q, T, np.float32(r))
    _both(ctx, Q, T, dist[np.arange(70), rng.integers(0, 300, 70)].astype(np.float32))


@pytest.mark.parametrize("route", ["i8", "f32"])
@pytest.mark.parametrize("nq,nt,dim", [(1, 1, 128), (63, 64, 64), (64, 65, 128), (65, 127, 32), (127, 128, 100),
                                       (128, 129, 128), (129, 63, 17), (300, 257, 128)])
def test_sizes(ctx, route, nq, nt, dim):
    rng = np.random.default_rng(nq * 1000 + nt)
    Q = synth.synth_sift(nq, rng, dim)
    T = synth.synth_sift(nt, rng, dim)
    if route == "f32":
        Q, T = _floaty(Q, rng), _floaty(T, rng)
        r = np.float32(0.9 * np.sqrt(dim / 128.0))
    else:
        r = np.float32(430.0 * np.sqrt(dim / 128.0))
    _both(ctx, Q, T, r)


@pytest.mark.parametrize("route", ["i8", "f32"])
def test_empty_banks_and_special_radii(ctx, route):
    rng = np.random.default_rng(9)
    Q = synth.synth_sift(50, rng)
    T = synth.synth_sift(90, rng)
    if route == "f32":
        Q, T = _floaty(Q, rng), _floaty(T, rng)
    for r in (0.0, -1.0, np.nan, np.inf, -np.inf):
        _both(ctx, Q, T, np.float32(r))
    rows = rng.choice(np.array([0.0, -2.0, np.nan, np.inf, 400.0 if route == "i8" else 0.8], np.float32), 50)
    _both(ctx, Q, T, rows)
    for q, t in ((Q[:0], T), (Q, T[:0]), (Q[:0], T[:0])):
        off, idx, dist = matchutil.bf_radius_match_arrays(q, t, np.inf, {"context": ctx})
        assert off.shape == (len(q) + 1,) and not off.any() and idx.shape == (0,) and dist.shape == (0,)


def test_integer_boundary_rows_at_the_limit(ctx):
    """Train rows at d2 = D - 1, D, D + 1 (and D + 2) around each radius's limit, below and inside the tie range: a
    row at dist == r is out."""
    def f32root(n):
        return np.sqrt(np.float32(n))
    targets = [1000, 65537, 300001, 4197203, 5000000, 6502051, 7500001]
    rows, d2s = [], []
    for n in targets:
        for dlt in (-1, 0, 1, 2):
            rows.append(row_with_sumsq(n + dlt))
            d2s.append(n + dlt)
    T = np.stack(rows)
    Q = np.zeros((2 * len(targets), 128), dtype=np.uint8)
    radii = np.array([f32root(n) for n in targets] + [np.nextafter(f32root(n), np.float32(0)) for n in targets], np.float32)
    off, idx, dist = ctx.radius_match(ctx.bank(Q), ctx.bank(T), radii)
    d2s = np.array(d2s)
    dd = f32root(d2s.astype(np.float32))
    for i, r in enumerate(radii):
        want = np.nonzero(dd < r)[0]
        want = want[np.lexsort((want, dd[want].view(np.uint32)))]
        assert np.array_equal(idx[off[i]:off[i + 1]], want), "row %d (r = %r)" % (i, r)
        assert not np.any(dd[idx[off[i]:off[i + 1]]] >= r)


def test_float32_boundary_at_realized_distances(ctx):
    """r = exact distances the float32 chain realises: the candidates sit inside the fp16 margin, the rescore decides."""
    rng = np.random.default_rng(13)
    Q, T, _ = synth.planted_pair(200, 500, seed=17)
    Q, T = _floaty(Q, rng), _floaty(T, rng)
    idx, dist = oracle.bf_knn(Q, T, 64, order=1)
    cols = rng.integers(0, 40, 200)
    r = dist[np.arange(200), cols]
    _both(ctx, Q, T, r, k_cap=64)
    _both(ctx, Q, T, np.float32(np.median(dist[:, 5])), k_cap=64)


@pytest.mark.parametrize("route", ["i8", "f32"])
def test_consistent_with_knn8_on_a_large_pair(ctx, route):
    """Every list of <= 8 entries equals the prefix of fm_knn(k = 8) below r, bit for bit; longer lists start with
    fm_knn's 8 entries."""
    rng = np.random.default_rng(21)
    Q, T, _ = synth.planted_pair(20000, 100000, seed=23)
    if route == "f32":
        Q, T = _floaty(Q, rng), _floaty(T, rng)
    qb, tb = ctx.bank(Q), ctx.bank(T)
    try:
        kidx, kdist = ctx.knn(qb, tb, 8)
        r = np.float32(np.median(kdist[:, 2]))
        off, idx, dist = ctx.radius_match(qb, tb, r)
    finally:
        qb.close()
        tb.close()
    n = np.diff(off)
    assert n.sum() > 20000
    m = kdist < r
    short = n <= 8
    assert np.array_equal(n[short], m[short].sum(1))
    pos = off[:-1, None] + np.arange(8)[None, :]
    sel = m & short[:, None]
    assert np.array_equal(idx[pos[sel]], kidx[sel])
    assert np.array_equal(dist[pos[sel]].view(np.uint32), kdist[sel].view(np.uint32))
    long_ = ~short
    if long_.any():
        assert np.array_equal(idx[pos[long_]], kidx[long_])


def _call(ctx, qb, tb, r, cap, offsets, idx, dist):
    tot = ctypes.c_int64(-1)
    ctx._check(ctx.lib.fm_radius_match(ctx.handle, qb.handle, tb.handle, None, float(r), int(cap), offsets.ctypes.data,
                                       idx.ctypes.data if idx is not None else None,
                                       dist.ctypes.data if dist is not None else None, ctypes.byref(tot)))
    return tot.value


@pytest.mark.parametrize("route", ["i8", "f32"])
def test_cap_contract(ctx, route):
    rng = np.random.default_rng(31)
    Q = synth.synth_sift(400, rng)
    T = synth.synth_sift(900, rng)
    if route == "f32":
        Q, T = _floaty(Q, rng), _floaty(T, rng)
    r = float(np.median(oracle.bf_knn(Q, T, 16, order=1)[1][:, 10]))       # ~10 entries per row
    qb, tb = ctx.bank(Q), ctx.bank(T)
    try:
        full = ctx.radius_match(qb, tb, r)
        n = int(full[0][-1])
        assert n > 400
        offs = np.full(401, -7, np.int64)
        assert _call(ctx, qb, tb, r, 0, offs, None, None) == n            # counts only
        assert np.array_equal(offs, full[0])
        for cap in (1, n // 3, n - 1):
            offs = np.full(401, -7, np.int64)
            idx = np.full(n, -5, np.int32)
            dist = np.full(n, -5.0, np.float32)
            assert _call(ctx, qb, tb, r, cap, offs, idx, dist) == n
            assert np.array_equal(offs, full[0])
            m = np.searchsorted(offs, cap, side="right") - 1            # longest prefix of rows that fits
            w = offs[m]
            assert np.array_equal(idx[:w], full[1][:w]) and np.array_equal(dist[:w], full[2][:w])
            assert np.all(idx[w:] == -5), "entries beyond the fitting prefix of rows were written"
        offs = np.zeros(401, np.int64)
        idx = np.empty(n, np.int32)
        dist = np.empty(n, np.float32)
        assert _call(ctx, qb, tb, r, n, offs, idx, dist) == n
        assert np.array_equal(offs, full[0]) and np.array_equal(idx, full[1]) and np.array_equal(dist, full[2])
    finally:
        qb.close()
        tb.close()


def _full_order_i8(Q, T):
    q, t = Q.astype(np.float64), T.astype(np.float64)          # (exact: every sum stays below 2^53)
    d2 = (q * q).sum(1)[:, None] + (t * t).sum(1)[None, :] - 2.0 * (q @ t.T)
    return np.sqrt(np.rint(d2).astype(np.int64).astype(np.float32))


def test_infinite_radius_in_chunks_with_long_segments():
    """r = inf on 1000 x 20000: every train row for every query, sorted; with "radius_ws_bytes" low enough that the call
    takes many query chunks and sorts segments longer than LDS holds (and, on 1000 rows, segments sorted in LDS)."""
    c = fastmatch_amd.Context(0)
    try:
        assert c.get_option("radius_ws_bytes") == 1 << 30
        rng = np.random.default_rng(41)
        Q = synth.synth_sift(1000, rng)
        T = synth.synth_sift(20000, rng)
        c.set_option("radius_ws_bytes", 24 * 20000 * 50)              # 50 rows per chunk
        for nt in (20000, 1000):
            off, idx, dist = c.radius_match(c.bank(Q), c.bank(T[:nt]), np.inf)
            assert np.array_equal(off, np.arange(1001, dtype=np.int64) * nt)
            D = _full_order_i8(Q, T[:nt])
            for i in range(0, 1000, 37):
                want = np.lexsort((np.arange(nt), D[i].view(np.uint32)))
                a = off[i]
                assert np.array_equal(idx[a:a + nt], want) and np.array_equal(dist[a:a + nt], D[i][want])
        Qf, Tf = _floaty(Q[:200], rng), _floaty(T[:3000], rng)
        off, idx, dist = c.radius_match(c.bank(Qf), c.bank(Tf), np.inf)
        assert np.array_equal(off, np.arange(201, dtype=np.int64) * 3000)
        ri, rd = oracle.bf_knn(Qf[::23], Tf, 3000, order=1)
        for k, i in enumerate(range(0, 200, 23)):
            assert np.array_equal(idx[off[i]:off[i + 1]], ri[k]) and np.array_equal(dist[off[i]:off[i + 1]], rd[k])
    finally:
        c.close()


def test_free_memory_unchanged_after_500_calls():
    c = fastmatch_amd.Context(0)
    try:
        rng = np.random.default_rng(43)
        Q = synth.synth_sift(300, rng)
        T = synth.synth_sift(2000, rng)
        banks = [(c.bank(Q), c.bank(T), 400.0), (c.bank(_floaty(Q, rng)), c.bank(_floaty(T, rng)), 0.8)]
        c.set_option("radius_ws_bytes", 1 << 20)
        for qb, tb, r in banks:
            c.radius_match(qb, tb, np.inf)
            c.radius_match(qb, tb, r)
        c.sync()
        free0 = c.mem_info()[0]
        for i in range(500):
            qb, tb, r = banks[i & 1]
            c.radius_match(qb, tb, np.inf if i % 5 == 0 else r)
        c.sync()
        assert c.mem_info()[0] >= free0 - (4 << 20)
    finally:
        c.close()


def test_dmatch_lists(ctx):
    rng = np.random.default_rng(47)
    Q = synth.synth_sift(30, rng)
    T = synth.synth_sift(80, rng)
    lists = matchutil.bf_radius_match(Q, T, 420.0, {"context": ctx})
    ref = _ref(Q, T, 420.0)
    assert len(lists) == 30
    for i, (l, (ri, rd)) in enumerate(zip(lists, ref)):
        assert [m.trainIdx for m in l] == list(ri) and all(m.queryIdx == i for m in l)
        assert [m.distance for m in l] == [float(x) for x in rd]
