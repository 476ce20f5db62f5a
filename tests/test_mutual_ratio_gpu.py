"""GPU: mutual nearest neighbours + ratio test on a bank pair (fm_mutual_ratio, its device form, torchmatch.mutual_ratio_match),
bit for bit against
  * the composition it replaces: the rows of Context.knn2_ratio(q, t, tau) filtered with Context.knn(t, q, 2) by the
    contract's rules 2 and 3 -- code older than this entry point,
  * the NumPy reference (tests/mutual_ratio_ref.py) on a structured input, mass ties and the float32-root tie banks."""
import ctypes
import os
import sys

import numpy as np
import pytest

from fastmatch_amd import _ffi, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f32_regimes                              # noqa: E402
import kat                                      # noqa: E402
import mutual_ratio_ref as ref                  # noqa: E402

pytestmark = pytest.mark.gpu

EINVAL, EUNSUP = -1, -4
INF = float("inf")
KINDS = ("u8", "f32int", "f32", "f32nofilter", "bin1", "bin32", "bin64")
SHAPES = [(0, 5), (5, 0), (1, 1), (2, 2), (1, 300), (300, 1), (127, 129), (129, 127), (300, 257), (1000, 4099), (4099, 1000)]
TAUS = (0.0, 0.8, INF)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want, what):
    assert np.array_equal(got[0], want[0]), what + ": query rows"
    assert np.array_equal(got[1], want[1]), what + ": train rows"
    assert np.array_equal(_bits(got[2]), _bits(want[2])), what + ": distances"
    assert np.array_equal(np.asarray(got[3]).view(np.uint64), np.asarray(want[3]).view(np.uint64)), what + ": ratios"


def _pair(kind, nq, nt, seed=0):
    """(Q, T) of a kind: a third of the query rows are noisy copies of train rows (some of one train row twice), so that ratio
    passes, mutual pairs and shared first neighbours all occur; deterministic."""
    rng = np.random.default_rng(3100 + 17 * KINDS.index(kind) + nq + 3 * nt + seed)
    if kind.startswith("bin"):
        w = int(kind[3:])
        T = rng.integers(0, 256, (nt, w), dtype=np.uint8)
        Q = rng.integers(0, 256, (nq, w), dtype=np.uint8)

        def noisy(row):
            out = row.copy()
            out[rng.integers(0, w)] ^= np.uint8(1 << rng.integers(0, 8))
            return out
    elif kind in ("u8", "f32int"):
        T = synth.synth_sift(max(nt, 1), rng)[:nt].copy()
        Q = synth.synth_sift(max(nq, 1), rng)[:nq].copy()

        def noisy(row):
            return np.clip(row.astype(np.int32) + rng.integers(-4, 5, row.shape), 0, 255).astype(np.uint8)
    else:
        T = rng.normal(0.0, 1.0, (nt, 128)).astype(np.float32)
        Q = rng.normal(0.0, 1.0, (nq, 128)).astype(np.float32)

        def noisy(row):
            return (row + rng.normal(0.0, 0.05, row.shape)).astype(np.float32)
    if nt:
        for j in range(0, nq, 3):
            Q[j] = noisy(T[(j * 7) % nt])
        for j in range(1, nq, 12):                 # a second, independent view of a train row that has one already
            Q[j] = noisy(T[((j - 1) * 7) % nt])
    if kind == "f32int":
        Q, T = Q.astype(np.float32), T.astype(np.float32)
    return Q, T


def _banks(ctx, kind, Q, T):
    if kind.startswith("bin"):
        return ctx.bank_binary(Q), ctx.bank_binary(T)
    fr = kind in ("f32", "f32nofilter")
    return ctx.bank(Q, float_route=fr), ctx.bank(T, float_route=fr)


def _filter_option(kind):
    return 2 if kind == "f32" else 0 if kind == "f32nofilter" else 1


def _compose(ctx, qb, tb, tau, symmetric):
    """The composition from older entry points: knn2_ratio's rows kept by rules 2 and 3 on knn(t, q, 2)."""
    qi, ti, d, r = ctx.knn2_ratio(qb, tb, tau)
    if qi.shape[0] == 0:
        return qi, ti, d, r, 0
    ridx, rdist = ctx.knn(tb, qb, 2)
    keep = ridx[ti, 0] == qi
    if symmetric:
        with np.errstate(divide="ignore", invalid="ignore"):
            rr = np.where(ridx[ti, 1] >= 0, rdist[ti, 0].astype(np.float64) / rdist[ti, 1].astype(np.float64), np.nan)
            keep &= rr < tau
        r = np.where(keep, np.maximum(r, rr), r)
    return qi[keep], ti[keep], d[keep], r[keep], qi.shape[0]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("kind", KINDS)
def test_equals_the_composition(ctx, kind, shape):
    nq, nt = shape
    Q, T = _pair(kind, nq, nt)
    qb, tb = _banks(ctx, kind, Q, T)
    try:
        ctx.set_option("f32_filter", _filter_option(kind))
        for tau in TAUS:
            for sym in (False, True):
                want = _compose(ctx, qb, tb, tau, sym)
                got = ctx.mutual_ratio(qb, tb, tau, sym)
                _same(got, want, "%s %dx%d tau=%s sym=%d" % (kind, nq, nt, tau, sym))
                assert ctx.mutual_ratio_count(qb, tb, tau, sym) == got[0].shape[0]
                assert (got[3] < tau).all()
                if tau == 0.0:
                    assert want[4] == 0 and got[0].shape[0] == 0                  # no candidates at all
                if tau == INF and nt >= 2 and not kind.startswith("bin1"):
                    assert want[4] >= nq - nq // 50                              # the gather sees (nearly) every query row
        if nq >= 127 and nt >= 127 and kind != "bin1":
            assert ctx.mutual_ratio(qb, tb, 0.8)[0].shape[0] >= 10                  # the planted pairs are found
    finally:
        ctx.set_option("f32_filter", 1)
        qb.close()
        tb.close()


@pytest.mark.parametrize("binary", [False, True])
def test_structured_input_against_the_reference(ctx, binary):
    Q, T = ref.structured(1, binary)
    t0, d0, fwd, ok, mutual, rev = ref.classes(Q, T, 0.8, binary)
    acc = ok & mutual
    with np.errstate(invalid="ignore"):
        sym_ok = acc & (rev < 0.8)
    # (asserted on the reference alone, before the device is looked at)
    assert min((ok & ~mutual).sum(), (mutual & ~ok).sum(), acc.sum(), (acc & ~sym_ok).sum()) >= 10
    qb, tb = (ctx.bank_binary(Q), ctx.bank_binary(T)) if binary else (ctx.bank(Q), ctx.bank(T))
    try:
        for tau in (0.8, 0.95, INF):
            for sym in (False, True):
                _same(ctx.mutual_ratio(qb, tb, tau, sym), ref.mutual_ratio(Q, T, tau, sym, binary), "tau=%s sym=%d" % (tau, sym))
    finally:
        qb.close()
        tb.close()


@pytest.mark.parametrize("binary", [False, True])
def test_mass_ties_take_the_lowest_index_in_both_directions(ctx, binary):
    """2000 x 4099 rows drawn from small pools: every distance is tied many times over.  The query and train pools are
    disjoint (d0 = d1 > 0: ratio 1, kept by tau = inf, dropped by tau = 1), so the accepted rows are exactly the
    lowest-index query row per elected train row, at the lowest-index train row."""
    rng = np.random.default_rng(3300)
    if binary:
        par = np.array([bin(v).count("1") & 1 for v in range(256)])
        tp, qp = np.nonzero(par == 0)[0].astype(np.uint8), np.nonzero(par == 1)[0].astype(np.uint8)
        Q, T = qp[rng.integers(0, len(qp), 2000)][:, None], tp[rng.integers(0, len(tp), 4099)][:, None]
    else:
        pool = synth.synth_sift(24, rng)
        Q, T = pool[rng.integers(0, 12, 2000)], pool[12 + rng.integers(0, 12, 4099)]
    qb, tb = (ctx.bank_binary(Q), ctx.bank_binary(T)) if binary else (ctx.bank(Q), ctx.bank(T))
    try:
        for sym in (False, True):
            want = ref.mutual_ratio(Q, T, INF, sym, binary)
            got = ctx.mutual_ratio(qb, tb, INF, sym)
            _same(got, want, "ties sym=%d" % sym)
            _same(got, _compose(ctx, qb, tb, INF, sym), "ties sym=%d, composition" % sym)
            assert ctx.mutual_ratio(qb, tb, 1.0, sym)[0].shape[0] == 0
        got = ctx.mutual_ratio(qb, tb, INF)
        assert 0 < got[0].shape[0] <= (128 if binary else 12) and (got[3] == 1.0).all()
        assert len(set(got[1].tolist())) == got[1].shape[0]                          # one query row per train row
    finally:
        qb.close()
        tb.close()


def test_float32_root_ties(ctx):
    cases = [(n, Q, T) for n, Q, T, _, _ in kat.sqrt_tie_knn2_cases()] + [(n, Q, T) for n, Q, T, _, _ in kat.sqrt_tie_xcheck_cases()]
    rng = np.random.default_rng(3400)
    cases.append(("far_banks",) + tuple(kat.far_banks(300, 500, rng)))
    for name, Q, T in cases:
        qb, tb = ctx.bank(Q), ctx.bank(T)
        try:
            for sym in (False, True):
                got = ctx.mutual_ratio(qb, tb, INF, sym)
                _same(got, ref.mutual_ratio(Q, T, INF, sym), name + " sym=%d" % sym)
                _same(got, _compose(ctx, qb, tb, INF, sym), name + " sym=%d, composition" % sym)
        finally:
            qb.close()
            tb.close()


@pytest.mark.parametrize("kind", ("u8", "f32", "bin32"))
def test_cross_link_with_xcheck1(ctx, kind):
    """tau = inf, symmetric = 0: the accepted set is {i : xcheck1(q, t)[i] == knn2(q, t)[i, 0] >= 0 and the ratio is a number}."""
    Q, T = _pair(kind, 1000, 4099, seed=1)
    qb, tb = _banks(ctx, kind, Q, T)
    try:
        xt, xd = ctx.xcheck1(qb, tb)
        idx, dist = ctx.knn2(qb, tb)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = dist[:, 0].astype(np.float64) / dist[:, 1].astype(np.float64)
        want = np.nonzero((xt == idx[:, 0]) & (idx[:, 0] >= 0) & (idx[:, 1] >= 0) & (r < INF))[0]
        got = ctx.mutual_ratio(qb, tb, INF)
        assert np.array_equal(got[0], want) and np.array_equal(got[1], idx[want, 0])
        assert np.array_equal(_bits(got[2]), _bits(xd[want])) and want.shape[0] > 100
    finally:
        qb.close()
        tb.close()


def test_caps_counts_and_stats(ctx):
    Q, T = _pair("u8", 1000, 4099, seed=2)
    qb, tb = ctx.bank(Q), ctx.bank(T)
    try:
        full = ctx.mutual_ratio(qb, tb, 0.8)
        m = full[0].shape[0]
        assert m > 20
        cut = ctx.mutual_ratio(qb, tb, 0.8, cap=7)                  # a prefix of the rows ...
        _same(cut, tuple(a[:7] for a in full), "cap 7")
        n = ctypes.c_int64(-1)
        out = (np.full(7, -5, np.int32), np.full(7, -5, np.int32), np.zeros(7, np.float32), np.zeros(7, np.float64))
        rc = ctx.lib.fm_mutual_ratio(ctx.handle, qb.handle, tb.handle, 0.8, 0, 7, _ffi._ptr(out[0]), _ffi._ptr(out[1]), _ffi._ptr(out[2]),
                                     _ffi._ptr(out[3]), ctypes.byref(n))
        assert rc == 0 and n.value == m                              # ... and the full count
        rc = ctx.lib.fm_mutual_ratio(ctx.handle, qb.handle, tb.handle, 0.8, 0, 0, None, None, None, None, ctypes.byref(n))
        assert rc == 0 and n.value == m                              # cap = 0 with NULL arrays: the count only
        # stats: one call adds nq * nt + n_cand * nq pairs, n_cand = knn2_ratio's count
        n_cand = ctx.knn2_ratio(qb, tb, 0.8)[0].shape[0]
        assert n_cand > m
        ctx.reset_stats()
        ctx.mutual_ratio(qb, tb, 0.8, True)
        st = ctx.stats()
        assert st["pairs"] == 1000 * 4099 + n_cand * 1000 and st["calls"] == 1
        ctx.reset_stats()
        ctx.mutual_ratio(qb, tb, 0.0)
        assert ctx.stats()["pairs"] == 1000 * 4099
    finally:
        qb.close()
        tb.close()


def test_refusals_in_order_and_the_banks_still_answer(ctx):
    Q, T = _pair("u8", 129, 127)
    qb, tb = ctx.bank(Q), ctx.bank(T)
    bb = ctx.bank_binary(np.zeros((4, 64), np.uint8))
    q64 = ctx.bank(np.zeros((4, 64), np.uint8))          # (as wide as the binary rows: the kinds differ, not the widths)
    lib, h = ctx.lib, ctx.handle
    n = ctypes.c_int64(77)
    a = (np.zeros(200, np.int32), np.zeros(200, np.int32), np.zeros(200, np.float32), np.zeros(200, np.float64))
    p = [_ffi._ptr(x) for x in a]
    try:
        before = ctx.mutual_ratio(qb, tb, 0.8)
        assert lib.fm_mutual_ratio(None, qb.handle, tb.handle, 0.8, 0, 200, *p, ctypes.byref(n)) == EINVAL
        assert lib.fm_mutual_ratio(h, None, tb.handle, 0.8, 0, 200, *p, ctypes.byref(n)) == EINVAL
        assert lib.fm_mutual_ratio(h, qb.handle, None, 0.8, 0, 200, *p, ctypes.byref(n)) == EINVAL
        # the pair comes before the outputs: a binary bank with a non-binary one, even with a bad cap
        assert lib.fm_mutual_ratio(h, q64.handle, bb.handle, 0.8, 0, -1, *p, ctypes.byref(n)) == EINVAL
        assert "binary" in ctx.lib.fm_last_error(h).decode().lower()
        assert lib.fm_mutual_ratio(h, qb.handle, tb.handle, 0.8, 0, -1, *p, ctypes.byref(n)) == EINVAL and n.value == 0
        assert lib.fm_mutual_ratio(h, qb.handle, tb.handle, 0.8, 0, 5, p[0], None, p[2], p[3], ctypes.byref(n)) == EINVAL
        NOS = _ffi._stream_arg(None)
        assert lib.fm_mutual_ratio_dev(h, q64.handle, bb.handle, 0.8, 0, 5, None, None, None, NOS) == EINVAL
        assert lib.fm_mutual_ratio_dev(h, qb.handle, tb.handle, 0.8, 0, 5, None, None, None, NOS) == EINVAL          # d_count NULL
        assert lib.fm_mutual_ratio_dev(h, qb.handle, tb.handle, 0.8, 0, 5, p[0], p[1], None, NOS) == EINVAL          # host memory
        assert "device" in ctx.lib.fm_last_error(h).decode().lower()
        _same(ctx.mutual_ratio(qb, tb, 0.8), before, "after the refusals")
    finally:
        for b in (qb, tb, bb, q64):
            b.close()


@pytest.mark.parametrize("kind", ("u8", "f16", "f32", "bin32"))
def test_device_forms_equal_the_host_form(ctx, kind):
    import torch
    from fastmatch_amd import torchmatch
    base = {"f16": "f32"}.get(kind, kind)
    Q, T = _pair(base, 700, 1500, seed=3)
    if kind == "f16":
        Q, T = Q.astype(np.float16), T.astype(np.float16)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):                                   # a non-default current stream
        tq, tt = torch.from_numpy(Q).cuda(), torch.from_numpy(T).cuda()
        if kind == "bin32":
            q, t = torchmatch.bank(tq, binary=True, context=ctx), torchmatch.bank(tt, binary=True, context=ctx)
        else:
            q, t = torchmatch.bank(tq, context=ctx), torchmatch.bank(tt, context=ctx)
        try:
            for tau, sym in ((0.8, False), (0.8, True), (INF, True), (0.0, False)):
                want = ctx.mutual_ratio(q, t, tau, sym)
                m = want[0].shape[0]
                for cap in (700, 5, 0):
                    rows = torch.full((max(cap, 1), 3), -7, dtype=torch.int32, device="cuda")
                    count = torch.full((1,), -7, dtype=torch.int64, device="cuda")
                    total = ctx.mutual_ratio_dev(q, t, tau, sym, rows.data_ptr() if cap else 0, count.data_ptr(), cap, want_count=True,
                                                 consumer_stream=side.cuda_stream)
                    k = min(m, cap)
                    assert total == m and int(count.item()) == k
                    got = rows[:k].cpu().numpy()
                    assert np.array_equal(got[:, 0], want[0][:k]) and np.array_equal(got[:, 1], want[1][:k])
                    assert np.array_equal(got[:, 2].view(np.uint32), _bits(want[2][:k]))
                    assert (rows[k:] == -7).all()
                qi, ti, d = torchmatch.mutual_ratio_match(q if kind == "bin32" else tq, t if kind == "bin32" else tt, tau, sym)
                assert np.array_equal(qi.cpu().numpy(), want[0]) and np.array_equal(ti.cpu().numpy(), want[1])
                assert np.array_equal(_bits(d.cpu().numpy()), _bits(want[2]))
            assert ctx.mutual_ratio(q, t, 0.8)[0].shape[0] >= 10
        finally:
            q.close()
            t.close()
    side.synchronize()
