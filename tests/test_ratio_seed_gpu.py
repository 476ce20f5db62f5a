"""GPU: the accepted-only calls seed K1 with the ratio test's distance cut (ratio_cut.h) -- their
rows, counts and order must equal the passing rows of fm_match_ratio, which runs the unseeded sweep, and the oracle's."""
import numpy as np
import pytest

import oracle
from fastmatch_amd import synth

pytestmark = pytest.mark.gpu


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8)


def _same(got, want):
    assert len(got) == len(want) == 4
    for g, w in zip(got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (g.dtype, w.dtype, g.shape, w.shape)
        assert np.array_equal(_bits(g), _bits(w))


def _passing(ctx, qb, tb, tau):
    """The accepted rows as the unseeded fm_match_ratio reports them."""
    tidx, dist, ratio, passed, npass = ctx.match_ratio(qb, tb, tau)
    q = np.nonzero(passed)[0].astype(np.int32)
    assert npass == len(q)
    return q, tidx[q], dist[q], ratio[q]


def _oracle(Q, T, sd, tau):
    otidx, odist = oracle.bf_xcheck1(Q, T)
    m = np.nonzero(otidx >= 0)[0]
    oratio, opass = oracle.ratio_filter(odist[m], sd, tau, qrows=m.astype(np.int32))
    q = m[opass].astype(np.int32)
    return q, otidx[q], odist[q], oratio[opass]


def _check(ctx, qb, tb, tau, Q=None, T=None, sd=None, expect_some=False):
    want = _passing(ctx, qb, tb, tau)
    got = ctx.match_accepted(qb, tb, tau)
    _same(got, want)
    if Q is not None:
        _same(got, _oracle(Q, T, sd, tau))
    if expect_some:
        assert len(got[0]) > 0
    return got


def _pair(ctx, Q, T, sd=None):
    qb, tb = ctx.bank(Q), ctx.bank(T)
    if sd is None:
        sd = ctx.self_dist(qb)
    qb.set_selfdist(sd)
    return qb, tb, sd


@pytest.mark.parametrize("seed,p,sigma", [(20250002, 0.3, 6.0), (7, 0.3, 6.0), (8, 0.55, 10.0)])
def test_bench_like_planted_pairs(ctx, seed, p, sigma):
    """Planted pairs as the benchmark draws them, large enough for many splits and cross-workgroup bounds."""
    Q, T, _ = synth.planted_pair(24000, 20000, seed=seed, p=p, sigma=sigma)
    qb, tb, _ = _pair(ctx, Q, T)
    got = _check(ctx, qb, tb, 0.7, expect_some=True)
    assert len(got[0]) > 0.2 * 20000 * p


def test_planted_pair_against_oracle(ctx):
    Q, T, _ = synth.planted_pair(2500, 3000, seed=3)
    qb, tb, sd = _pair(ctx, Q, T)
    for tau in (0.7, 0.0, 1.0, 5.0, float("nan")):
        _check(ctx, qb, tb, tau, Q, T, sd)


def _delta(rng, d2, dim=128):
    """An integer vector of squared length d2 with entries in [-40, 40] on distinct dimensions."""
    v = np.zeros(dim, np.int64)
    left = d2
    dims = rng.permutation(dim)
    k = 0
    while left > 0:
        a = min(int(np.sqrt(left)), 40)
        v[dims[k]] = a if rng.random() < 0.5 else -a
        left -= a * a
        k += 1
    assert (v * v).sum() == d2
    return v


def test_matches_on_both_sides_of_the_cut(ctx):
    """Every query row has exactly one close partner at a chosen d2; with all self distances S and tau = sqrtf(K) / S the
    cut is D* = K: partners at K - 2, K - 1 are accepted, at K, K + 1 rejected (ratio == tau is not < tau)."""
    rng = np.random.default_rng(31)
    nq, K, S = 1024, 2000, 100.0
    Q = rng.integers(45, 211, (nq, 128)).astype(np.uint8)
    offs = np.array([K - 2, K - 1, K, K + 1])[np.arange(nq) % 4]
    T = np.stack([(Q[i].astype(np.int64) + _delta(rng, int(offs[i]))) for i in range(nq)]).astype(np.uint8)
    perm = rng.permutation(nq)
    T = T[perm]
    sd = np.full(nq, S)
    tau = float(np.sqrt(np.float32(K))) / S
    qb, tb, _ = _pair(ctx, Q, T, sd)
    q, t, d, r = _check(ctx, qb, tb, tau, Q, T, sd, expect_some=True)
    assert set(q.tolist()) == set(np.nonzero(offs < K)[0].tolist())
    assert np.array_equal(perm[t], q)


def test_duplicate_query_rows(ctx):
    """Duplicates have self distance 0: they can never pass, and do not weaken the cut of the other rows."""
    Q, T, _ = synth.planted_pair(3000, 3500, seed=12)
    Q[100:140] = Q[10]
    Q[700] = Q[2999]
    qb, tb, sd = _pair(ctx, Q, T)
    assert (sd == 0).sum() >= 42
    _check(ctx, qb, tb, 0.7, Q, T, sd, expect_some=True)


def test_one_row_query_bank(ctx):
    """One query row: its self distance is +inf, no cut (the ratio is 0 or NaN, never accepted either way)."""
    Q, T, _ = synth.planted_pair(1, 5000, seed=13)
    qb, tb, sd = _pair(ctx, Q, T)
    assert np.isinf(sd[0])
    _check(ctx, qb, tb, 0.7, Q, T, sd)


@pytest.mark.parametrize("special", [np.inf, np.nan, 0.0, -0.0, -1.0, 1e-300])
def test_caller_self_distances(ctx, special):
    """fm_bank_set_selfdist with caller values: one odd value among normal ones -- inf, NaN and sign bits mean no cut;
    0 and tiny values keep it."""
    Q, T, _ = synth.planted_pair(3000, 3000, seed=14)
    qb, tb = ctx.bank(Q), ctx.bank(T)
    sd = ctx.self_dist(qb)
    sd[[5, 1700]] = special
    qb.set_selfdist(sd)
    for tau in (0.7, 1.0):
        _check(ctx, qb, tb, tau, Q, T, sd)


def test_float32_root_tie_range(ctx):
    """Distances above 4 197 200 (query rows near 0, train rows near 255), where neighbouring d2 share a float32 root; tau
    puts the cut among the winners' distances, on a root shared by two integers where one exists."""
    rng = np.random.default_rng(15)
    Q = rng.integers(0, 30, (700, 128)).astype(np.uint8)
    T = rng.integers(225, 256, (900, 128)).astype(np.uint8)
    sd = np.full(700, 1000.0)
    otidx, odist = oracle.bf_xcheck1(Q, T)
    w = np.sort(odist[otidx >= 0].astype(np.float64))
    assert w[0] ** 2 > 4197200
    qb, tb, _ = _pair(ctx, Q, T, sd)
    for x in (w[len(w) // 4], w[len(w) // 2], w[(3 * len(w)) // 4]):
        _check(ctx, qb, tb, float(x) / 1000.0, Q, T, sd)


def _batch(ctx, pairs, tau, cap):
    outs = [(ctx.pinned_empty(cap, np.int32), ctx.pinned_empty(cap, np.int32), ctx.pinned_empty(cap, np.float32),
             ctx.pinned_empty(cap, np.float64)) for _ in pairs]
    cnts = [ctx.pinned_empty(1, np.int64) for _ in pairs]
    ctx.match_accepted_batch(pairs, tau, outs, cnts)
    ctx.sync()
    return [tuple(np.array(a[:int(c[0])]) for a in o) for o, c in zip(outs, cnts)]


def _mixed_pairs(ctx):
    """Pairs with a cut (normal self distances), without one (a NaN among them; a one-row query bank), of several sizes."""
    pairs = []
    for k in range(6):
        Q, T, _ = synth.planted_pair(4000 + 500 * k, 5000, seed=40 + k)
        qb, tb = ctx.bank(Q), ctx.bank(T)
        sd = ctx.self_dist(qb)
        if k == 2:
            sd[77] = np.nan
        qb.set_selfdist(sd)
        pairs.append((qb, tb))
    Q1, T1, _ = synth.planted_pair(1, 3000, seed=50)
    q1, t1, _ = _pair(ctx, Q1, T1)
    pairs.insert(3, (q1, t1))
    return pairs


def test_batch_mixes_pairs_with_and_without_a_cut(ctx):
    pairs = _mixed_pairs(ctx)
    for tau in (0.7, 1.0):
        got = _batch(ctx, pairs, tau, 7000)
        for (qb, tb), g in zip(pairs, got):
            _same(g, _passing(ctx, qb, tb, tau))


def test_dev_batch(ctx):
    import torch
    from fastmatch_amd import sharding
    pairs = _mixed_pairs(ctx)
    cap = 7000
    dev = torch.device("cuda", 0)
    rows = torch.full((len(pairs), cap, 3), -7, dtype=torch.int32, device=dev)
    cnts = torch.zeros(len(pairs), dtype=torch.int64, device=dev)
    ctx.match_accepted_dev_batch(pairs, 0.7, rows.data_ptr(), cnts.data_ptr(), cap)
    ctx.sync()
    torch.cuda.synchronize()
    rows, cnts = rows.cpu().numpy(), cnts.cpu().numpy()
    for k, (qb, tb) in enumerate(pairs):
        q, t, d, _ = _passing(ctx, qb, tb, 0.7)
        assert int(cnts[k]) == len(q)
        assert np.array_equal(rows[k, :len(q)], sharding.pack_matches(q, t, d))


def test_async_and_dev_single_pair(ctx):
    import torch
    Q, T, _ = synth.planted_pair(6000, 6000, seed=60)
    qb, tb, _ = _pair(ctx, Q, T)
    want = _passing(ctx, qb, tb, 0.7)
    out = (ctx.pinned_empty(6000, np.int32), ctx.pinned_empty(6000, np.int32), ctx.pinned_empty(6000, np.float32),
           ctx.pinned_empty(6000, np.float64))
    cnt = ctx.pinned_empty(1, np.int64)
    ctx.match_accepted_async(qb, tb, 0.7, out, cnt)
    ctx.sync()
    _same(tuple(np.array(a[:int(cnt[0])]) for a in out), want)
    dev = torch.device("cuda", 0)
    rows = torch.zeros((6000, 3), dtype=torch.int32, device=dev)
    c = torch.zeros(1, dtype=torch.int64, device=dev)
    assert ctx.match_accepted_dev(qb, tb, 0.7, rows.data_ptr(), c.data_ptr(), 6000) == len(want[0])


def test_refilled_bank(ctx):
    """A bank refilled after its self distances were set: to fewer rows (the old values still bound the ones read: the cut
    stays), to more rows (values beyond those reduced: no cut), and recomputed by fm_self_dist_batch."""
    Q, T, _ = synth.planted_pair(5000, 5000, seed=70)
    qb, tb, _ = _pair(ctx, Q, T)
    _check(ctx, qb, tb, 0.7, expect_some=True)
    Q2, _, _ = synth.planted_pair(3000, 10, seed=71)
    Q2[:1500] = Q[:1500]
    src = ctx.pinned_empty((3000, 128), np.uint8)
    src[:] = Q2
    qb.refill_async(src)
    ctx.upload_fence()
    _check(ctx, qb, tb, 0.7, expect_some=True)
    Q3 = ctx.pinned_empty((5100, 128), np.uint8)         # (within the bank's capacity: 5120 padded rows)
    Q3[:5000] = Q
    Q3[5000:] = T[:100]
    qb.refill_async(Q3)
    ctx.upload_fence()
    _check(ctx, qb, tb, 0.7, expect_some=True)
    ctx.self_dist_batch([qb], want_host=False)
    _check(ctx, qb, tb, 0.7, expect_some=True)
    sd3 = ctx.self_dist_batch([qb])[0]
    _check(ctx, qb, tb, 0.7, np.array(Q3), T, sd3, expect_some=True)
