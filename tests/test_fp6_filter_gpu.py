"""GPU: the accepted-only sweep as an FP6 filter with exact rescoring (filter6.hip; option "fp6_filter") must report, byte for
byte, what K1 reports (option 0) -- query rows, train rows, distance bits, ratio bits, counts -- and what the oracle reports.
The pairs go through the batched call, which plans every pair in the filter's shape whatever its size."""
import numpy as np
import pytest

import oracle
from fastmatch_amd import synth

pytestmark = pytest.mark.gpu

TAU = 0.7


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(got, want):
    assert len(got) == len(want) == 4
    for g, w in zip(got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (g.dtype, w.dtype, g.shape, w.shape)
        assert np.array_equal(_bits(g), _bits(w))


def _oracle(Q, T, sd, tau):
    otidx, odist = oracle.bf_xcheck1(Q, T)
    m = np.nonzero(otidx >= 0)[0]
    oratio, opass = oracle.ratio_filter(odist[m], sd, tau, qrows=m.astype(np.int32))
    q = m[opass].astype(np.int32)
    return q, otidx[q], odist[q], oratio[opass]


def _batch(ctx, pairs, tau):
    cap = max(qb.n for qb, _ in pairs)
    outs = [(ctx.pinned_empty(cap, np.int32), ctx.pinned_empty(cap, np.int32), ctx.pinned_empty(cap, np.float32),
             ctx.pinned_empty(cap, np.float64)) for _ in pairs]
    cnts = [ctx.pinned_empty(1, np.int64) for _ in pairs]
    ctx.match_accepted_batch(pairs, tau, outs, cnts)
    ctx.sync()
    return [tuple(np.array(a[:int(c[0])]) for a in o) for o, c in zip(outs, cnts)]


def _ab(ctx, pairs, tau, cap=None):
    """The batch under the filter and under K1: (filter results, K1 results, records, fallbacks) after asserting equality."""
    keep = ctx.get_option("fp6_cap")
    try:
        if cap is not None:
            ctx.set_option("fp6_cap", cap)
        ctx.set_option("fp6_filter", 1)
        got = _batch(ctx, pairs, tau)
        rec, fb = ctx.get_option("fp6_records"), ctx.get_option("fp6_fallbacks")
        ctx.set_option("fp6_filter", 0)
        want = _batch(ctx, pairs, tau)
    finally:
        ctx.set_option("fp6_filter", 1)
        ctx.set_option("fp6_cap", keep)
    for g, w in zip(got, want):
        _same(g, w)
    return got, want, rec, fb


def _pair(ctx, Q, T, sd=None):
    qb, tb = ctx.bank(Q), ctx.bank(T)
    if sd is None:
        sd = ctx.self_dist(qb)
    qb.set_selfdist(sd)
    return qb, tb, sd


def _dstar(sd_max, tau):
    """ratio_cut_d2 (ratio_cut.h) on the host: the smallest d2 with !((double)sqrtf((float)d2) / sd_max < tau)."""
    fails = lambda d2: not (float(np.sqrt(np.float32(d2))) / sd_max < tau)
    lo, hi = 0, 0xffffffff
    assert fails(hi)
    while lo < hi:
        mid = (lo + hi) // 2
        if fails(mid):
            hi = mid
        else:
            lo = mid + 1
    return lo


SHAPES = [(300, 257), (1000, 3001), (4099, 5000), (5000, 4099), (100, 90)]


@pytest.fixture(scope="module")
def planted(ctx):
    """The planted pairs of every shape with their banks, self distances and oracle rows (computed once)."""
    out = []
    for k, (nq, nt) in enumerate(SHAPES):
        Q, T, _ = synth.planted_pair(nq, nt, seed=100 + k)
        qb, tb, sd = _pair(ctx, Q, T)
        out.append((Q, T, sd, qb, tb, _oracle(Q, T, sd, TAU)))
    return out


def test_planted_pairs_of_mixed_sizes_in_one_batch(ctx, planted):
    """Partial last chunk, stage, unit and split; a pair below 128 rows; all five in one launch."""
    pairs = [(p[3], p[4]) for p in planted]
    got, _, rec, fb = _ab(ctx, pairs, TAU)
    assert rec > 0 and fb == 0          # (the filter ran, and kept its hits within the list)
    for g, p in zip(got, planted):
        _same(g, p[5])
        assert len(g[0]) > 0


def _delta(rng, d2, dims):
    """An integer vector of squared length d2 with entries of magnitude <= 40 on the given dimensions."""
    v = np.zeros(128, np.int64)
    left, k = d2, 0
    while left > 0:
        a = min(int(np.sqrt(left)), 40)
        v[dims[k]] = a if rng.random() < 0.5 else -a
        left -= a * a
        k += 1
    assert (v * v).sum() == d2
    return v


def test_copies_at_the_cut(ctx):
    """Every query row is a copy of one train row at exactly d2 = D* - 1, D* or D* + 1 (D* from the cut's own arithmetic on
    the host): the copy at D* - 1 with one more byte moved by 1 is at D*, with two at D* + 1.  Only D* - 1 is accepted."""
    rng = np.random.default_rng(41)
    nq, S = 1500, 450.0
    D = _dstar(S, TAU)
    assert 300 ** 2 < D < 330 ** 2
    T = rng.integers(45, 211, (nq + 700, 128)).astype(np.uint8)
    perm = rng.permutation(len(T))[:nq]
    Q = np.empty((nq, 128), np.uint8)
    kind = np.arange(nq) % 3
    for i in range(nq):
        dims = rng.permutation(128)
        v = _delta(rng, D - 1, dims[2:])
        v[dims[0]] = 1 if kind[i] >= 1 else 0
        v[dims[1]] = -1 if kind[i] >= 2 else 0
        Q[i] = (T[perm[i]].astype(np.int64) + v).astype(np.uint8)
    assert np.array_equal(((Q.astype(np.int64) - T[perm]) ** 2).sum(1), D - 1 + kind)
    sd = np.full(nq, S)
    qb, tb, _ = _pair(ctx, Q, T, sd)
    Q2, T2, _ = synth.planted_pair(700, 600, seed=42)
    q2, t2, _ = _pair(ctx, Q2, T2)
    got, _, rec, fb = _ab(ctx, [(qb, tb), (q2, t2)], TAU)
    assert rec >= nq // 3 and fb == 0
    q, t, d, r = got[0]
    _same(got[0], _oracle(Q, T, sd, TAU))
    assert set(q.tolist()) == set(np.nonzero(kind == 0)[0].tolist())
    assert np.array_equal(t, perm[q])


TIES = [(31, 32), (127, 128), (1023, 1024), (2047, 2048), (3071, 3072), (4095, 4096), (63, 4999)]


def _tied_pair(seed):
    """5000 query rows against 4099 train rows (five splits of 1024 query rows); query rows a and b of every TIES entry are
    one noisy copy of a train row."""
    Q, T, _ = synth.planted_pair(5000, 4099, seed=seed)
    rng = np.random.default_rng(seed + 1)
    for k, (a, b) in enumerate(TIES):
        Q[a] = np.clip(T[40 * k + 7].astype(np.int64) + rng.integers(-6, 7, 128), 0, 255)
        Q[b] = Q[a]
    return Q, T


def test_ties_across_unit_stage_and_split_boundaries(ctx):
    """Duplicate query rows on both sides of a 32-row unit boundary, of a stage boundary and of the boundaries between the
    sweep's splits: the train row they copy must elect the lower one.  Caller self distances, so that duplicates (self
    distance 0 otherwise) can be accepted."""
    Q, T = _tied_pair(51)
    sd = np.full(5000, 450.0)
    qb, tb, _ = _pair(ctx, Q, T, sd)
    Q2, T2, _ = synth.planted_pair(900, 1100, seed=53)
    q2, t2, _ = _pair(ctx, Q2, T2)
    got, _, rec, fb = _ab(ctx, [(q2, t2), (qb, tb)], TAU)
    assert rec > 0 and fb == 0
    _same(got[1], _oracle(Q, T, sd, TAU))
    q = got[1][0].tolist()
    for a, b in TIES:
        assert a in q and b not in q


def test_rows_of_255s_and_of_0s_on_both_sides(ctx):
    """A row of 255s has the largest rounding error there is (15 per byte): the worst-case bound then lets most of the sweep
    through -- the list may overflow and K1 redo the pair; the results must not care."""
    Q, T = _tied_pair(55)
    Q[500], Q[501], T[600], T[601] = 255, 0, 255, 0
    Q[502] = np.where(np.arange(128) == 5, 254, 255)
    T[602] = np.where(np.arange(128) == 9, 1, 0)
    sd = np.full(5000, 450.0)
    qb, tb, _ = _pair(ctx, Q, T, sd)
    Q2, T2, _ = synth.planted_pair(900, 1100, seed=53)
    Q2[3], T2[4], Q2[5], T2[6] = 0, 0, 255, 255
    q2, t2, sd2 = _pair(ctx, Q2, T2)
    got, _, rec, fb = _ab(ctx, [(q2, t2), (qb, tb)], TAU)
    assert rec > 0
    _same(got[0], _oracle(Q2, T2, sd2, TAU))
    _same(got[1], _oracle(Q, T, sd, TAU))
    q = got[1][0].tolist()
    assert 500 in q and 501 in q and 31 in q and 32 not in q


def test_list_overflow_falls_back_to_k1(ctx, planted):
    """One query row with a huge self distance cuts the ratio test loose: most blocks of the sweep fire.  With a list of 64
    records the pair overflows and K1 redoes it on the device; with the default list it fits."""
    Q, T, sd, _, _, _ = planted[1]
    sd = sd.copy()
    sd[17] = 900.0
    qb, tb, _ = _pair(ctx, Q, T, sd)
    _, _, _, qb0, tb0, want0 = planted[0]
    got, _, rec, fb = _ab(ctx, [(qb, tb), (qb0, tb0)], TAU, cap=64)
    assert rec > 64 and fb >= 1
    _same(got[0], _oracle(Q, T, sd, TAU))
    _same(got[1], want0)
    got, _, rec, fb = _ab(ctx, [(qb, tb), (qb0, tb0)], TAU)
    assert rec > 64 and fb == 0
    _same(got[0], _oracle(Q, T, sd, TAU))


def test_calls_without_a_cut_stay_on_k1(ctx, planted):
    """tau = NaN (no filter launch at all) and a NaN among the self distances (no finite cut, known on the device only: the
    guarded K1 redoes the pair)."""
    Q, T, sd, qb, tb, _ = planted[2]
    _, _, _, qb0, tb0, _ = planted[0]
    got, _, _, _ = _ab(ctx, [(qb, tb), (qb0, tb0)], float("nan"))
    assert len(got[0][0]) == 0
    sdn = sd.copy()
    sdn[33] = np.nan
    qn, tn, _ = _pair(ctx, Q, T, sdn)
    got, _, rec, fb = _ab(ctx, [(qn, tn), (qb0, tb0)], TAU)
    assert fb == 1
    _same(got[0], _oracle(Q, T, sdn, TAU))


def test_refilled_banks(ctx):
    """A query bank refilled to other contents and to fewer rows, a train bank refilled too: the FP6 plane follows."""
    Q, T, _ = synth.planted_pair(3000, 2600, seed=61)
    qb, tb, sd = _pair(ctx, Q, T)
    Q0, T0, _ = synth.planted_pair(400, 500, seed=62)
    q0, t0, _ = _pair(ctx, Q0, T0)
    _ab(ctx, [(qb, tb), (q0, t0)], TAU)
    Q2, T2, _ = synth.planted_pair(1700, 2100, seed=63)
    srcq, srct = ctx.pinned_empty((1700, 128), np.uint8), ctx.pinned_empty((2100, 128), np.uint8)
    srcq[:], srct[:] = Q2, T2
    qb.refill_async(srcq)
    tb.refill_async(srct)
    ctx.upload_fence()
    sd2 = ctx.self_dist_batch([qb])[0]
    got, _, rec, fb = _ab(ctx, [(qb, tb), (q0, t0)], TAU)
    assert rec > 0 and fb == 0
    _same(got[0], _oracle(Q2, T2, sd2, TAU))
    assert len(got[0][0]) > 0
