"""GPU: the FP6 filter sweep keeps a wave's hits in a private list in LDS (filter6.hip: kF6HitSlots records per wave) and
copies the list to the pair's list when it is full and when the wave's sweep ends.  The results must stay, byte for byte, what
K1 reports (option "fp6_filter" 0) and what the oracle reports, and "fp6_records" / "fp6_fallbacks" must count what they counted
when every hit went to the pair's list at once.  Train rows are the sweep's output rows, query rows the streamed ones.  Every
batch has two pairs: a lone small pair is planned in K1's 4-wave shape, which the filter leaves to K1."""
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


def _ab(ctx, pairs, tau, **options):
    """The batch under the filter and under K1, both with the given context options: (filter results, records, fallbacks)
    after asserting that the two are equal byte for byte."""
    keep = {k: ctx.get_option(k) for k in options}
    try:
        for k, v in options.items():
            ctx.set_option(k, v)
        ctx.set_option("fp6_filter", 1)
        got = _batch(ctx, pairs, tau)
        rec, fb = ctx.get_option("fp6_records"), ctx.get_option("fp6_fallbacks")
        ctx.set_option("fp6_filter", 0)
        want = _batch(ctx, pairs, tau)
    finally:
        ctx.set_option("fp6_filter", 1)
        for k, v in keep.items():
            ctx.set_option(k, v)
    for g, w in zip(got, want):
        _same(g, w)
    return got, rec, fb


def _pair(ctx, Q, T, sd):
    qb, tb = ctx.bank(Q), ctx.bank(T)
    qb.set_selfdist(sd)
    return qb, tb


def test_a_waves_list_overflows_many_times_while_the_pairs_list_holds(ctx):
    """Random bytes 45 .. 210, 700 query x 1537 train rows, caller self distances of 3000: the cut D* = (0.7 * 3000)^2 =
    4.41e6 is beyond every possible d2 (<= 128 * 165^2 = 3.48e6), so a lane that holds a real train row fires for every unit
    with a real query row, in both lane halves (the 28 real rows of the last unit reach either half's 16).  A wave then
    produces 128 rows x 22 units x 2 = 5 632 records against the 128 of its list, and the pair exactly
    1537 x ceil(700 / 32) x 2 = 67 628, in whatever order.  A planted pair rides in the same batch; its own record count comes
    from a batch of two of it ("fp6_records" is the sum over a launch's pairs).  With "fp6_cap" at the big pair's count its
    list is exactly full and nothing falls back; with one less the pair goes to K1, and the sweep's count stays what it was."""
    rng = np.random.default_rng(23)
    nq, nt = 700, 1537
    Q = rng.integers(45, 211, (nq, 128)).astype(np.uint8)
    T = rng.integers(45, 211, (nt, 128)).astype(np.uint8)
    sd = np.full(nq, 3000.0)
    qb, tb = _pair(ctx, Q, T, sd)
    want = _oracle(Q, T, sd, TAU)
    assert len(want[0]) > 0
    Q2, T2, _ = synth.planted_pair(300, 257, seed=100)
    q2 = ctx.bank(Q2)
    sd2 = ctx.self_dist(q2)
    q2.set_selfdist(sd2)
    t2 = ctx.bank(T2)
    want2 = _oracle(Q2, T2, sd2, TAU)
    assert len(want2[0]) > 0

    _, rec22, fb = _ab(ctx, [(q2, t2), (q2, t2)], TAU)
    assert rec22 > 0 and rec22 % 2 == 0 and fb == 0, (rec22, fb)
    small = rec22 // 2
    big = nt * ((nq + 31) // 32) * 2
    assert big == 67628 and small < big

    for cap, falls_back in ((None, False), (big, False), (big - 1, True)):
        got, rec, fb = _ab(ctx, [(qb, tb), (q2, t2)], TAU, **({} if cap is None else {"fp6_cap": cap}))
        print("fp6_cap", cap, "fp6_records", rec, "fp6_fallbacks", fb)
        assert rec == big + small, (cap, rec, big, small)
        assert (fb >= 1) if falls_back else (fb == 0), (cap, fb)
        _same(got[0], want)
        _same(got[1], want2)


def _ends_pair(rng, nq, units, extra=20):
    """A query bank of random rows and a train bank whose first rows are noisy copies (|noise| <= 3 per byte: d2 <= 1152)
    of every real query row of the given 32-row units, followed by `extra` random rows: (Q, T, the copied query rows)."""
    Q = rng.integers(45, 211, (nq, 128)).astype(np.uint8)
    src = np.concatenate([np.arange(32 * u, min(32 * u + 32, nq)) for u in units])
    src = rng.permutation(src)
    T = np.concatenate([np.clip(Q[src].astype(np.int64) + rng.integers(-3, 4, (len(src), 128)), 0, 255),
                        rng.integers(45, 211, (extra, 128))]).astype(np.uint8)
    return Q, T, src


def test_hits_only_where_the_pipelines_ends_are(ctx):
    """A query bank of 128 * 40 + 5 rows: 41 stages, the last one with 5 real rows in its first unit.  Copies of query rows
    sit only in the first unit of the first stage (multiplied first behind the first hand-over), in the last partial unit, and
    in the last unit of every split but the last (the last split ends in padding): the unit that a wave carries in registers
    across the next hand-over.  Once with the plan's splits -- one 512-row piece of train rows and at least 8 stages per
    split: 41 / 8 = 5 splits of 9 stages -- and once with "nsplit" 41, every split a single stage, where every stage's last
    unit is such an end.  The self distances are 450: D* = 99 225 against d2 ~ 590 000 of random rows, so exactly the copies are
    accepted; all of them leave the sweep through the flush at its end."""
    rng = np.random.default_rng(29)
    nstages, nq = 41, 128 * 40 + 5
    sd = np.full(nq, 450.0)
    Q2, T2, _ = synth.planted_pair(300, 257, seed=100)
    q2 = ctx.bank(Q2)
    sd2 = ctx.self_dist(q2)
    q2.set_selfdist(sd2)
    t2 = ctx.bank(T2)
    want2 = _oracle(Q2, T2, sd2, TAU)
    per = -(-nstages // (nstages // 8))
    plan_ends = [4 * st1 - 1 for st1 in range(per, nstages, per)]
    stage_ends = [4 * st1 - 1 for st1 in range(1, nstages)]
    assert plan_ends == [35, 71, 107, 143] and set(plan_ends) <= set(stage_ends)
    for ends, options in ((plan_ends, {}), (stage_ends, {"nsplit": nstages})):
        Q, T, src = _ends_pair(rng, nq, [0] + ends + [4 * (nstages - 1)])
        assert len(src) == 32 * (1 + len(ends)) + 5
        qb, tb = _pair(ctx, Q, T, sd)
        want = _oracle(Q, T, sd, TAU)
        assert np.array_equal(np.sort(want[0]), np.sort(src))
        got, rec, fb = _ab(ctx, [(qb, tb), (q2, t2)], TAU, **options)
        print(options, "fp6_records", rec, "fp6_fallbacks", fb)
        assert rec >= len(src) and fb == 0, (rec, fb)
        _same(got[0], want)
        _same(got[1], want2)
        assert np.array_equal(np.sort(got[0][0]), np.sort(src))
