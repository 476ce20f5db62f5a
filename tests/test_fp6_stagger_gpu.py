"""GPU: the FP6 filter sweep's loop order and its records (filter6.hip).  The cases were laid out for a loop in which waves
4 - 7 of a workgroup run a unit's epilogue half a unit late and carry a stage's last sums across the hand-over (measured
slower and not shipped: DESIGN.md, K12); they hold for any order of the loop: every (wave, unit) must meet exactly one
epilogue, and a record must carry the unit's own number and the lane half that fired, because the rescoring reads only that
half's 16 streamed rows.  The results must be, byte for byte, what K1 reports (option "fp6_filter" 0) and what the oracle
reports, and "fp6_records" must count every firing (lane, unit).  Train rows are the sweep's output rows, query rows the
streamed ones.  Every batch has two pairs: a lone small pair is planned in K1's 4-wave shape, which the filter leaves to K1."""
import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

TAU = 0.7
NQ = 1029           # 9 stages of 128 streamed rows = 33 units of 32; the last unit has 5 real rows (rows 0 - 3 in one lane half, 4 in the other)


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


@pytest.fixture(scope="module")
def dense():
    """Random bytes 45 .. 210, 1029 query x 1537 train rows, self distances 3000: D* = (0.7 * 3000)^2 = 4.41e6 is beyond every
    possible d2 (<= 128 * 165^2 = 3.48e6), so a lane with a real train row fires for every unit with a real query row, in both
    lane halves.  1537 train rows are two workgroups; in the second, waves 0 - 3 are full, wave 4 holds one row, waves 5 - 7 none."""
    rng = np.random.default_rng(41)
    Q = rng.integers(45, 211, (NQ, 128)).astype(np.uint8)
    T = rng.integers(45, 211, (1537, 128)).astype(np.uint8)
    sd = np.full(NQ, 3000.0)
    want = _oracle(Q, T, sd, TAU)
    assert len(want[0]) > 0
    return Q, T, sd, want


@pytest.mark.parametrize("nsplit", [1, 2, 4, 9])
def test_every_wave_and_unit_meets_one_epilogue(ctx, dense, nsplit):
    """The pair twice: exactly 2 x 1537 rows x 33 units x 2 halves = 202 884 records, no fallback.  "nsplit" 1, 2, 4 and 9 give
    9, 5 + 4, 3 and 1 stages per split: every remainder of the stage loop's unroll by three in front of the end-of-sweep
    epilogues of both wave halves.  A skipped or doubled epilogue, or one on sums that nothing wrote, changes the count."""
    Q, T, sd, want = dense
    qb, tb = _pair(ctx, Q, T, sd)
    got, rec, fb = _ab(ctx, [(qb, tb), (qb, tb)], TAU, nsplit=nsplit)
    print("nsplit", nsplit, "fp6_records", rec, "fp6_fallbacks", fb)
    assert rec == 2 * 1537 * 33 * 2 == 202884 and fb == 0, (nsplit, rec, fb)
    _same(got[0], want)
    _same(got[1], want)


@pytest.fixture(scope="module")
def sparse():
    """The train bank holds noisy copies (|noise| <= 3 per byte: d2 <= 1152) of all 1029 query rows: the copy of row i < 1024 at
    train row 128 (i mod 8) + i div 8, so each wave of the first workgroup owns four copies from each of the 32 full units; the
    copies of rows 1024 - 1028 at rows 1024 - 1028 (the second workgroup owns the partial unit), then 20 random rows.  Self
    distances 450: D* = 99 225 against d2 ~ 590 000 of random rows, so exactly the copies are accepted."""
    rng = np.random.default_rng(43)
    Q = rng.integers(45, 211, (NQ, 128)).astype(np.uint8)
    src = np.empty(NQ, np.int64)                 # src[train row] = the query row it copies
    i = np.arange(1024)
    src[128 * (i % 8) + i // 8] = i
    src[1024:] = np.arange(1024, NQ)
    T = np.concatenate([np.clip(Q[src].astype(np.int64) + rng.integers(-3, 4, (NQ, 128)), 0, 255),
                        rng.integers(45, 211, (20, 128))]).astype(np.uint8)
    sd = np.full(NQ, 450.0)
    want = _oracle(Q, T, sd, TAU)
    assert np.array_equal(np.sort(want[0]), np.arange(NQ))
    assert np.array_equal(src[want[1]], want[0])
    return Q, T, sd, want


@pytest.mark.parametrize("options", [{}, {"nsplit": 9}], ids=["plan", "nsplit9"])
def test_sparse_hits_in_every_wave_from_every_unit(ctx, sparse, options):
    """All 1029 query rows are accepted, each with its copy: a wrong unit number in a deferred epilogue's record is a missing
    match.  Once at the plan's splits and once with every split a single stage."""
    Q, T, sd, want = sparse
    qb, tb = _pair(ctx, Q, T, sd)
    got, rec, fb = _ab(ctx, [(qb, tb), (qb, tb)], TAU, **options)
    print(options, "fp6_records", rec, "fp6_fallbacks", fb)
    assert rec >= NQ and fb == 0, (rec, fb)
    _same(got[0], want)
    _same(got[1], want)
    assert np.array_equal(np.sort(got[0][0]), np.arange(NQ))
