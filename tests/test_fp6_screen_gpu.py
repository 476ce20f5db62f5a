"""GPU: the FP6 sweep with zero accumulator starts (filter6.hip; fp6_filter.h; DESIGN.md section 4 K12, "Zero start").

The sweep screens a block's maximum against  thr - (largest start of the streamed STAGE)  and reads the rows' starts only
where a lane passes; the exact test on acc + start then decides as the sweep with starts in the C operand did.  So the
record set is that sweep's, and `_model_records` states its rule in NumPy -- code table, E_c, T_c, per-row starts, the lane
halves of the 32 x 32 tile -- so that "fp6_records" can be demanded to the record.  MEASURED once against the library of
the commit before this change: the 1 100 x 1 300 pair of test_record_model 396 records, with its 300-row bank 525; equal.

Train rows are the sweep's output rows c (banks of 300 and 1 100 rows), query rows the streamed rows m: 1 300 rows = 11
stages, so the ring of four stages' starts wraps twice, and the last stage has 20 real rows.  Every case runs through the
batched call under "fp6_nsplit" 1 (one workgroup sweeps all 11 stages) and 2 (6 + 5), must equal K1 (option "fp6_filter" 0)
and the oracle byte for byte with "fp6_fallbacks" 0, and must leave exactly the model's count in "fp6_records"."""
import numpy as np
import pytest

from fastmatch_amd import synth
from test_fp6_filter import GRID
from test_fp6_filter_gpu import TAU, _ab, _dstar, _oracle, _same

pytestmark = pytest.mark.gpu

NQ, NT, NT_SMALL = 1300, 1100, 300
S = 450.0                                   # every self distance: the cut is D* = _dstar(S, TAU), about 315^2
VAL = GRID[np.argmin(np.abs(GRID[None, :] - np.arange(256)[:, None]), axis=1)]
# register r of lane half h holds streamed row (r & 3) + 8 (r >> 2) + 4 h of the unit
HALF = np.array([[(r & 3) + 8 * (r >> 2) + 4 * h for r in range(16)] for h in range(2)])


def _stats(A):
    a, h = A.astype(np.int64), VAL[A]
    return (a * a).sum(1), (h * h).sum(1), ((a - h) ** 2).sum(1), h


def _thresholds(Q, T, D):
    """T_c of every output row in units of c^.m^ (fp6_threshold: float64, E_c rounded up, floored)."""
    uq, _, eq, _ = _stats(Q)
    uc, hc, ec, _ = _stats(T)
    E = np.sqrt(ec.astype(np.float64)) * np.sqrt(np.float64(uq.max())) + np.sqrt(hc.astype(np.float64)) * np.sqrt(np.float64(eq.max()))
    E = E * (1.0 + 1.0 / 1048576.0) + 1.0 / 1024.0
    return np.floor((uc.astype(np.float64) - float(D) + 1.0) * 0.5 - E).astype(np.int64)


def _fires(Q, T, D, starts=True):
    """[output row, streamed row]: acc >= T_c / 1024 with acc = c^.m^ / 1024 + start, in integers: one step of the
    accumulator is 16 units, |T_c| < 2^24 makes T_c / 1024 a float32.  starts=False: the accumulator without its start."""
    uq, _, _, hq = _stats(Q)
    _, _, _, hc = _stats(T)
    Tc = _thresholds(Q, T, D)
    assert np.abs(Tc).max() < 1 << 24
    dot = hc @ hq.T
    assert (dot % 16 == 0).all()
    steps = dot // 16 - ((uq >> 5)[None, :] if starts else 0)
    return 16 * steps >= Tc[:, None]


def _model_records(Q, T, D):
    """The records of a pair: one per (output row, 32-row unit, lane half) with a firing real streamed row among its 16."""
    f = _fires(Q, T, D)
    nq = f.shape[1]
    pad = np.zeros((f.shape[0], -nq % 32), bool)
    f = np.concatenate([f, pad], axis=1).reshape(f.shape[0], -1, 32)
    return int(sum(f[:, :, HALF[h]].any(axis=2).sum() for h in range(2)))


def _noisy(rng, row, amp):
    return np.clip(row.astype(np.int64) + rng.integers(-amp, amp + 1, 128), 0, 255).astype(np.uint8)


# (a) streamed rows in unit 3 of stages 0, 3, 4 and 9 -- the unit a wave carries across the hand-over and tests behind it,
# from ring slots 0, 3, 0 (after the wrap) and 1 -- on both lane halves, and in the 20 real rows of stage 10 (unit 3 of that
# stage is padding: it is the unit multiplied behind the loop)
CARRIED = [128 * st + 96 + r for st in (0, 3, 4, 9) for r in (2, 21)] + [1280 + 1, 1280 + 14]
CARRIED_TRAIN = [11 + 23 * k for k in range(len(CARRIED))]          # all below 300: both output banks hold them
LOW_TRAIN, ZERO_TRAIN, ZERO_QUERY = 37, 250, 1290


def _pair_a():
    """The 1 100 x 1 300 pair: planted copies all over, (a)'s copies in the carried units, and for (c) a zero row among the
    last stage's 20 real rows -- the stage's largest start is 0, so every block of that stage passes the screen, its padding
    rows at accumulator 0 included -- with two low-norm output rows whose thresholds are negative."""
    Q, T, _ = synth.planted_pair(NQ, NT, seed=311)
    rng = np.random.default_rng(312)
    for q, t in zip(CARRIED, CARRIED_TRAIN):
        Q[q] = _noisy(rng, T[t], 6)
    T[LOW_TRAIN] = rng.integers(0, 4, 128)
    T[ZERO_TRAIN] = 0
    Q[ZERO_QUERY] = 0
    return Q, T


class Pair(object):
    def __init__(self, ctx, Q, T, qb=None, tb=None):
        self.Q, self.T = Q, T
        self.sd = np.full(len(Q), S)
        self.D = _dstar(S, TAU)
        self.qb = ctx.bank(Q) if qb is None else qb
        self.tb = ctx.bank(T) if tb is None else tb
        self.qb.set_selfdist(self.sd)
        self.want = _oracle(Q, T, self.sd, TAU)
        self.records = _model_records(Q, T, self.D)


def _run(ctx, pairs, nsplits=(1, 2)):
    """The pairs in one launch under every split count: the filter equals K1 (_ab) and the oracle, keeps its pairs itself
    and leaves the model's number of records."""
    keep = ctx.get_option("fp6_nsplit")
    try:
        for ns in nsplits:
            ctx.set_option("fp6_nsplit", ns)
            got, _, rec, fb = _ab(ctx, [(p.qb, p.tb) for p in pairs], TAU)
            print("fp6_nsplit", ns, "fp6_records", rec, "model", [p.records for p in pairs], "fp6_fallbacks", fb)
            for p, g in zip(pairs, got):
                _same(g, p.want)
            assert fb == 0
            assert rec == sum(p.records for p in pairs), (ns, rec, [p.records for p in pairs])
    finally:
        ctx.set_option("fp6_nsplit", keep)
    return got


@pytest.fixture(scope="module")
def pair_a(ctx):
    Q, T = _pair_a()
    big = Pair(ctx, Q, T)
    return big, Pair(ctx, Q, T[:NT_SMALL].copy(), qb=big.qb)


def test_record_model(ctx, pair_a):
    """(e) The seeded 1 100 x 1 300 pair, and its first 300 output rows as a bank of their own against the same streamed bank:
    the record counts are the model's (the module's docstring has the figures measured on the library before the change)."""
    big, small = pair_a
    assert 100 < small.records < big.records < 1000
    _run(ctx, [big, small])
    _run(ctx, [small, big], nsplits=(2,))


def test_carried_units(ctx, pair_a):
    """(a) Every copy planted in a carried unit is accepted with its train row, under both output banks."""
    big, small = pair_a
    for p in (big, small):
        q, t = p.want[0].tolist(), p.want[1].tolist()
        for cq, ct in zip(CARRIED, CARRIED_TRAIN):
            assert cq in q and t[q.index(cq)] == ct, (cq, ct)
    got = _run(ctx, [big, small])
    for g in got:
        assert set(CARRIED) <= set(g[0].tolist())


def test_padding_of_the_last_stage(ctx, pair_a):
    """(c) The low-norm output rows have negative thresholds, below the accumulator 0 of a padding row without its start;
    the last stage's largest start is 0 (the zero row), so there the screen is thr itself and every unit of that stage --
    real rows, padding rows, the all-padding unit behind the loop -- takes the exact test.  The only records these output
    rows may leave in the last stage are the zero row's: the model counts them, and the zero rows are matched."""
    big, small = pair_a
    Tc = _thresholds(big.Q, big.T, big.D)
    assert Tc[LOW_TRAIN] < 0 and Tc[ZERO_TRAIN] < 0
    f = _fires(big.Q, big.T, big.D)
    last = np.arange(1280, NQ)
    assert f[ZERO_TRAIN, last].tolist() == (last == ZERO_QUERY).tolist() and f[LOW_TRAIN, ZERO_QUERY]
    # without its start every row of the last stage passes the screen of these output rows, and of most others
    nostart = _fires(big.Q, big.T, big.D, starts=False)
    assert nostart[LOW_TRAIN, last].all() and nostart[ZERO_TRAIN, last].all() and nostart[:, last].any(axis=1).mean() > 0.9
    got = _run(ctx, [big, small])
    for g in got:
        q, t = g[0].tolist(), g[1].tolist()
        assert t[q.index(ZERO_QUERY)] == ZERO_TRAIN


def test_screen_fires_and_the_exact_test_rejects(ctx, pair_a):
    """(b) Independent banks: no output row has a candidate, the model counts no record.  Streamed row 700 (stage 5) is all
    zero, so that stage's largest start is 0 and its screen is thr itself: the accumulators of ordinary rows, c^.m^ / 1024
    without the -|m|^2 / 2048, pass it for every output row in every unit of the stage, and every exact test fails -- the zero
    row's too, its accumulator 0 being below the positive thresholds.  The pair leaves NO record and no match."""
    Q, T, _ = synth.planted_pair(NQ, NT_SMALL, seed=321, p=0.0)
    Q[700] = 0
    p = Pair(ctx, Q, T)
    assert p.records == 0 and len(p.want[0]) == 0
    assert (_thresholds(Q, T, p.D) > 0).all()
    nostart = _fires(Q, T, p.D, starts=False)
    stage5 = nostart[:, 640:768].reshape(NT_SMALL, 4, 32)
    assert stage5.any(axis=2).all()                      # every (output row, unit) of the stage passes the screen
    # (a batch of one pair is planned as a single-pair call, which keeps banks of this size on K1; beside the large pair the
    # launch's count is that pair's own, which also shows that the filter ran)
    got = _run(ctx, [p, pair_a[0]])
    assert len(got[0][0]) == 0


def _refill(ctx, bank, rows, sd):
    src = ctx.pinned_empty(rows.shape, np.uint8)
    src[:] = rows
    bank.refill_async(src)
    ctx.upload_fence()
    bank.set_selfdist(sd)


@pytest.mark.parametrize("grid", [1, None])
def test_stage_maximum_after_a_refill(ctx, grid):
    """(d) The stage's largest start follows a refill ("refill_grid" workgroups prepare the bank; 1: one workgroup walks
    all stages).  Contents X: stage 2 holds a low-norm row that is a copy of a low-norm train row, stage 7 ordinary rows.
    Contents Y: the reverse.  X -> Y raises stage 7's maximum and lowers stage 2's, Y -> X the other way.  A maximum left
    over from ordinary rows (about -127) puts the screen of the low-norm copy's stage 127 above its threshold and loses the
    copy, whose accumulator without start is below 1; one left over from the low-norm row only makes a stage pass the
    screen for nothing.  X's copy sits in unit 3 of its stage, which is multiplied behind the next hand-over: screened
    against the NEXT stage's value (ordinary rows) it is lost in the same way.  Y's copy sits in unit 2."""
    keep = ctx.get_option("refill_grid")
    rng = np.random.default_rng(331)
    Q, T, _ = synth.planted_pair(NQ, NT_SMALL, seed=332)
    T[123] = rng.integers(0, 6, 128)
    low = _noisy(rng, T[123], 1)
    X, Y = Q.copy(), Q.copy()
    at_x, at_y = 2 * 128 + 96 + 5, 7 * 128 + 64 + 13
    X[at_x], Y[at_y] = low, low
    uq = _stats(X)[0]
    assert uq[at_x] < 32 * 64 and np.delete(uq, at_x).min() > 100 * 32 * 64
    try:
        if grid is not None:
            ctx.set_option("refill_grid", grid)
        p = Pair(ctx, X, T)
        other = Pair(ctx, *synth.planted_pair(NQ, NT, seed=333)[:2])
        for k, (rows, at) in enumerate(((X, at_x), (Y, at_y), (X, at_x), (Y, at_y))):
            if k > 0:
                _refill(ctx, p.qb, rows, p.sd)
                p = Pair(ctx, rows, T, qb=p.qb, tb=p.tb)
            q, t = p.want[0].tolist(), p.want[1].tolist()
            assert t[q.index(at)] == 123
            got = _run(ctx, [p, other])
            assert at in got[0][0].tolist()
    finally:
        ctx.set_option("refill_grid", keep)
