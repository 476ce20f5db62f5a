"""GPU: the FP6 sweep with the max trees rotated into the next half's matrix instructions (filter6.hip; DESIGN.md section 4
K12, "Rotated epilogue").

A unit's blocks 0, 1 are tested half a unit behind their instructions and its blocks 2, 3 a whole half later, inside the NEXT
unit -- for the unit carried across a hand-over that is the second multiply of the next stage, for a workgroup's last unit
a drain behind the loop.  What can go wrong is timing: the stage's screen value thr_s per block pair, the ring slot and the
unit number of a hit found one multiply late, accumulator presets that fire, a flush of the wave's list between matrix
instructions in flight.  None of it changes WHICH records the sweep leaves, so every case here holds for a sweep that tests
all four blocks behind their unit as well.

The record model and the shapes are those of test_fp6_screen_gpu.py (1 300 streamed rows = 11 stages, the ring wraps twice,
20 real rows in the last stage; output banks of 300 and 1 100 rows), with "fp6_nsplit" 1, 2, 3 and 11: a workgroup sweeps
11 / 6, 5 / 4, 4, 3 stages -- every residue of the loop's unrolling by three -- or a single stage, the fewest there are.  Every
case demands, through _run: results byte-identical to K1 ("fp6_filter" 0) and to the oracle, "fp6_records" equal to the
model, "fp6_fallbacks" 0; and here, on the CPU, that the model's count is below "fp6_cap", so that K1 is never asked to
redo a pair that lost a record.

Screened is the model WITH the screen: a record needs its lane's exact test and a lane of its block (32 output rows, both
halves) that passes thr - smax of the stage the kernel holds at that time.  With the right stage it is _model_records to the
record; with blocks 2, 3 of a carried unit held against the next stage, or blocks 0, 1 of a stage's first unit against the
stage before, it loses records of case (a) -- asserted, so that the case cannot pass for nothing.

Case (b) needs real rows in the last unit of the streamed bank, which 1 300 rows do not have: it streams 1 408 rows, 11 full
stages."""
import numpy as np
import pytest

from fastmatch_amd import synth
from test_fp6_screen_gpu import HALF, NQ, NT, NT_SMALL, Pair, _fires, _noisy, _refill, _run, _stats, _thresholds

pytestmark = pytest.mark.gpu

NSPLITS = (1, 2, 3, 11)
NSTAGES = 11
NQ_FULL = 128 * NSTAGES


def _per(nsplit):
    """Stages per split under a forced count (fp6_plan_split_forced)."""
    return -(-NSTAGES // min(nsplit, NSTAGES))


def test_split_counts_cover_the_unrolled_loop():
    counts = {ns: [min(_per(ns), NSTAGES - s) for s in range(0, NSTAGES, _per(ns))] for ns in NSPLITS}
    assert counts[1] == [11] and counts[2] == [6, 5] and counts[3] == [4, 4, 3] and counts[11] == [1] * 11
    assert {c % 3 for v in counts.values() for c in v} == {0, 1, 2}


def _fire_cube(Q, T, D):
    """[output row, unit, half]: the lane's exact test (a real streamed row among its 16 fires)."""
    f = _fires(Q, T, D)
    f = np.concatenate([f, np.zeros((f.shape[0], -f.shape[1] % 32), bool)], axis=1).reshape(f.shape[0], -1, 32)
    return np.stack([f[:, :, HALF[h]].any(axis=2) for h in range(2)], axis=2)


def _round_down32(x):
    f = x.astype(np.float32)
    return np.where(f.astype(np.float64) > x, np.nextafter(f, np.float32(-np.inf)), f).astype(np.float64)


class Screened(object):
    """The sweep's records [output row, unit, half] WITH the screen in front of the exact test: a block is screened against
    thr - smax(stage), rounded down to a float32.  records(nsplit) holds every unit against its own stage;
    "late23" holds blocks 2, 3 of a carried unit (unit 3 of a stage that is not its split's last) against the NEXT stage,
    "early01" blocks 0, 1 of unit 0 of a stage that is not its split's first against the stage BEFORE."""
    def __init__(self, Q, T, D):
        uq, _, _, hq = _stats(Q)
        _, _, _, hc = _stats(T)
        nq, self.nt = len(Q), len(T)
        self.nst = nst = -(-nq // 128)
        Tc = _thresholds(Q, T, D)
        self.thr = Tc.astype(np.float64) / 1024.0                            # exact in float32: |T_c| < 2^24
        assert np.array_equal(self.thr, self.thr.astype(np.float32).astype(np.float64))
        start = np.full(nst * 128, -3.4e38)
        start[:nq] = -(uq >> 5).astype(np.float64) / 64.0
        self.smax = start.reshape(nst, 128).max(axis=1)
        acc = np.zeros((self.nt, nst * 128))                                 # padding rows: zero codes
        acc[:, :nq] = (hc.astype(np.float64) @ hq.T.astype(np.float64)) / 1024.0       # (exact: integers below 2^53)
        self.acc = acc.reshape(self.nt, nst * 4, 32).max(axis=2)             # [output row, unit]: the best lane of both halves
        fire = _fire_cube(Q, T, D)
        self.fire = np.concatenate([fire, np.zeros((self.nt, nst * 4 - fire.shape[1], 2), bool)], axis=1)

    def records(self, nsplit, variant="right"):
        nst, nt = self.nst, self.nt
        per = -(-nst // min(nsplit, nst))
        group = np.arange(nt) // 32
        block = group % 4
        out = np.zeros_like(self.fire)
        for u in range(nst * 4):
            st = u // 4
            held = np.full(nt, st)
            if variant == "late23" and u % 4 == 3 and (st + 1) % per != 0 and st + 1 < nst:
                held[block >= 2] = st + 1
            if variant == "early01" and u % 4 == 0 and st % per != 0:
                held[block < 2] = st - 1
            lane_pass = self.acc[:, u] >= _round_down32(self.thr - self.smax[held])
            block_pass = np.zeros(group.max() + 1, bool)
            np.logical_or.at(block_pass, group, lane_pass)
            out[:, u, :] = self.fire[:, u, :] & block_pass[group][:, None]
        return out


def _check_cap(ctx, *pairs):
    cap = ctx.get_option("fp6_cap")
    for p in pairs:
        assert p.records < cap, (p.records, cap)


# ---------------------------------------------------------------------------------------------------------------------
# (a) every block of every wave, both lane halves, in carried units and in the units behind them

UNITS_A = [(0, 3), (1, 0), (3, 3), (4, 0), (4, 3), (5, 0), (9, 3), (10, 0)]             # (stage, unit)
LOW_23, LOW_01 = 32 * 3 + 20, 32 * 4 + 20                                                # output rows of blocks 3 and 0, wave 0
AT_23, AT_01 = 2 * 128 + 96 + 5, 7 * 128 + 9                                             # unit 3 of stage 2, unit 0 of stage 7


def _pair_a():
    Q, T, _ = synth.planted_pair(NQ, NT, seed=411)
    rng = np.random.default_rng(412)
    planted = []
    for g in range(-(-NT // 32)):                      # 35 groups of 32 output rows: 8 waves x 4 blocks, and 3 of the next chunk
        t = 32 * g + (7 * g + 3) % 12
        st, u = UNITS_A[g % len(UNITS_A)]
        for h in range(2):
            i = g // len(UNITS_A)
            q = 128 * st + 32 * u + (i & 3) + 8 * (i >> 2) + 4 * h
            Q[q] = _noisy(rng, T[t], 6)
            planted.append((q, t))
    # low-norm output rows, and a copy of each alone in its stage: that stage's largest start is near 0, its neighbours' near
    # -127.  LOW_23's copy sits in a carried unit (the stage behind it is ordinary), LOW_01's in the first unit of a stage
    # behind an ordinary one.
    T[LOW_23] = rng.integers(0, 6, 128)
    T[LOW_01] = rng.integers(0, 6, 128)
    Q[AT_23] = _noisy(rng, T[LOW_23], 1)
    Q[AT_01] = _noisy(rng, T[LOW_01], 1)
    return Q, T, planted


@pytest.fixture(scope="module")
def pair_a(ctx):
    Q, T, planted = _pair_a()
    big = Pair(ctx, Q, T)
    return big, Pair(ctx, Q, T[:NT_SMALL].copy(), qb=big.qb), planted


def test_every_block_in_carried_units_and_behind_them(ctx, pair_a):
    big, small, planted = pair_a
    _check_cap(ctx, big, small)
    assert {(t // 32) % 4 for _, t in planted} == {0, 1, 2, 3} and {(t % 1024) // 128 for _, t in planted} == set(range(8))
    fire = _fire_cube(big.Q, big.T, big.D)
    for q, t in planted:                               # every copy is a record of its lane half
        assert fire[t, q // 32, (q % 32 >> 2) & 1], (q, t)
    want_q, want_t = big.want[0].tolist(), big.want[1].tolist()
    for q, t in [(AT_23, LOW_23), (AT_01, LOW_01)]:    # (the low-norm copies are accepted matches as well)
        assert q in want_q and want_t[want_q.index(q)] == t, (q, t)
    uq = _stats(big.Q)[0]
    assert uq[AT_23] < 32 * 64 and uq[AT_01] < 32 * 64 and np.delete(uq, [AT_23, AT_01]).min() > 100 * 32 * 64
    for p in (big, small):
        m = Screened(p.Q, p.T, p.D)
        for ns in NSPLITS:
            right = m.records(ns)
            assert int(right.sum()) == p.records
            late, early = m.records(ns, "late23"), m.records(ns, "early01")
            if ns < NSTAGES:                           # (a workgroup of one stage carries no unit)
                assert right[LOW_23, AT_23 // 32].any() and not late[LOW_23, AT_23 // 32].any(), ns
                assert right[LOW_01, AT_01 // 32].any() and not early[LOW_01, AT_01 // 32].any(), ns
                assert late.sum() < right.sum() and early.sum() < right.sum()
    got = _run(ctx, [big, small], nsplits=NSPLITS)
    for g in got:
        assert {AT_23, AT_01} <= set(g[0].tolist())
    _run(ctx, [small, big], nsplits=(3,))


# ---------------------------------------------------------------------------------------------------------------------
# (b) the drain

def _pair_b(stages, seed):
    """Independent banks (no record), then copies of output rows of blocks 2 and 3 -- waves 0, 1 and, by its first rows, 2 --
    in unit 3 of the given stages, both lane halves."""
    Q, T, _ = synth.planted_pair(NQ_FULL, NT_SMALL, seed=seed, p=0.0)
    rng = np.random.default_rng(seed + 1)
    rows = [64 + 9, 96 + 30, 128 + 64 + 1, 128 + 96 + 17]
    for i, st in enumerate(stages):
        for t, r in zip(rows, (0, 7, 10, 13)):          # (rows 0 .. 3 and 8 .. 11 of a unit are lane half 0)
            Q[128 * st + 96 + r] = _noisy(rng, T[t + i], 6)
    return Q, T


@pytest.mark.parametrize("nsplit", [1, 2])
def test_hits_only_in_the_drain(ctx, pair_a, nsplit):
    per = _per(nsplit)
    last = [min(s + per, NSTAGES) - 1 for s in range(0, NSTAGES, per)]
    assert last == ([10] if nsplit == 1 else [5, 10])
    p = Pair(ctx, *_pair_b(last, 421 + 10 * nsplit))
    _check_cap(ctx, p, pair_a[0])
    c, u, h = np.nonzero(_fire_cube(p.Q, p.T, p.D))
    assert len(c) >= 4 * len(last) and set((c // 32 % 4).tolist()) == {2, 3} and set(u.tolist()) == {4 * s + 3 for s in last}
    assert set(h.tolist()) == {0, 1}
    got = _run(ctx, [p, pair_a[0]], nsplits=(nsplit,))
    assert len(got[0][0]) == 4 * len(last)


# ---------------------------------------------------------------------------------------------------------------------
# (c) the lowest thresholds there are, in blocks 2, 3 of every wave

def test_zero_output_rows_in_blocks_2_and_3(ctx):
    """An all-zero output row has T_c = (1 - D*) / 2 - E_c with E_c next to nothing: no row's threshold is lower, and it sits
    below every accumulator without its start (>= 0).  In stages whose largest start is above that threshold -- those with a
    zero or low-norm streamed row -- these blocks pass the screen in every unit, padding units included; the records they
    may leave are those of the model.  Accumulator presets that fire, or a first test against anything but "never", leave
    more."""
    Q, T, _ = synth.planted_pair(NQ, NT, seed=431)
    rng = np.random.default_rng(432)
    zero_rows = [128 * w + 32 * j + (5 * w + 11 * j) % 32 for w in range(9) for j in (2, 3) if 128 * w + 32 * j + 32 <= NT]
    assert len(zero_rows) == 16
    T[zero_rows] = 0
    Q[3] = 0                                            # the first unit a workgroup multiplies behind its priming
    Q[128 * 4 + 96 + 31] = rng.integers(0, 3, 128)      # a carried unit
    Q[1290] = 0                                         # the last stage: 20 real rows, then padding
    p = Pair(ctx, Q, T)
    small = Pair(ctx, Q, T[:NT_SMALL].copy(), qb=p.qb)
    _check_cap(ctx, p, small)
    Tc = _thresholds(Q, T, p.D)
    assert (Tc[zero_rows] == Tc.min()).all() and Tc.min() < 0
    nostart = _fires(Q, T, p.D, starts=False)
    assert nostart[zero_rows].all()
    f = _fires(Q, T, p.D)
    assert f[zero_rows][:, [3, 128 * 4 + 96 + 31, 1290]].all() and f[zero_rows].sum() == 3 * len(zero_rows)
    m = Screened(Q, T, p.D)
    for ns in NSPLITS:
        assert int(m.records(ns).sum()) == p.records
    _run(ctx, [p, small], nsplits=NSPLITS)


# ---------------------------------------------------------------------------------------------------------------------
# (d) a wave's list fills from blocks 2, 3

def test_list_fills_from_a_late_block(ctx, pair_a):
    """Output rows 70 (block 2 of wave 0) and 100 (block 3) are near copies of each other, and two rows of every unit of the
    streamed bank, one per lane half, are near copies of them: 2 x 41 x 2 = 164 records of wave 0 and no other of that
    workgroup, so under one split the wave's list of 128 fills -- and is flushed -- at a hit of block 2 or 3."""
    Q, T, _ = synth.planted_pair(NQ, NT_SMALL, seed=441, p=0.0)
    rng = np.random.default_rng(442)
    T[100] = _noisy(rng, T[70], 1)
    for u in range(-(-NQ // 32)):
        for h in range(2):
            q = 32 * u + (3 * u + 1) % 4 + 8 * (u % 2) + 4 * h
            assert q < NQ
            Q[q] = _noisy(rng, T[70], 3)
    p = Pair(ctx, Q, T)
    _check_cap(ctx, p, pair_a[0])
    fire = _fire_cube(Q, T, p.D)
    c = np.nonzero(fire)[0]
    assert set(c.tolist()) == {70, 100} and fire[70].all() and fire[100].all() and p.records == 164 > 128
    _run(ctx, [p, pair_a[0]], nsplits=(1, 2))


# ---------------------------------------------------------------------------------------------------------------------
# (e) a refill moves a stage's maximum both ways

def test_refill_moves_the_stage_maximum(ctx):
    """test_fp6_screen_gpu's refill case with both copies where the rotation tests them late: output row 123 is block 3 of
    wave 0.  Contents X: its low-norm copy in unit 3 of stage 1, carried into stage 2 (ordinary rows).  Contents Y: in unit 3
    of stage 9, carried into stage 10.  X -> Y -> X lowers and raises both stages' largest start; thr_s[2], thr_s[3] moved
    to the next stage's value in front of the carried unit's late test lose the copy (in these two units no other row of
    the block passes the wrong screen and has the block tested all the same: the model says so below)."""
    rng = np.random.default_rng(451)
    Q, T, _ = synth.planted_pair(NQ, NT_SMALL, seed=452)
    T[123] = rng.integers(0, 6, 128)
    low = _noisy(rng, T[123], 1)
    X, Y = Q.copy(), Q.copy()
    at_x, at_y = 1 * 128 + 96 + 5, 9 * 128 + 96 + 5
    X[at_x], Y[at_y] = low, low
    p = Pair(ctx, X, T)
    other = Pair(ctx, *synth.planted_pair(NQ, NT, seed=453)[:2])
    _check_cap(ctx, p, other)
    for k, (rows, at) in enumerate(((X, at_x), (Y, at_y), (X, at_x))):
        if k > 0:
            _refill(ctx, p.qb, rows, p.sd)
            p = Pair(ctx, rows, T, qb=p.qb, tb=p.tb)
        q, t = p.want[0].tolist(), p.want[1].tolist()
        assert t[q.index(at)] == 123
        m = Screened(rows, T, p.D)
        for ns in (1, 3):
            right = m.records(ns)
            assert int(right.sum()) == p.records
            assert right[123, at // 32].any() and not m.records(ns, "late23")[123, at // 32].any()
        got = _run(ctx, [p, other], nsplits=(1, 3))
        assert at in got[0][0].tolist()
