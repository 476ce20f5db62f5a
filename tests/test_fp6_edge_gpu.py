"""GPU: the FP6 filter's threshold at equality (filter6.hip's prologue; fp6_filter.h).

Constant rows of a byte that rounds down to its e2m3 image make Cauchy-Schwarz an equality: the image's dot product loses
exactly E_c, and with the cut at D* = d2 + 1 the pair clears its threshold by one unit of c^.m^, 1/16 of an accumulator
step (tests/test_fp6_filter.py measures it on the host).  A threshold computed from the wrong bank's max6 words or from
smaller maxima left over from before a refill loses the pair, and the accepted match with it.  (|m|^2 of a constant row is
a multiple of 32: the start value's rounding direction is pinned by the host test alone.  The stat6 columns have a family of
their own, the last one below.)

Train rows are the sweep's output rows c, query rows the streamed rows m.  Per bank pair one family (c byte, m byte):
1 100 train rows (two 512-row pieces and a partial one: all 8 waves of the first workgroup, one wave of the second) and
300 query rows (two stages and 44 rows: a partial last stage and unit).  The copies of c sit on every wave of a workgroup,
on all four 32-row blocks of a wave, on the first and last row of a 512-row piece and on the last real row; the copies of
m on every position of a 32-row unit (both lane halves), in the first unit, in the units carried across the two
hand-overs and in the last partial unit.  Every family starts its copies at another of these places, because the
cross-check's tie rule accepts one match per bank pair: lowest query copy, lowest train copy.

Backgrounds (uniform bytes), checked in NumPy in front of the call -- the planted m attains the query bank's largest |m|^2
and |m - m^|^2, every background row is farther from the planted row of the other bank than its partner is, and no two
background rows are within the cut:
  136 / 152   query 0 .. 40, train 216 .. 255; the query background is beyond d2 + 2 E_c from c
  136 / 168   query 0 .. 40, train 232 .. 255; beyond d2 + 2 E_c
  200 / 232   query 0 .. 40, train 100 .. 140; beyond d2 + 2 E_c
  136 / 255   query 0 .. 6, train 130 .. 135.  d2 + 2 E_c = 2.8 M is more than any row's distance from a row of 136s, so the
              background is beyond d2 only: the filter may list it, the rescoring drops it
   36 / 255   a row of 255s is the farthest row there is from a row of 36s: EVERY query row is a copy of m; train 0 .. 30
  255 / 36    likewise every train row is a copy of c; query 0, 4 .. 32 (grid values: m = 36 is one, its error is 0)
  233 / 36    query 0, 4 .. 32, train 236 .. 255 (the row that rounds up; beyond d2 only)
All self distances of a query bank are one constant S with ratio_cut_d2(S, TAU) = d2 + 1, found on the host."""
import numpy as np
import pytest

from fastmatch_amd import sharding
from test_fp6_filter import GRID
from test_fp6_filter_gpu import TAU, _ab, _dstar, _oracle, _same

pytestmark = pytest.mark.gpu

NT, NQ = 1100, 300
# wave 0: its four blocks; waves 1 .. 7: block w % 4; the ends of the 512-row pieces; the second workgroup; the last real row
C_ROWS = sorted([0, 39, 84, 127] + [128 * w + 32 * (w % 4) + (5 * w) % 32 for w in range(1, 8)] + [511, 512, 1023, 1024, NT - 1])
# the first unit; all of unit 1; the last unit of stages 0 and 1 (multiplied behind a hand-over); the partial unit 288 .. 299
M_ROWS = sorted([0, 5, 31] + list(range(32, 64)) + [96, 101, 127] + [230, 255] + [288, 293, NQ - 1])
# the e2m3 image of a byte, x 32 (the lower of two equally near grid values)
VAL = GRID[np.argmin(np.abs(GRID[None, :] - np.arange(256)[:, None]), axis=1)]

# c byte, m byte, query background (lo, hi, step) or None, train background (lo, hi) or None, first c copy, first m copy,
# query background beyond d2 + 2 E_c
FAMILIES = [
    (136, 152, (0, 41, 1), (216, 256), 0, 0, True),
    (136, 168, (0, 41, 1), (232, 256), 39, 5, True),
    (200, 232, (0, 41, 1), (100, 141), 511, 31, True),
    (136, 255, (0, 7, 1), (130, 136), 1023, 96, False),
    (36, 255, None, (0, 31), 1024, 0, False),
    (255, 36, (0, 33, 4), None, 0, 293, False),
    (233, 36, (0, 33, 4), (236, 256), 84, 101, False),       # (not on the threshold: test_a_row_that_rounds_up)
]


def _sq(a):
    a = np.asarray(a, np.int64)
    return (a * a).sum(-1)


def _find_S(D):
    """A self distance S with ratio_cut_d2(S, TAU) == D: from sqrtf(D) / TAU, nudged one float64 at a time."""
    S = float(np.sqrt(np.float32(D))) / TAU
    for _ in range(64):
        got = _dstar(S, TAU)
        if got == D:
            return S
        S = float(np.nextafter(S, 0.0 if got > D else np.inf))       # (a smaller S fails earlier: a smaller D*)
    raise AssertionError("no self distance gives the cut %d" % D)


def _rows(k, mrow=None):
    """Family k's query rows, train rows, copy rows and d2, checked as the module's docstring says.  `mrow`: an edited
    row in the planted m's place."""
    cb, mb, qbg, tbg, c_from, m_from, far = FAMILIES[k]
    rng = np.random.default_rng(700 + k)
    c = np.full(128, cb, np.uint8)
    m = np.full(128, mb, np.uint8) if mrow is None else np.asarray(mrow, np.uint8)
    crows = [r for r in C_ROWS if r >= c_from] if tbg else list(range(NT))
    mrows = [r for r in M_ROWS if r >= m_from] if qbg else list(range(NQ))
    Q = np.empty((NQ, 128), np.uint8)
    T = np.empty((NT, 128), np.uint8)
    if qbg:
        Q[:] = rng.choice(np.arange(*qbg), (NQ, 128))
    if tbg:
        T[:] = rng.integers(tbg[0], tbg[1], (NT, 128))
    Q[mrows], T[crows] = m, c
    d2 = int(_sq(c.astype(np.int64) - m))
    isc, ism = np.zeros(NT, bool), np.zeros(NQ, bool)
    isc[crows], ism[mrows] = True, True
    um, em = _sq(Q), _sq(Q.astype(np.int64) - VAL[Q])
    assert um[mrows[0]] == um.max() and em[mrows[0]] == em.max()
    assert (um[~ism] < um.max()).all() and (em[~ism] <= em.max()).all()
    E = np.sqrt(float(_sq(c.astype(np.int64) - VAL[c]))) * np.sqrt(float(um.max())) + np.sqrt(float(_sq(VAL[c]))) * np.sqrt(float(em.max()))
    dq = _sq(Q[~ism].astype(np.int64) - c)
    assert (dq > (d2 + 2 * E if far else d2)).all()
    assert (_sq(T[~isc].astype(np.int64) - m) > d2).all()
    if qbg and tbg:
        qq, tt = Q[~ism].astype(np.int64), T[~isc].astype(np.int64)
        bg = _sq(qq)[:, None] + _sq(tt)[None, :] - 2 * qq @ tt.T
        assert bg.min() > d2 + 1
    return Q, T, crows, mrows, d2


class Family(object):
    def __init__(self, ctx, k, D=None, mrow=None, tb=None):
        """Family k in banks of its own, the query bank's self distances all S with D* = D (default: d2 + 1)."""
        self.Q, self.T, self.crows, self.mrows, self.d2 = _rows(k, mrow)
        self.D = self.d2 + 1 if D is None else D
        self.S = _find_S(self.D)
        assert _dstar(self.S, TAU) == self.D
        self.sd = np.full(NQ, self.S)
        self.qb = ctx.bank(self.Q)
        self.tb = ctx.bank(self.T) if tb is None else tb
        self.qb.set_selfdist(self.sd)
        self.want = _oracle(self.Q, self.T, self.sd, TAU)
        self.check_oracle()

    def check_oracle(self):
        """Exactly one match, lowest query copy with lowest train copy, iff d2 < D*."""
        q, t, d, _ = self.want
        if self.d2 < self.D:
            assert q.tolist() == [self.mrows[0]] and t.tolist() == [self.crows[0]]
            assert d[0] == np.sqrt(np.float32(self.d2))
        else:
            assert len(q) == 0

    def check(self, got):
        _same(got, self.want)


@pytest.fixture(scope="module")
def families(ctx):
    return [Family(ctx, k) for k in range(len(FAMILIES))]


def _run(ctx, fams):
    """The families in one launch under the filter and under K1: equal to each other and to the oracle, kept by the filter
    itself (no K1 redo), with at least one record per copy of c."""
    got, _, rec, fb = _ab(ctx, [(f.qb, f.tb) for f in fams], TAU)
    for f, g in zip(fams, got):
        f.check(g)
    assert fb == 0
    assert rec >= sum(len(f.crows) for f in fams if f.d2 < f.D), rec
    return got, rec


def test_six_families_in_one_launch(ctx, families):
    """The six constant pairs of the first table, one per bank pair, every one at its own cut D* = d2 + 1."""
    assert [f.d2 for f in families[:6]] == [32768, 131072, 131072, 1812608, 6139008, 6139008]
    got, _ = _run(ctx, families[:6])
    assert all(len(g[0]) == 1 for g in got)


def test_asymmetric_pair_in_both_directions(ctx, families):
    """36 against 255 and 255 against 36 in one batch: with the OUTPUT bank's max6 in the threshold the first is lost and the
    second kept (the host test's sharpness assertion), with the two banks' words exchanged between the pairs likewise."""
    got, _ = _run(ctx, families[4:6])
    assert got[0][0].tolist() == [0] and got[0][1].tolist() == [1024]
    assert got[1][0].tolist() == [293] and got[1][1].tolist() == [0]
    got, _ = _run(ctx, families[5:3:-1])
    assert got[0][0].tolist() == [293] and got[1][1].tolist() == [1024]


def test_a_row_that_rounds_up(ctx, families):
    """233 (image 240) against 36: |c^|^2 > |c|^2, so a prologue that takes the stat6 columns in another order raises the
    threshold past the pair (tests/test_fp6_filter.py has the figures); for the rows of the other families, which round
    down, every order of the columns lowers it."""
    got, _ = _run(ctx, [families[6], families[0]])
    assert got[0][0].tolist() == [101] and got[0][1].tolist() == [84]


def test_the_same_pairs_at_a_cut_of_d2(ctx, families):
    """The self distance one step the other way, D* = d2: the pair is not accepted, and K1 agrees."""
    fams = [Family(ctx, k, D=families[k].d2, tb=families[k].tb) for k in (0, 4)]
    got, _, _, fb = _ab(ctx, [(f.qb, f.tb) for f in fams], TAU)
    assert fb == 0
    for f, g in zip(fams, got):
        f.check(g)
        assert len(g[0]) == 0


def test_near_misses(ctx, families):
    """136 against 152 with one byte of m moved by 1.  m[5] = 153 puts the pair at d2 = 32 801: with D* = 32 801 (d2 = D*)
    and D* = 32 800 (d2 = D* + 1) it is rejected.  Another edit, m[77] = 151, puts it at 32 737 and D* = 32 738 accepts it
    (d2 = D* - 1).  (One byte moved opens the gap to the threshold to tens of steps: these are cases of the rescoring's
    comparison, not of the threshold.)"""
    m1, m2 = np.full(128, 152, np.uint8), np.full(128, 152, np.uint8)
    m1[5], m2[77] = 153, 151
    tb = families[0].tb
    fams = [Family(ctx, 0, D=32801, mrow=m1, tb=tb), Family(ctx, 0, D=32800, mrow=m1, tb=tb), Family(ctx, 0, mrow=m2, tb=tb)]
    assert [f.d2 for f in fams] == [32801, 32801, 32737] and fams[2].D == 32738
    got, _ = _run(ctx, fams)
    assert [len(g[0]) for g in got] == [0, 0, 1]


def _refill(ctx, bank, rows, sd):
    src = ctx.pinned_empty(rows.shape, np.uint8)
    src[:] = rows
    bank.refill_async(src)
    ctx.upload_fence()
    bank.set_selfdist(sd)


@pytest.mark.parametrize("grid", [1, None])
def test_max6_after_a_refill(ctx, families, grid):
    """max6 follows a refill, whose preparation runs with "refill_grid" workgroups (1: one workgroup walks the whole bank).
    A 136 / 152 query bank is created with a row of 255s among its background (larger maxima than the family's: words left
    over from it only loosen the threshold) and refilled to the family's rows; another is created with rows of 0 .. 6
    (smaller maxima: words left over from them raise the threshold above the edge pair's accumulator, and words that no
    refill updates are these) and refilled to the family's rows; that one then goes to the small rows, to the family's, to
    the large ones and to the family's again.  The second pair of the batch, 136 / 255, stays as it is."""
    f, other = families[0], families[3]
    keep = ctx.get_option("refill_grid")
    rng = np.random.default_rng(77)
    big = rng.integers(0, 41, (NQ, 128)).astype(np.uint8)
    big[17] = 255
    small = rng.integers(0, 7, (NQ, 128)).astype(np.uint8)
    assert _sq(big).max() > _sq(f.Q).max() > _sq(small).max()
    err = lambda a: _sq(a.astype(np.int64) - VAL[a]).max()
    assert err(big) > err(f.Q) > err(small)
    try:
        if grid is not None:
            ctx.set_option("refill_grid", grid)
        def to_the_family(qb):
            _refill(ctx, qb, f.Q, f.sd)
            got, _, rec, fb = _ab(ctx, [(qb, f.tb), (other.qb, other.tb)], TAU)
            f.check(got[0])
            other.check(got[1])
            assert fb == 0 and rec >= len(f.crows) + len(other.crows)
            assert got[0][0].tolist() == [f.mrows[0]] and got[0][1].tolist() == [f.crows[0]]

        for created in (big, small):
            qb = ctx.bank(created)
            qb.set_selfdist(f.sd)
            _ab(ctx, [(qb, f.tb), (other.qb, other.tb)], TAU)
            to_the_family(qb)
        _refill(ctx, qb, small, f.sd)
        _ab(ctx, [(qb, f.tb), (other.qb, other.tb)], TAU)
        to_the_family(qb)
        _refill(ctx, qb, big, f.sd)
        to_the_family(qb)
    finally:
        ctx.set_option("refill_grid", keep)


def _packed(want):
    q, t, d, _ = want
    return sharding.pack_matches(q, t, d)


def _ran(ctx, n_copies):
    """The last filter launch left at least one record per copy of c and kept its pairs itself."""
    rec, fb = ctx.get_option("fp6_records"), ctx.get_option("fp6_fallbacks")
    assert rec >= n_copies > 0 and fb == 0, (rec, fb)


def test_single_pair_calls_with_host_results(ctx, families):
    """With "nw" 8 the single-pair plan has the filter's shape at these sizes, so the single-pair calls reach the filter: the
    six families one by one through fm_match_accepted, then through fm_match_accepted_async back to back with one sync
    (the calls share the one FP6 list; "fp6_records" then holds the last launch's words)."""
    keep = ctx.get_option("nw")
    try:
        ctx.set_option("nw", 8)
        for f in families[:6]:
            f.check(ctx.match_accepted(f.qb, f.tb, TAU))
            _ran(ctx, len(f.crows))
        outs = [(ctx.pinned_empty(NQ, np.int32), ctx.pinned_empty(NQ, np.int32), ctx.pinned_empty(NQ, np.float32),
                 ctx.pinned_empty(NQ, np.float64)) for _ in families[:6]]
        cnts = [ctx.pinned_empty(1, np.int64) for _ in families[:6]]
        for f, o, c in zip(families[:6], outs, cnts):
            ctx.match_accepted_async(f.qb, f.tb, TAU, o, c)
        ctx.sync()
        _ran(ctx, len(families[5].crows))
        for f, o, c in zip(families[:6], outs, cnts):
            f.check(tuple(np.array(a[:int(c[0])]) for a in o))
    finally:
        ctx.set_option("nw", keep)


def test_calls_with_device_results(ctx, families):
    """fm_match_accepted_dev pair by pair (the filter's shape through "nw" 8) and fm_match_accepted_dev_batch on the six pairs:
    the packed rows (query row, train row, distance bits) on the device equal the oracle's."""
    import torch
    keep = ctx.get_option("nw")
    dev = torch.device("cuda", 0)
    try:
        ctx.set_option("nw", 8)
        for f in families[:6]:
            rows = torch.full((NQ, 3), -7, dtype=torch.int32, device=dev)
            cnt = torch.zeros(1, dtype=torch.int64, device=dev)
            n = ctx.match_accepted_dev(f.qb, f.tb, TAU, rows.data_ptr(), cnt.data_ptr(), NQ)
            _ran(ctx, len(f.crows))
            assert n == len(f.want[0]) == int(cnt.cpu()[0])
            assert np.array_equal(rows.cpu().numpy()[:n], _packed(f.want))
        rows = torch.full((6, NQ, 3), -7, dtype=torch.int32, device=dev)
        cnt = torch.zeros(6, dtype=torch.int64, device=dev)
        ctx.match_accepted_dev_batch([(f.qb, f.tb) for f in families[:6]], TAU, rows.data_ptr(), cnt.data_ptr(), NQ)
        ctx.sync()
        torch.cuda.synchronize()
        _ran(ctx, sum(len(f.crows) for f in families[:6]))
        rows, cnt = rows.cpu().numpy(), cnt.cpu().numpy()
        for k, f in enumerate(families[:6]):
            assert int(cnt[k]) == len(f.want[0])
            assert np.array_equal(rows[k, :int(cnt[k])], _packed(f.want))
    finally:
        ctx.set_option("nw", keep)
