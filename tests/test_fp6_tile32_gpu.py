"""GPU: the FP6 filter sweep on 32 x 32 x 64 tiles (filter6.hip: 128 output rows per wave, 1024 per workgroup) must report, byte
for byte, what K1 reports (option "fp6_filter" 0) and what the oracle reports.  Two things are new with the tile: the 32 x 32
accumulator layout, through which every streamed row gets its accumulator start, and the workgroup's two 512-row pieces of
K1's key array.  Train rows are the sweep's output rows, query rows the streamed ones.

What the first case cannot see: a start-value map that is wrong by a PERMUTATION of a unit's rows gives some high-norm row
a low-norm row's start; against a low-norm output row that lane then fires falsely, the (row, unit) record is written
anyway and the rescoring finds the true match.  The case catches maps that lose or repeat rows."""
import numpy as np
import pytest

import oracle
from fastmatch_amd import synth

pytestmark = pytest.mark.gpu

TAU = 0.7
SELF = 450.0          # caller self distances: the cut is D* = (0.7 * 450)^2 = 99 225


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


def _ab(ctx, pairs, tau):
    """The batch under the filter and under K1, equal byte for byte; the filter ran and kept its hits within the list."""
    try:
        ctx.set_option("fp6_filter", 1)
        got = _batch(ctx, pairs, tau)
        rec, fb = ctx.get_option("fp6_records"), ctx.get_option("fp6_fallbacks")
        ctx.set_option("fp6_filter", 0)
        want = _batch(ctx, pairs, tau)
    finally:
        ctx.set_option("fp6_filter", 1)
    for g, w in zip(got, want):
        _same(g, w)
    assert rec > 0 and fb == 0, (rec, fb)
    return got


def _pair(ctx, Q, T):
    qb, tb = ctx.bank(Q), ctx.bank(T)
    sd = np.full(len(Q), SELF)
    qb.set_selfdist(sd)
    return qb, tb, sd


def test_accumulator_start_of_every_streamed_row(ctx):
    """320 query rows (2.5 stages); inside every 32-row unit low-norm rows (bytes 20 .. 60) alternate with high-norm ones
    (180 .. 250), the phase flipping from unit to unit so that either class sits on every position of a unit.  200 train rows
    are noisy copies (|noise| <= 3 per byte: d2 <= 1152, the cut is 99 225) of 200 distinct query rows.  A lane that starts a
    low-norm row's accumulator from a high-norm row's value ends far below its threshold and the copy is lost."""
    rng = np.random.default_rng(7)
    nq, nt = 320, 200
    i = np.arange(nq)
    high = ((i & 1) ^ ((i >> 5) & 1)).astype(bool)
    Q = np.where(high[:, None], rng.integers(180, 251, (nq, 128)), rng.integers(20, 61, (nq, 128))).astype(np.uint8)
    # one copied row per (class, position of a unit), from a random unit; the other 136 anywhere
    must = np.array([rng.choice(np.nonzero((high == cls) & ((i & 31) == pos))[0]) for cls in (False, True) for pos in range(32)])
    src = rng.permutation(np.concatenate([must, rng.permutation(np.setdiff1d(i, must))[:nt - len(must)]]))
    T = np.clip(Q[src].astype(np.int64) + rng.integers(-3, 4, (nt, 128)), 0, 255).astype(np.uint8)
    qb, tb, sd = _pair(ctx, Q, T)
    want = _oracle(Q, T, sd, TAU)
    # (from the oracle's rows, so that the comparison below is not vacuous)
    q = want[0]
    assert np.array_equal(np.sort(q), np.sort(src))
    for cls in (False, True):
        assert set((q[high[q] == cls] & 31).tolist()) == set(range(32)), cls
    # (a second pair beside it: a batch of one small pair is planned in K1's 4-wave shape, which the filter leaves to K1)
    Q2, T2, _ = synth.planted_pair(300, 257, seed=100)
    q2, t2, sd2 = _pair(ctx, Q2, T2)
    got = _ab(ctx, [(qb, tb), (q2, t2)], TAU)
    _same(got[0], want)
    _same(got[1], _oracle(Q2, T2, sd2, TAU))


EDGE_SIZES = [(257, 31), (300, 129), (411, 1023), (512, 1025), (640, 1100), (700, 1537)]     # (query rows, train rows)
EDGE_ROWS = [0, 127, 128, 511, 512, 1023, 1024]


def test_tile_and_chunk_edges_in_one_batch(ctx):
    """Train banks around the wave tile (128 rows), K1's 512-row piece and the workgroup's 1024 rows; 31, 129, 1025 and 1100
    rows make an odd number of 512-row pieces, whose last workgroup has its second piece beyond the key array.  Copies of
    distinct query rows sit on the train rows at the edges and on the last row; everything else is random (d2 ~ 590 000, far
    beyond the cut), so the planted rows are the ones to accept."""
    rng = np.random.default_rng(11)
    pairs, wants, planted = [], [], []
    for nq, nt in EDGE_SIZES:
        Q = rng.integers(45, 211, (nq, 128)).astype(np.uint8)
        T = rng.integers(45, 211, (nt, 128)).astype(np.uint8)
        rows = sorted(set([r for r in EDGE_ROWS if r < nt] + [nt - 1]))
        src = rng.permutation(nq)[:len(rows)]
        T[rows] = np.clip(Q[src].astype(np.int64) + rng.integers(-3, 4, (len(rows), 128)), 0, 255).astype(np.uint8)
        qb, tb, sd = _pair(ctx, Q, T)
        pairs.append((qb, tb))
        wants.append(_oracle(Q, T, sd, TAU))
        planted.append(rows)
    got = _ab(ctx, pairs, TAU)
    for g, w, rows in zip(got, wants, planted):
        _same(g, w)
        assert set(rows) <= set(g[1].tolist())
