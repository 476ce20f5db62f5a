"""GPU: the FP6 filter sweep under its own split of the streamed bank (filter6.hip, fp6_plan.h).  K1's plan keeps laying out
the key array `partial` ([K1 splits][output rows]); the filter sweeps the streamed bank in splits of its own count, and its
workgroup (chunk, f) presets K1's slices f, f + nsplit_f, ... of its 1024 output rows.  Whatever the two counts are, the
results must be, byte for byte, what K1 reports (option "fp6_filter" 0) and what the oracle reports, "fp6_records" must
count every firing (lane, unit), and no pair may fall back to K1.

Train rows are the sweep's output rows, query rows the streamed ones: 1029 query rows are 9 stages, the last 32-row unit with
5 real rows; 1537 train rows are 4 of K1's 512-row chunks (two filter workgroups per split), 1100 train rows 3 (the second
piece of the last workgroup lies outside the key array).  Every batch has at least two pairs: a lone small pair is planned in
K1's 4-wave shape, which the filter leaves to K1.  The constructions are those of test_fp6_stagger_gpu.py."""
import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

TAU = 0.7
NQ = 1029
BATCH_SLOTS = 32        # fm_ctx::kBatchSlots: the ring of per-pair workspaces of fm_match_accepted_batch
SPLITS = [(4, 1), (4, 3), (2, 5), (1, 9), (9, 2), (0, 0)]           # ("nsplit", "fp6_nsplit")


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


def _outputs(ctx, pairs):
    cap = max(qb.n for qb, _ in pairs)
    outs = [(ctx.pinned_empty(cap, np.int32), ctx.pinned_empty(cap, np.int32), ctx.pinned_empty(cap, np.float32),
             ctx.pinned_empty(cap, np.float64)) for _ in pairs]
    cnts = [ctx.pinned_empty(1, np.int64) for _ in pairs]
    return outs, cnts


def _read(outs, cnts):
    return [tuple(np.array(a[:int(c[0])]) for a in o) for o, c in zip(outs, cnts)]


def _batch(ctx, pairs, tau):
    outs, cnts = _outputs(ctx, pairs)
    ctx.match_accepted_batch(pairs, tau, outs, cnts)
    ctx.sync()
    return _read(outs, cnts)


class _Options:
    """Context options for the length of a with block."""

    def __init__(self, ctx, **options):
        self.ctx, self.options = ctx, options

    def __enter__(self):
        self.keep = {k: self.ctx.get_option(k) for k in list(self.options) + ["fp6_filter"]}
        for k, v in self.options.items():
            self.ctx.set_option(k, v)
        return self

    def __exit__(self, *exc):
        for k, v in self.keep.items():
            self.ctx.set_option(k, v)
        return False


def _dense(seed, nt):
    """Random bytes 45 .. 210, self distances 3000: D* = (0.7 * 3000)^2 = 4.41e6 is beyond every possible d2 (<= 128 * 165^2 =
    3.48e6), so a lane with a real train row fires for every unit with a real query row, in both lane halves: nt x 33 x 2
    records."""
    rng = np.random.default_rng(seed)
    Q = rng.integers(45, 211, (NQ, 128)).astype(np.uint8)
    T = rng.integers(45, 211, (nt, 128)).astype(np.uint8)
    sd = np.full(NQ, 3000.0)
    want = _oracle(Q, T, sd, TAU)
    assert len(want[0]) > 0
    return Q, T, sd, want


def _sparse(seed, nt, shift=0, noise=3):
    """The train bank holds noisy copies (|noise| <= 3 per byte: d2 <= 1152) of all 1029 query rows -- the copy of row i < 1024
    at train row 128 (i mod 8) + i div 8, those of rows 1024 - 1028 at rows 1024 - 1028 -- then random rows up to nt.  Self
    distances 450: D* = 99 225 against d2 ~ 590 000 of random rows, so exactly the copies are accepted.  With `shift` train row
    t holds the copy that belongs at row t + shift (mod 1029): the same key positions, other keys."""
    rng = np.random.default_rng(seed)
    Q = rng.integers(45, 211, (NQ, 128)).astype(np.uint8)
    src = np.empty(NQ, np.int64)                 # src[train row] = the query row it copies
    i = np.arange(1024)
    src[128 * (i % 8) + i // 8] = i
    src[1024:] = np.arange(1024, NQ)
    src = np.roll(src, -shift)
    T = np.concatenate([np.clip(Q[src].astype(np.int64) + rng.integers(-noise, noise + 1, (NQ, 128)), 0, 255),
                        rng.integers(45, 211, (nt - NQ, 128))]).astype(np.uint8)
    sd = np.full(NQ, 450.0)
    want = _oracle(Q, T, sd, TAU)
    assert np.array_equal(np.sort(want[0]), np.arange(NQ))
    assert np.array_equal(src[want[1]], want[0])
    return Q, T, sd, want


@pytest.fixture(scope="module")
def data():
    """Inputs and oracle results, computed once: dense pairs of 1537 and 1100 train rows, sparse pairs of 1100 and 1537, and
    `stale`: the sparse pair of 1100 rows (same seed, same query bank) with EXACT copies one train row off -- a key K1 leaves
    for it (d2 = 0, the neighbour's query row) beats the true key of the same train row wherever it survives."""
    return {"dense1537": _dense(41, 1537), "dense1100": _dense(42, 1100),
            "sparse1100": _sparse(43, 1100), "sparse1537": _sparse(44, 1537),
            "stale": _sparse(43, 1100, shift=1, noise=0)}


@pytest.fixture(scope="module")
def banks(ctx, data):
    out = {}
    for name, (Q, T, sd, _) in data.items():
        qb, tb = ctx.bank(Q), ctx.bank(T)
        qb.set_selfdist(sd)
        out[name] = (qb, tb)
    return out


def _want(data, names):
    return [data[n][3] for n in names]


DENSE = ["dense1537", "dense1100"]
SPARSE = ["sparse1100", "sparse1537"]


@pytest.mark.parametrize("nsplit,fp6_nsplit", SPLITS)
def test_dense_records_under_both_counts(ctx, data, banks, nsplit, fp6_nsplit):
    """Every real (row, unit, half) fires once: (1537 + 1100) x 33 x 2 = 174 042 records.  K1's 9 stages in "nsplit" slices, the
    filter's in "fp6_nsplit" splits (0, 0: K1's plan gives one slice, the filter's rule two splits): more splits than slices,
    fewer, a count that does not divide the other, and each remainder of the stage loop's unroll by three."""
    pairs = [banks[n] for n in DENSE]
    with _Options(ctx, nsplit=nsplit, fp6_nsplit=fp6_nsplit):
        ctx.set_option("fp6_filter", 1)
        got = _batch(ctx, pairs, TAU)
        rec, fb = ctx.get_option("fp6_records"), ctx.get_option("fp6_fallbacks")
        ctx.set_option("fp6_filter", 0)
        k1 = _batch(ctx, pairs, TAU)
    print("nsplit", nsplit, "fp6_nsplit", fp6_nsplit, "fp6_records", rec, "fp6_fallbacks", fb)
    assert rec == (1537 + 1100) * 33 * 2 == 174042 and fb == 0, (rec, fb)
    for g, k, w in zip(got, k1, _want(data, DENSE)):
        _same(g, k)
        _same(g, w)


@pytest.mark.parametrize("nsplit,fp6_nsplit", SPLITS)
def test_sparse_copies_under_both_counts(ctx, data, banks, nsplit, fp6_nsplit):
    """All 1029 query rows are accepted, each with its copy, in both pairs: a slice of K1's keys that no workgroup preset, or
    a stage that no split swept, is a wrong or a missing match."""
    pairs = [banks[n] for n in SPARSE]
    with _Options(ctx, nsplit=nsplit, fp6_nsplit=fp6_nsplit):
        ctx.set_option("fp6_filter", 1)
        got = _batch(ctx, pairs, TAU)
        rec, fb = ctx.get_option("fp6_records"), ctx.get_option("fp6_fallbacks")
        ctx.set_option("fp6_filter", 0)
        k1 = _batch(ctx, pairs, TAU)
    print("nsplit", nsplit, "fp6_nsplit", fp6_nsplit, "fp6_records", rec, "fp6_fallbacks", fb)
    assert rec >= 2 * NQ and fb == 0, (rec, fb)
    for g, k, w in zip(got, k1, _want(data, SPARSE)):
        _same(g, k)
        _same(g, w)
        assert np.array_equal(np.sort(g[0]), np.arange(NQ))


def test_filter_presets_every_slice_k1_left(ctx, data, banks):
    """K1 runs ("fp6_filter" 0, "nsplit" 4: three slices of three stages) alternate with filter runs of the sparse pair at
    "fp6_nsplit" 1 -- one split, whose workgroups must preset all of K1's slices -- for 2 x kBatchSlots + 1 calls.  A K1 call
    takes three workspaces of the ring (the dense pair and twice `stale`, which has the sparse pair's layout), a filter call
    two, so the filter's workspaces come round to ones that hold K1's keys in every slice; a `stale` key that survives takes
    its train row away from the query row that owns it."""
    k1_names = ["dense1537", "stale", "stale"]
    f_names = ["sparse1100", "sparse1100"]
    k1_pairs, f_pairs = [banks[n] for n in k1_names], [banks[n] for n in f_names]
    with _Options(ctx, nsplit=4, fp6_nsplit=1):
        for call in range(2 * BATCH_SLOTS + 1):
            if call % 2 == 0:
                ctx.set_option("fp6_filter", 0)
                for g, w in zip(_batch(ctx, k1_pairs, TAU), _want(data, k1_names)):
                    _same(g, w)
            else:
                ctx.set_option("fp6_filter", 1)
                got = _batch(ctx, f_pairs, TAU)
                assert ctx.get_option("fp6_fallbacks") == 0
                for g, w in zip(got, _want(data, f_names)):
                    _same(g, w)


def test_five_launches_in_flight(ctx, data, banks):
    """The two-pair batch five times back to back, dense and sparse alternating, each into its own outputs, a ticket after each
    (fm_mark) and no host wait until all are enqueued: launches in flight must not share the filter's lists, its count words
    or the cut words.  fm_wait on a ticket must cover that launch's sweep, rescoring, guard and tails."""
    names = [DENSE, SPARSE, DENSE, SPARSE, DENSE]
    sets, tickets = [], []
    for ns in names:
        pairs = [banks[n] for n in ns]
        outs, cnts = _outputs(ctx, pairs)
        for c in cnts:
            c[0] = -1
        ctx.match_accepted_batch(pairs, TAU, outs, cnts)
        sets.append((outs, cnts))
        tickets.append(ctx.mark())
    try:
        for ns, (outs, cnts), tk in zip(names, sets, tickets):
            ctx.wait(tk)
            for g, w in zip(_read(outs, cnts), _want(data, ns)):
                _same(g, w)
    finally:
        ctx.sync()
    assert ctx.get_option("fp6_fallbacks") == 0
    assert ctx.get_option("fp6_records") == (1537 + 1100) * 33 * 2
