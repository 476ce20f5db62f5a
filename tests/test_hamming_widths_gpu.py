"""GPU: every Hamming entry point at every K-step count.  The Hamming kernels are compiled once per KS = ceil(bytes / 16) =
1 .. 4 and the host code sizes rows, strides and stack views from KS; this module runs the bank-pair calls at 1, 16, 17, 32,
33, 40, 48, 49 and 64 bytes and the collection calls at 1, 33, 48 and 64 bytes, on the rows of tests/hamming_width_ref.py, in
which every 16-byte K step and every row's last real byte decide the answers (tests/test_hamming_widths_host.py asserts that).

The references are the NumPy ones the other Hamming tests use (hamming_ref, hamming_fast_ref, hamming_radius_ref,
masked_ref.knn_bin, mutual_ratio_ref, xcheck_each_ref, pairs_ref).  Hamming distances are integers: indices, counts and order
are compared exactly, float32 and float64 values as bit patterns.  There is no tolerance anywhere.

Shapes: 300 query rows (two 256-row output chunks, the second partial) against 1100 train rows (9 stages of 128 in 3 splits,
the last stage partial); images of 129, 0, 1, 128, 700 and 127 rows."""
import functools

import numpy as np
import pytest

import fastmatch_amd
import hamming_fast_ref as HF
import hamming_radius_ref as HR
import hamming_ref as H
import hamming_width_ref as W
import masked_ref
import mutual_ratio_ref as MR
import pairs_ref
import xcheck_each_ref as XE
from fastmatch_amd import _ffi

pytestmark = pytest.mark.gpu

WIDTHS = W.WIDTHS
COLL_WIDTHS = W.COLL_WIDTHS
MASK_WIDTHS = [1, 33, 48, 64]
EINVAL = -1
TAU = W.TAU
INF = float("inf")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same(got, want, what=""):
    """Tuples of arrays: shapes, dtypes and raw bits."""
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype, "%s [%d]: %s %s / %s %s" % (what, i, g.shape, g.dtype, w.shape, w.dtype)
        bad = np.nonzero(_bits(g) != _bits(w))
        assert not len(bad[0]), "%s [%d]: %d differ, first at %s" % (what, i, len(bad[0]), [int(b[0]) for b in bad])


def _same_accepted(got, want, what=""):
    """(qidx, tidx, dist, ratio): the float64 ratios bit for bit (none of them is NaN: an accepted row passed ratio < tau)."""
    assert not np.isnan(want[3]).any()
    _same(got, want, what)


def _torch():
    import torch
    return torch


@functools.lru_cache(maxsize=None)
def _knn8(width, reverse=False):
    Q, T = W.pair(width)
    return H.knn(T, Q, 8) if reverse else H.knn(Q, T, 8)


@functools.lru_cache(maxsize=None)
def _selfdist(width):
    Q, T = W.pair(width)
    return HF.self_dist(Q), HF.self_dist(T)


@functools.lru_cache(maxsize=None)
def _gallery_selfdist(width):
    return HF.self_dist(W.gallery(width)[0])


class _Banks(object):
    """Context manager: binary banks of the given matrices, closed at the end."""

    def __init__(self, ctx, *mats):
        self.ctx, self.mats, self.banks = ctx, mats, []

    def __enter__(self):
        for m in self.mats:
            self.banks.append(self.ctx.bank_binary(m))
        return self.banks

    def __exit__(self, *exc):
        for b in self.banks:
            b.close()
        return False


def _collection(ctx, images):
    c = ctx.collection()
    for i, im in enumerate(images):
        assert c.add_binary(im) == i
    return c


def _raises_einval(call, what):
    with pytest.raises(fastmatch_amd.FastMatchHipError) as e:
        call()
    assert e.value.code == EINVAL, (what, str(e.value))
    assert "width" in str(e.value) or "dim mismatch" in str(e.value), (what, str(e.value))      # (refused for the width, nothing else)


# ---- bank pairs ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", WIDTHS)
def test_knn_crosscheck_and_ratio_in_both_directions(ctx, width):
    Q, T = W.pair(width)
    assert W.sweep_splits(W.NQ, W.NT) == (3, 3)
    with _Banks(ctx, Q, T) as (qb, tb):
        assert qb.dim == tb.dim == width and qb.kind == _ffi.FM_BANK_BIN
        for reverse, (a, b, A, B) in enumerate(((qb, tb, Q, T), (tb, qb, T, Q))):
            what = "%d bytes, %s" % (width, "T against Q" if reverse else "Q against T")
            ridx, rdist = _knn8(width, bool(reverse))
            for k in range(1, 9):
                _same(ctx.knn(a, b, k), (ridx[:, :k], rdist[:, :k]), "%s, knn k = %d" % (what, k))
            _same(ctx.knn2(a, b), (ridx[:, :2], rdist[:, :2]), what + ", knn2")
            _same(ctx.xcheck1(a, b), H.xcheck(A, B), what + ", xcheck1")
            want = H.ratio_match(A, B, TAU)
            assert len(want[0]) > 0
            _same_accepted(ctx.knn2_ratio(a, b, TAU), want, what + ", knn2_ratio")


@pytest.mark.parametrize("width", WIDTHS)
def test_self_distances_of_one_bank(ctx, width):
    Q, T = W.pair(width)
    with _Banks(ctx, Q, T) as banks:
        for b, sd in zip(banks, _selfdist(width)):
            _same((ctx.hamming_self_dist(b),), (sd,), "%d bytes, %d rows" % (width, b.n))
            _same(ctx.hamming_self_dist_batch([b]), (sd,), "%d bytes, %d rows, a batch of one" % (width, b.n))


def test_self_distances_of_a_batch_that_mixes_all_widths(ctx):
    """One call over the query and train banks of every width.  In ascending width order consecutive banks of one K-step count
    share a launch ((1, 16), (17, 32), (33, 40, 48), (49, 64)); interleaved, every bank splits it."""
    mats = [m for w in WIDTHS for m in W.pair(w)]
    refs = [sd for w in WIDTHS for sd in _selfdist(w)]
    by_bank = [m for i in (0, 1) for w in WIDTHS for m in (W.pair(w)[i],)]
    by_bank_refs = [sd for i in (0, 1) for w in WIDTHS for sd in (_selfdist(w)[i],)]
    mixed = [4, 0, 6, 2, 8, 5, 1, 7, 3]                               # 33, 1, 48, 17, 64, 40, 16, 49, 32 bytes
    assert all(W.ksteps(WIDTHS[a]) != W.ksteps(WIDTHS[b]) for a, b in zip(mixed, mixed[1:])) and sorted(mixed) == list(range(9))
    for what, ms, rs in (("width by width", mats, refs), ("all query banks, then all train banks", by_bank, by_bank_refs),
                         ("no two neighbours of one K-step count", [W.pair(WIDTHS[i])[0] for i in mixed],
                          [_selfdist(WIDTHS[i])[0] for i in mixed])):
        with _Banks(ctx, *ms) as banks:
            _same(ctx.hamming_self_dist_batch(banks), rs, what)
            # the enqueue-only form attaches the same values: the ratios of a pair call are a division by them
            with _Banks(ctx, *ms[:6]) as fresh:
                assert ctx.hamming_self_dist_batch(fresh, want_host=False) is None
                for m, b, sd in zip(ms, fresh, rs):
                    t = W.pair(m.shape[1])[1]
                    with _Banks(ctx, t) as (tb,):
                        _same_accepted(ctx.hamming_match_accepted(b, tb, INF), HF.match_accepted(m, t, sd, INF), what + ", attached")
    ctx.sync()            # (the enqueue-only calls are accounted at the next sync: none of that is left for a later test's stats)


@pytest.mark.parametrize("width", WIDTHS)
def test_match_ratio_and_accepted_in_both_directions(ctx, width):
    Q, T = W.pair(width)
    sdq, sdt = _selfdist(width)
    with _Banks(ctx, Q, T) as (qb, tb):
        _same(ctx.hamming_self_dist_batch([qb, tb]), (sdq, sdt), "%d bytes, self distances" % width)
        some = 0
        for a, b, A, B, sd in ((qb, tb, Q, T, sdq), (tb, qb, T, Q, sdt)):
            for tau in (TAU, INF):
                what = "%d bytes, %d rows against %d, tau = %r" % (width, a.n, b.n, tau)
                rt, rd, rr, rp = HF.match_ratio(A, B, sd, tau)
                tidx, dist, ratio, passed, npass = ctx.hamming_match_ratio(a, b, tau)
                _same((tidx, dist), (rt, rd), what)
                assert HF.same_f64(ratio, rr) and np.array_equal(passed, rp) and npass == rp.sum(), what
                want = HF.match_accepted(A, B, sd, tau)
                _same_accepted(ctx.hamming_match_accepted(a, b, tau), want, what + ", accepted")
                some += len(want[0])
        assert some > 0


@pytest.mark.parametrize("width", WIDTHS)
def test_mutual_ratio_in_both_directions(ctx, width):
    Q, T = W.pair(width)
    with _Banks(ctx, Q, T) as (qb, tb):
        some = 0
        for a, b, A, B in ((qb, tb, Q, T), (tb, qb, T, Q)):
            for symmetric in (False, True):
                want = MR.mutual_ratio(A, B, TAU, symmetric, binary=True)
                what = "%d bytes, %d rows against %d, symmetric = %r" % (width, a.n, b.n, symmetric)
                _same_accepted(ctx.mutual_ratio(a, b, TAU, symmetric), want, what)
                assert ctx.mutual_ratio_count(a, b, TAU, symmetric) == len(want[0]), what
                some += len(want[0])
        assert some > 0


@pytest.mark.parametrize("width", WIDTHS)
def test_radius_match_with_one_radius_and_with_one_per_row(ctx, width):
    Q, T = W.pair(width)
    with _Banks(ctx, Q, T) as (qb, tb):
        for a, b, A, B in ((qb, tb, Q, T), (tb, qb, T, Q)):
            ref = HR.Ref(A, B)
            what = "%d bytes, %d rows against %d" % (width, a.n, b.n)
            assert (ref.counts(np.float32(3)) > 0).any()
            for r in (1, 3, 6, 11, 4 * width, INF):          # h < 11: every row of the same base; 4 * width: about half of the others
                HR.same_pair_lists(ctx.hamming_radius_match(a, b, np.float32(r)), ref.cut(np.float32(r)), "%s, r = %r" % (what, r))
            radii = HR.mixed_radii(ref, seed=width)
            HR.same_pair_lists(ctx.hamming_radius_match(a, b, radii), ref.cut(radii), what + ", one radius per row")


def _pair_masks(width):
    """A random mask of density 0.5, and one that forbids exactly every row's reference nearest neighbour."""
    rng = np.random.default_rng(300 + width)
    half = (rng.random((W.NQ, W.NT)) < 0.5).astype(np.uint8)
    second = np.ones((W.NQ, W.NT), np.uint8)
    second[np.arange(W.NQ), _knn8(width)[0][:, 0]] = 0
    return (("density 0.5", half), ("the nearest neighbour forbidden", second))


@pytest.mark.parametrize("width", MASK_WIDTHS)
def test_knn_masked(ctx, width):
    Q, T = W.pair(width)
    ridx, rdist = _knn8(width)
    with _Banks(ctx, Q, T) as (qb, tb):
        for name, m in _pair_masks(width):
            with ctx.mask(W.NQ, W.NT) as mk:
                mk.set(m)
                for k in (1, 2, 3, 8):
                    want = masked_ref.knn_bin(Q, T, m, k)
                    _same(ctx.knn_masked(qb, tb, mk, k), want, "%d bytes, %s, k = %d" % (width, name, k))
                    if name != "density 0.5":               # (the lists move up by one: what was second is first)
                        assert not np.array_equal(want[0][:, 0], ridx[:, 0]) and np.array_equal(want[1][:, 0], rdist[:, 1])


# ---- device sources --------------------------------------------------------------------------------------------------------
def _pitched(rows, extra=7, fill=0xFF):
    """A uint8 CUDA tensor [n, width + extra] with `rows` in its first `width` columns and `fill` behind every row."""
    n, width = rows.shape
    wide = np.full((n, width + extra), fill, np.uint8)
    wide[:, :width] = rows
    return _torch().from_numpy(wide).cuda()


@pytest.mark.parametrize("width", [33, 48])
def test_banks_and_images_from_pitched_device_rows(ctx, width):
    """pitch = width + 7 with 0xFF between the rows: a byte read from behind the row's width would count 8 bits."""
    torch = _torch()
    Q, T = W.pair(width)
    s = torch.cuda.current_stream().cuda_stream
    dq, dt = _pitched(Q), _pitched(T)
    dev_q = ctx.bank_from_device(dq.data_ptr(), _ffi.FM_DT_BIN, W.NQ, width, pitch=width + 7, stream=s)
    dev_t = ctx.bank_from_device(dt.data_ptr(), _ffi.FM_DT_BIN, W.NT, width, pitch=width + 7, stream=s)
    try:
        assert (dev_q.n, dev_q.dim, dev_q.kind) == (W.NQ, width, _ffi.FM_BANK_BIN)
        with _Banks(ctx, Q, T) as (qb, tb):
            ridx, rdist = _knn8(width)
            for a, b, what in ((dev_q, dev_t, "both from the device"), (dev_q, tb, "the query"), (qb, dev_t, "the train bank")):
                _same(ctx.knn2(a, b), ctx.knn2(qb, tb), "%d bytes, %s, knn2 against the host-built pair" % (width, what))
                _same(ctx.knn2(a, b), (ridx[:, :2], rdist[:, :2]), "%d bytes, %s, knn2" % (width, what))
                _same(ctx.xcheck1(a, b), ctx.xcheck1(qb, tb), "%d bytes, %s, xcheck1 against the host-built pair" % (width, what))
                _same(ctx.xcheck1(a, b), H.xcheck(Q, T), "%d bytes, %s, xcheck1" % (width, what))
            _same((ctx.hamming_self_dist(dev_q),), (_selfdist(width)[0],), "self distances of the device-built bank")
    finally:
        dev_q.close()
        dev_t.close()
    Q, images = W.gallery(width)
    keep = [_pitched(im) for im in images]
    with ctx.collection() as dev, _collection(ctx, images) as host, _Banks(ctx, Q) as (qb,):
        for i, (im, t) in enumerate(zip(images, keep)):
            n = im.shape[0]
            assert dev.add_from_device(t.data_ptr() if n else 0, _ffi.FM_DT_BIN, n, width, pitch=width + 7, stream=s) == i
        assert dev.info() == host.info() == (len(images), sum(W.IMAGE_SIZES), width, _ffi.FM_BANK_BIN)
        for k in (2, 8):
            _same(dev.knn(qb, k), host.knn(qb, k), "%d bytes, device adds, knn k = %d against host adds" % (width, k))
            _same(dev.knn(qb, k), W.stacked_knn(Q, images, k), "%d bytes, device adds, knn k = %d" % (width, k))
        _same(dev.xcheck1_each(qb), host.xcheck1_each(qb), "%d bytes, device adds, xcheck1_each against host adds" % width)
        _same(dev.xcheck1_each(qb), XE.xcheck_each(Q, images, binary=True), "%d bytes, device adds, xcheck1_each" % width)


# ---- collections -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", COLL_WIDTHS)
def test_collection_knn_ratio_and_votes(ctx, width):
    Q, images = W.gallery(width)
    with _collection(ctx, images) as c, _Banks(ctx, Q) as (qb,):
        assert c.info() == (len(images), sum(W.IMAGE_SIZES), width, _ffi.FM_BANK_BIN)
        for k in (1, 2, 3, 8):
            _same(c.knn(qb, k), W.stacked_knn(Q, images, k), "%d bytes, knn k = %d" % (width, k))
        accepted, votes0, votes1 = W.stacked_ratio(Q, images, TAU)
        assert len(accepted[0]) > 0 and votes1.sum() > 0
        _same_accepted(c.knn2_ratio(qb, TAU), accepted, "%d bytes, knn2_ratio" % width)
        _same((c.votes(qb, TAU, 0), c.votes(qb, TAU, 1)), (votes0, votes1), "%d bytes, votes" % width)
        idx, dist = c.knn2_each(qb)
        for i, im in enumerate(images):
            _same((idx[i], dist[i]), H.knn(Q, im, 2), "%d bytes, knn2_each, image %d" % (width, i))


def _image_masks(width):
    Q, images = W.gallery(width)
    rng = np.random.default_rng(400 + width)
    half = [(rng.random((W.NQ, n)) < 0.5).astype(np.uint8) for n in W.IMAGE_SIZES]
    second = [np.ones((W.NQ, n), np.uint8) for n in W.IMAGE_SIZES]
    img, loc, _ = W.stacked_knn(Q, images, 1)
    for q in range(W.NQ):
        second[img[q, 0]][q, loc[q, 0]] = 0
    return (("density 0.5", half), ("the nearest neighbour forbidden", second))


@pytest.mark.parametrize("width", COLL_WIDTHS)
def test_collection_knn_masked_with_one_mask_per_image(ctx, width):
    Q, images = W.gallery(width)
    with _collection(ctx, images) as c, _Banks(ctx, Q) as (qb,):
        for name, masks in _image_masks(width):
            with c.mask(W.NQ) as mk:
                for i, m in enumerate(masks):
                    mk.set(m, img=i)
                for k in (1, 2, 3, 8):
                    _same(c.knn_masked(qb, mk, k), W.stacked_knn_masked(Q, images, masks, k), "%d bytes, %s, k = %d" % (width, name, k))


@pytest.mark.parametrize("width", COLL_WIDTHS)
def test_collection_radius_match(ctx, width):
    Q, images = W.gallery(width)
    ref = HR.Ref(Q, images)
    with _collection(ctx, images) as c, _Banks(ctx, Q) as (qb,):
        for r in (1, 3, 11, 4 * width, INF):
            HR.same_coll_lists(c.hamming_radius_match(qb, np.float32(r)), ref.cut(np.float32(r)), "%d bytes, r = %r" % (width, r))
        radii = HR.mixed_radii(ref, seed=width)
        HR.same_coll_lists(c.hamming_radius_match(qb, radii), ref.cut(radii), "%d bytes, one radius per row" % width)


@pytest.mark.parametrize("width", COLL_WIDTHS)
def test_collection_crosscheck_mutual_ratio_and_accepted_image_by_image(ctx, width):
    Q, images = W.gallery(width)
    sd = _gallery_selfdist(width)
    with _collection(ctx, images) as c, _Banks(ctx, Q) as (qb,):
        want = XE.xcheck_each(Q, images, binary=True)
        assert (want[0] >= 0).any()
        _same(c.xcheck1_each(qb), want, "%d bytes, xcheck1_each" % width)
        _same((c.mutual_votes(qb),), (XE.counts(want[0]),), "%d bytes, mutual_votes" % width)
        for symmetric in (False, True):
            ref = MR.mutual_ratio_each(Q, images, TAU, symmetric, binary=True)
            got = c.mutual_ratio_each(qb, TAU, symmetric)
            assert len(got) == len(images) and sum(len(r[0]) for r in ref) > 0
            for i, (g, r) in enumerate(zip(got, ref)):
                _same_accepted(g, r, "%d bytes, mutual_ratio_each, symmetric = %r, image %d" % (width, symmetric, i))
        _same(ctx.hamming_self_dist_batch([qb]), (sd,), "%d bytes, self distances" % width)
        for tau in (TAU, INF):
            got = c.hamming_match_accepted_each(qb, tau)
            ref = [HF.match_accepted(Q, im, sd, tau) for im in images]
            assert len(got) == len(images) and sum(len(r[0]) for r in ref) > 0
            for i, (g, r) in enumerate(zip(got, ref)):
                _same_accepted(g, r, "%d bytes, hamming_match_accepted_each, tau = %r, image %d" % (width, tau, i))


@pytest.mark.parametrize("width", COLL_WIDTHS)
def test_collection_image_pairs(ctx, width):
    """The match graph with the images themselves as its nodes: every ordered pair of images, through sub-bank views into the
    stack that are taken by row bytes."""
    _, images = W.gallery(width)
    ordered = [(a, b) for a in range(len(images)) for b in range(len(images)) if a != b]
    with _collection(ctx, images) as c:
        for symmetric in (False, True):
            for pairs in (None, ordered):
                ref = pairs_ref.pairs_mutual_ratio(images, pairs, TAU, symmetric, binary=True)
                got = c.pairs_mutual_ratio(pairs, TAU, symmetric)
                assert len(got) == len(ref) == (15 if pairs is None else 30) and sum(len(r[0]) for r in ref) > 0
                for p, (g, r) in enumerate(zip(got, ref)):
                    _same_accepted(g, r, "%d bytes, symmetric = %r, pair %d of %s" % (width, symmetric, p, "all" if pairs is None else "ordered"))
                offsets = c.pairs_mutual_ratio_counts(pairs, TAU, symmetric)
                assert np.array_equal(np.diff(offsets), [len(r[0]) for r in ref])


def test_collection_device_results_at_48_bytes(ctx):
    torch = _torch()
    width = 48
    Q, images = W.gallery(width)
    sd = _gallery_selfdist(width)
    s = torch.cuda.current_stream().cuda_stream
    with _collection(ctx, images) as c, _Banks(ctx, Q) as (qb,):
        for k in (2, 5):
            d = [torch.from_numpy(np.full((W.NQ, k), -9, dt)).cuda() for dt in (np.int32, np.int32, np.float32)]
            c.knn_dev(qb, k, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), consumer_stream=s)
            _same([x.cpu().numpy() for x in d], W.stacked_knn(Q, images, k), "knn_dev, k = %d" % k)
        ctx.hamming_self_dist_batch([qb], want_host=False)
        ref = [HF.match_accepted(Q, im, sd, INF) for im in images]
        full = np.array([len(r[0]) for r in ref], np.int64)
        cap = int(full.max()) - 3                                        # one image overflows
        assert cap > 0
        rows = torch.from_numpy(np.full((len(images), cap, 3), -9, np.int32)).cuda()
        cnt = torch.from_numpy(np.full(len(images), -9, np.int64)).cuda()
        h = np.full(len(images), -9, np.int64)
        c.hamming_match_accepted_each_dev(qb, INF, rows.data_ptr(), cnt.data_ptr(), cap, h_counts=h, consumer_stream=s)
        r, n = rows.cpu().numpy(), cnt.cpu().numpy()
        assert np.array_equal(h, full) and np.array_equal(n, np.minimum(full, cap))
        for i, (aq, at, ad, _) in enumerate(ref):
            m = int(n[i])
            _same((r[i, :m, 0], r[i, :m, 1], r[i, :m, 2].view(np.float32)), (aq[:m], at[:m], ad[:m]), "accepted_each_dev, image %d" % i)
            assert (r[i, m:] == -9).all()
    ctx.sync()


# ---- one collection, three widths ------------------------------------------------------------------------------------------
def _collection_outputs(ctx, c, qb):
    out = list(c.knn(qb, 2)) + list(c.knn(qb, 8)) + list(c.knn2_each(qb)) + list(c.xcheck1_each(qb))
    out += list(c.hamming_radius_match(qb, np.float32(6)))
    for rows in c.mutual_ratio_each(qb, TAU):
        out += list(rows)
    return out


def test_a_collection_refilled_at_other_widths(ctx):
    """48 bytes, clear(), 33 bytes (the same K-step count: the arrays stay, and what the 48-byte rows left in the bytes 33 .. 47
    must not count), clear(), 17 bytes (another K-step count: new arrays).  Every time the collection answers as a fresh one."""
    with ctx.collection() as c:
        for width in (48, 33, 17):
            Q, images = W.gallery(width)
            for i, im in enumerate(images):
                assert c.add_binary(im) == i
            assert c.info() == (len(images), sum(W.IMAGE_SIZES), width, _ffi.FM_BANK_BIN)
            with _Banks(ctx, Q) as (qb,), _collection(ctx, images) as fresh:
                got = _collection_outputs(ctx, c, qb)
                _same(got, _collection_outputs(ctx, fresh, qb), "%d bytes, against a fresh collection" % width)
                _same(got[:3], W.stacked_knn(Q, images, 2), "%d bytes, knn" % width)
                _same(got[3:6], W.stacked_knn(Q, images, 8), "%d bytes, knn k = 8" % width)
                _same(got[8:10], XE.xcheck_each(Q, images, binary=True), "%d bytes, xcheck1_each" % width)
                _same(c.pairs_mutual_ratio(None, TAU)[2], pairs_ref.pairs_mutual_ratio(images, [(0, 3)], TAU, binary=True)[0],
                      "%d bytes, image pair (0, 3)" % width)
            c.clear()
            assert c.info()[:2] == (0, 0)


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_a_33_byte_query_is_refused_by_48_byte_rows(ctx):
    """33 and 48 bytes share the K-step count (3) and differ in width: FM_EINVAL, and everything still answers afterwards."""
    Q33 = W.pair(33)[0]
    Q48, T48 = W.pair(48)
    _, images48 = W.gallery(48)
    _, images33 = W.gallery(33)
    with _Banks(ctx, Q33, Q48, T48) as (q33, q48, t48), _collection(ctx, images48) as c:
        ctx.hamming_self_dist_batch([q33, q48], want_host=False)
        with ctx.mask(W.NQ, W.NT) as mk, c.mask(W.NQ) as cmk:
            mk.set_all(True)
            for i in range(len(images48)):
                cmk.set_all(True, img=i)
            calls = [
                ("knn2", lambda: ctx.knn2(q33, t48)), ("knn", lambda: ctx.knn(q33, t48, 3)), ("xcheck1", lambda: ctx.xcheck1(q33, t48)),
                ("knn2_ratio", lambda: ctx.knn2_ratio(q33, t48, TAU)), ("knn_masked", lambda: ctx.knn_masked(q33, t48, mk, 2)),
                ("hamming_radius_match", lambda: ctx.hamming_radius_match(q33, t48, 5.0)),
                ("mutual_ratio", lambda: ctx.mutual_ratio(q33, t48, TAU)),
                ("hamming_match_accepted", lambda: ctx.hamming_match_accepted(q33, t48, TAU)),
                ("the other way round", lambda: ctx.knn2(t48, q33)),
                ("collection knn", lambda: c.knn(q33, 2)), ("collection knn2_ratio", lambda: c.knn2_ratio(q33, TAU)),
                ("collection knn2_each", lambda: c.knn2_each(q33)), ("collection votes", lambda: c.votes(q33, TAU)),
                ("collection knn_masked", lambda: c.knn_masked(q33, cmk, 2)),
                ("collection hamming_radius_match", lambda: c.hamming_radius_match(q33, 5.0)),
                ("collection xcheck1_each", lambda: c.xcheck1_each(q33)),
                ("collection mutual_ratio_each", lambda: c.mutual_ratio_each(q33, TAU)),
                ("collection hamming_match_accepted_each", lambda: c.hamming_match_accepted_each(q33, TAU)),
                ("a 33-byte image", lambda: c.add_binary(images33[0])),
            ]
            for what, call in calls:
                _raises_einval(call, what)
            # ... and nothing was disturbed: the same banks, the same collection, the same masks
            ridx, rdist = _knn8(48)
            _same(ctx.knn2(q48, t48), (ridx[:, :2], rdist[:, :2]), "knn2 after the refusals")
            _same(ctx.xcheck1(q48, t48), H.xcheck(Q48, T48), "xcheck1 after the refusals")
            _same(ctx.knn_masked(q48, t48, mk, 3), (ridx[:, :3], rdist[:, :3]), "knn_masked after the refusals")
            assert c.info() == (len(images48), sum(W.IMAGE_SIZES), 48, _ffi.FM_BANK_BIN)
            _same(c.knn(q48, 3), W.stacked_knn(Q48, images48, 3), "collection knn after the refusals")
            _same(c.knn_masked(q48, cmk, 3), W.stacked_knn(Q48, images48, 3), "collection knn_masked after the refusals")
            _same(c.xcheck1_each(q48), XE.xcheck_each(Q48, images48, binary=True), "collection xcheck1_each after the refusals")
        with _Banks(ctx, Q33, W.pair(33)[1]) as (a, b):              # the refused 33-byte query is a good one against 33-byte rows
            r33 = _knn8(33)
            _same(ctx.knn2(a, b), (r33[0][:, :2], r33[1][:, :2]), "33 bytes after the refusals")
    ctx.sync()
