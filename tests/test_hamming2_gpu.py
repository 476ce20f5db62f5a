"""GPU: cv2.BFMatcher(NORM_HAMMING2) on FM_BANK_BIN2 bank pairs (K11b, csrc/hamming2.hip), bit for bit against hamming2_ref.

Widths: both sides of every K-step boundary of the tetrahedral FP4 image (1, 10 | 11, 21 | 22, 32 | 33, 42 | 43, 53 | 54, 64
bytes = 1 .. 6 K steps), which also cross the packed plane's 16-byte pieces at 16, 32 and 48.  Shapes: 300 x 700 rows -- a
second 256-row output chunk with a ragged end, six 128-row stages, a tail stage with 60 real rows, two splits -- and train
banks of 0, 1, 2 and 129 rows, a query bank of 0 rows.  Data: random bytes with planted duplicates, rows that differ in BOTH
bits of a cell (where NORM_HAMMING disagrees), near-duplicates at equal distance on both sides of a stage boundary and in the
tail stage, and a train bank whose only row lies exactly 3 P / 4 from the queries -- the distance of a padding row."""
import ctypes
import functools

import numpy as np
import pytest

import hamming2_ref as H2
import hamming_ref
from fastmatch_amd import _ffi, matchutil

pytestmark = pytest.mark.gpu

WIDTHS = [1, 10, 11, 21, 22, 32, 33, 42, 43, 53, 54, 64]
NQ, NT = 300, 700
EINVAL, EUNSUPPORTED = -1, -4
INF = np.float32(np.inf)


def _flip_cells(row, cells, both):
    """row with the given cells changed: both bits of each (both) or its low bit only."""
    r = row.copy()
    for c in cells:
        r[c >> 2] ^= np.uint8((3 if both else 1) << (2 * (c & 3)))
    return r


@functools.lru_cache(maxsize=None)
def data(nbytes, nq=NQ, nt=NT):
    rng = np.random.default_rng(4200 + nbytes)
    Q = rng.integers(0, 256, (nq, nbytes), dtype=np.uint8)
    T = rng.integers(0, 256, (nt, nbytes), dtype=np.uint8)
    P = 4 * nbytes
    if nq >= 300 and nt >= 700:
        T[10] = Q[3]; T[650] = Q[3]                         # exact duplicates, first and tail stage: d0 = d1 = 0
        T[20] = _flip_cells(Q[4], [0, P - 1], True)         # h2 = 2, popcount 4 ...
        T[21] = _flip_cells(Q[4], [0, 1, P - 1], False)     # ... h2 = 3, popcount 3: the two norms order them differently
        T[127] = _flip_cells(Q[5], [1], True)               # h2 = 1 on both sides of the first stage boundary
        T[128] = _flip_cells(Q[5], [2], False)
        T[255] = _flip_cells(Q[6], [0, 3], True)            # h2 = 2 on both sides of the second
        T[256] = _flip_cells(Q[6], [1, 2], False)
        T[126] = _flip_cells(Q[7], [3], False)              # h2 = 1 in the first stage and in the tail stage
        T[690] = _flip_cells(Q[7], [0], True)
        T[699] = _flip_cells(Q[299], [P - 1], True)         # the last real row of the tail stage, the last query row
    Q.setflags(write=False); T.setflags(write=False)
    return Q, T


@functools.lru_cache(maxsize=None)
def ref(nbytes):
    return H2.Ref(*data(nbytes))


@pytest.fixture(scope="module")
def banks(ctx):
    """(query bank, train bank) per width, uploaded once."""
    made = {}

    def get(nbytes):
        if nbytes not in made:
            Q, T = data(nbytes)
            made[nbytes] = (ctx.bank_binary2(Q), ctx.bank_binary2(T))
        return made[nbytes]
    yield get
    for qb, tb in made.values():
        qb.close(); tb.close()


def _same(got, want, what):
    (gi, gd), (wi, wd) = got, want
    assert np.array_equal(gi, wi), what + " idx"
    assert np.array_equal(H2.bits(gd), H2.bits(wd)), what + " dist"


# ---- 1. every width: knnMatch, crossCheck, the ratio tests ---------------------------------------------------------------------
@pytest.mark.parametrize("nbytes", WIDTHS)
def test_knn_xcheck_and_ratio_tests_at_every_width(ctx, banks, nbytes):
    Q, T = data(nbytes)
    qb, tb = banks(nbytes)
    assert (qb.kind, qb.dim, qb.n, tb.n) == (_ffi.FM_BANK_BIN2, nbytes, NQ, NT)
    w8 = H2.knn(Q, T, 8)
    h2, h = H2.distances(Q, T), hamming_ref.distances(Q, T)
    if nbytes >= 2:     # the planted rows: NORM_HAMMING2 ranks T[20] before T[21], NORM_HAMMING the other way round
        assert (h2[4, 20], h2[4, 21], h[4, 20], h[4, 21]) == (2, 3, 4, 3)
        assert list(w8[0][4, :2]) == [20, 21] and list(w8[0][3, :2]) == [10, 650] and w8[1][3, 1] == 0
        assert list(w8[0][5, :2]) == [127, 128] and list(w8[0][6, :2]) == [255, 256] and list(w8[0][7, :2]) == [126, 690]
        assert w8[0][299, 0] == 699
    if nbytes == 32:    # about a quarter of the random rows tie between rank 0 and rank 1
        assert 0.1 < (w8[1][:, 0] == w8[1][:, 1]).mean() < 0.5
    assert not np.array_equal(w8[0][:, :2], hamming_ref.knn(Q, T, 2)[0])         # a plain-Hamming answer fails
    _same(ctx.knn2(qb, tb), (w8[0][:, :2], w8[1][:, :2]), "knn2")
    _same(ctx.knn(qb, tb, 1), (w8[0][:, :1], w8[1][:, :1]), "knn k = 1")
    _same(ctx.knn(qb, tb, 2), (w8[0][:, :2], w8[1][:, :2]), "knn k = 2")
    _same(ctx.knn(qb, tb, 3), (w8[0][:, :3], w8[1][:, :3]), "knn k = 3")
    _same(ctx.knn(qb, tb, 8), w8, "knn k = 8")
    _same(ctx.xcheck1(qb, tb), H2.xcheck(Q, T), "xcheck1")
    _same(ctx.xcheck1(tb, qb), H2.xcheck(T, Q), "xcheck1, banks swapped")
    wq, wt, wd, wr = H2.ratio_match(Q, T, 0.9)
    gq, gt, gd, gr = ctx.knn2_ratio(qb, tb, 0.9)
    assert 3 not in wq                                                            # d1 == 0: rejected
    assert np.array_equal(gq, wq) and np.array_equal(gt, wt) and np.array_equal(H2.bits(gd), H2.bits(wd)) and np.array_equal(gr, wr)
    for sym in (False, True):
        wq, wt, wd, wr = H2.mutual_ratio(Q, T, 0.9, sym)
        gq, gt, gd, gr = ctx.mutual_ratio(qb, tb, 0.9, sym)
        assert np.array_equal(gq, wq) and np.array_equal(gt, wt) and np.array_equal(H2.bits(gd), H2.bits(wd)) and np.array_equal(gr, wr), sym
        assert len(wq) > 0


# ---- 2. every width: radiusMatch --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbytes", WIDTHS)
def test_radius_match_at_every_width(ctx, banks, nbytes):
    qb, tb = banks(nbytes)
    r = ref(nbytes)
    P = 4 * nbytes
    for rad in (1, 2.5, 3 * P / 4, 3 * P / 4 + 0.5, P, P + 0.5, np.inf):
        H2.same_lists(ctx.hamming_radius_match(qb, tb, np.float32(rad)), r.cut(np.float32(rad)), "%d bytes, r = %r" % (nbytes, rad))
    # r > P admits every real row and no padding row (a padding row sits at 3 P / 4, inside the radius)
    assert np.array_equal(np.diff(ctx.hamming_radius_match(qb, tb, np.float32(P + 0.5))[0]), np.full(NQ, NT))


def _mixed_radii(r, P):
    rng = np.random.default_rng(3)
    rad = np.array([r.sorted[i, rng.integers(0, 40)] for i in range(r.nq)], np.float32)      # H exactly: that distance is outside
    rad[1::3] += np.float32(0.5)                                                             # H + 0.5: inside
    for j, v in enumerate((0.0, np.nan, np.inf, P + 1.0, -2.0)):
        rad[7 + j::37] = v
    return rad


def _raw(ctx, qb, tb, r, cap, size, lists=True):
    """One host call into sentinel-filled arrays: (rc, n_total, offsets, idx, dist)."""
    off = np.full(qb.n + 1, -7, np.int64)
    idx, dist = np.full(size, -78, np.int32), np.full(size, -79.0, np.float32)
    rad = np.ascontiguousarray(r, dtype=np.float32) if np.ndim(r) else None
    p = (lambda a: a.ctypes.data_as(ctypes.c_void_p)) if lists and size else (lambda a: None)
    tot = ctypes.c_int64(-5)
    rc = ctx.lib.fm_hamming_radius_match(ctx.handle, qb.handle, tb.handle, rad.ctypes.data_as(ctypes.c_void_p) if rad is not None else None,
                                         0.0 if rad is not None else float(np.float32(r)), cap, off.ctypes.data_as(ctypes.c_void_p),
                                         p(idx), p(dist), ctypes.byref(tot))
    return rc, tot.value, off, idx, dist


@pytest.mark.parametrize("nbytes", [10, 32, 53, 64])
def test_per_row_radii_counts_cap_and_device_forms(ctx, banks, nbytes):
    import torch
    from fastmatch_amd import torchmatch
    qb, tb = banks(nbytes)
    r = ref(nbytes)
    P = 4 * nbytes
    rad = _mixed_radii(r, P)
    assert np.isnan(rad).sum() >= 3 and np.isinf(rad).sum() >= 3 and (rad == 0).sum() >= 3 and (rad > P).sum() >= 6
    want = r.cut(rad)
    total = int(want[0][-1])
    H2.same_lists(ctx.hamming_radius_match(qb, tb, rad), want, "per-row radii, host form")
    # counts only, then a cap inside a row: the longest prefix of whole rows, n_total and the offsets complete
    rc, tot, off, _, _ = _raw(ctx, qb, tb, rad, 0, 0, lists=False)
    assert rc == 0 and tot == total and np.array_equal(off, want[0])
    row = int(np.nonzero(np.diff(want[0]) >= 2)[0][20])
    mid, k = int(want[0][row]) + 1, int(want[0][row])
    rc, tot, off, idx, dist = _raw(ctx, qb, tb, rad, mid, total)
    assert rc == 0 and tot == total and np.array_equal(off, want[0])
    assert np.array_equal(idx[:k], want[1][:k]) and np.array_equal(H2.bits(dist[:k]), H2.bits(want[2][:k]))
    assert (idx[k:] == -78).all() and (dist[k:] == np.float32(-79.0)).all()
    # the device form through torchmatch: a scalar radius and a tensor of radii, equal to the host form
    for rr, w in ((np.float32(2.5), r.cut(np.float32(2.5))), (torch.from_numpy(rad).cuda(), want)):
        got = tuple(x.cpu().numpy() for x in torchmatch.hamming_radius_match(qb, tb, rr))
        H2.same_lists(got, w, "torchmatch")


# ---- 3. small banks ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbytes", [10, 32, 43, 64])
@pytest.mark.parametrize("nt", [0, 1, 2, 129])
def test_small_train_banks(ctx, banks, nbytes, nt):
    Q, T = data(nbytes)
    T = np.ascontiguousarray(T[:nt])
    qb = banks(nbytes)[0]
    tb = ctx.bank_binary2(T)
    q0 = ctx.bank_binary2(Q[:0])
    try:
        for k in (1, 2, 3, 8):
            got = ctx.knn(qb, tb, k)
            _same(got, H2.knn(Q, T, k), "nt = %d, k = %d" % (nt, k))
            if nt < k:
                assert (got[0][:, nt:] == -1).all() and np.isinf(got[1][:, nt:]).all()
            gi, gd = ctx.knn(q0, tb, k)
            assert gi.shape == gd.shape == (0, k)
        _same(ctx.knn2(qb, tb), H2.knn(Q, T, 2), "knn2")
        _same(ctx.xcheck1(qb, tb), H2.xcheck(Q, T), "xcheck1")
        _same(ctx.xcheck1(tb, qb), H2.xcheck(T, Q), "xcheck1, one real row per stage side")
        for a, b in zip(ctx.knn2_ratio(qb, tb, 0.9), H2.ratio_match(Q, T, 0.9)):
            assert np.array_equal(a, b)
        for sym in (False, True):
            for a, b in zip(ctx.mutual_ratio(qb, tb, 0.9, sym), H2.mutual_ratio(Q, T, 0.9, sym)):
                assert np.array_equal(a, b)
        for rad in (np.inf, 3 * nbytes + 0.5):                      # a padding row's distance is inside both
            got = ctx.hamming_radius_match(qb, tb, np.float32(rad))
            assert np.diff(got[0]).max(initial=0) <= nt
            H2.same_lists(got, H2.radius_match(Q, T, np.float32(rad)), "radius, nt = %d" % nt)
        off, idx, dist = ctx.hamming_radius_match(q0, tb, INF)
        assert off.shape == (1,) and off[0] == 0 and idx.size == dist.size == 0
    finally:
        tb.close(); q0.close()


@pytest.mark.parametrize("nbytes", WIDTHS)
def test_a_real_row_at_the_distance_of_a_padding_row(ctx, nbytes):
    """Every real train row lies exactly 3 P / 4 from every query row, where an all-zero FP4 row decodes to: with nt = 1 and
    k = 2 the second slot must stay empty -- padding is excluded by index, never by value."""
    P = 4 * nbytes
    Q = np.zeros((5, nbytes), np.uint8)
    T = np.full((1, nbytes), 0b00010101, np.uint8)                  # three of the four cells of every byte differ
    assert (H2.distances(Q, T) == 3 * P // 4).all()
    qb, tb = ctx.bank_binary2(Q), ctx.bank_binary2(T)
    try:
        idx, dist = ctx.knn2(qb, tb)
        assert (idx[:, 0] == 0).all() and (dist[:, 0] == 3 * P / 4).all()
        assert (idx[:, 1] == -1).all() and np.isinf(dist[:, 1]).all()
        tidx, tdist = ctx.xcheck1(qb, tb)
        assert list(tidx) == [0, -1, -1, -1, -1] and tdist[0] == 3 * P / 4
        off, ridx, _ = ctx.hamming_radius_match(qb, tb, np.float32(3 * P / 4 + 0.5))
        assert np.array_equal(off, np.arange(6)) and not ridx.any()
        off, _, _ = ctx.hamming_radius_match(qb, tb, np.float32(3 * P / 4))
        assert not off.any()
    finally:
        qb.close(); tb.close()


# ---- 4. device banks and device results ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbytes", [21, 32, 64])
def test_torchmatch_device_banks_and_results(ctx, banks, nbytes):
    import torch
    from fastmatch_amd import torchmatch
    Q, T = data(nbytes)
    wide = torch.zeros((NQ, nbytes + 5), dtype=torch.uint8, device="cuda")
    wide[:, 2:2 + nbytes] = torch.from_numpy(np.array(Q)).cuda()
    qb = torchmatch.bank(wide[:, 2:2 + nbytes], hamming2=True, context=ctx)          # pitched rows, read in place
    tb = torchmatch.bank(torch.from_numpy(np.array(T)).cuda(), hamming2=True, context=ctx)
    try:
        assert qb.kind == tb.kind == _ffi.FM_BANK_BIN2 and qb.dim == nbytes
        for k in (1, 2, 3, 8):
            gi, gd = torchmatch.knn(qb, tb, k)
            _same((gi.cpu().numpy(), gd.cpu().numpy()), H2.knn(Q, T, k), "torchmatch.knn k = %d" % k)
        gi, gd = torchmatch.mutual_nn(qb, tb)
        _same((gi.cpu().numpy(), gd.cpu().numpy()), H2.xcheck(Q, T), "torchmatch.mutual_nn")
        wq, wt, wd, _ = H2.ratio_match(Q, T, 0.9)
        gq, gt, gd = (x.cpu().numpy() for x in torchmatch.ratio_match(qb, tb, 0.9))
        assert np.array_equal(gq, wq) and np.array_equal(gt, wt) and np.array_equal(H2.bits(gd), H2.bits(wd))
        for sym in (False, True):
            wq, wt, wd, _ = H2.mutual_ratio(Q, T, 0.9, sym)
            gq, gt, gd = (x.cpu().numpy() for x in torchmatch.mutual_ratio_match(qb, tb, 0.9, symmetric=sym))
            assert np.array_equal(gq, wq) and np.array_equal(gt, wt) and np.array_equal(H2.bits(gd), H2.bits(wd))
        # refusals of the tensor layer: ValueError, nothing reaches the library
        m = torch.ones((NQ, NT), dtype=torch.bool, device="cuda")
        for call in (lambda: torchmatch.knn(qb, tb, 2, mask=m), lambda: torchmatch.radius_match(qb, tb, 3.0),
                     lambda: torchmatch.radius_match(qb, tb, 3.0, mask=m), lambda: torchmatch.hamming_radius_match(qb, tb, 3.0, mask=m),
                     lambda: torchmatch.hamming_radius_match(qb, torch.from_numpy(np.array(T)).cuda(), 3.0),
                     lambda: torchmatch.Collection(context=ctx).add(torch.from_numpy(np.array(T)).cuda(), hamming2=True),
                     lambda: torchmatch.bank(wide, hamming2=True, binary=True, context=ctx)):
            with pytest.raises(ValueError):
                call()
        with torchmatch.Collection(context=ctx) as coll:
            coll.add(torch.from_numpy(np.array(T)).cuda(), binary=True)
            for call in (lambda: coll.knn(qb, 2), lambda: coll.ratio_match(qb, 0.9), lambda: coll.hamming_radius_match(qb, 3.0)):
                with pytest.raises(ValueError):
                    call()
    finally:
        qb.close(); tb.close()


# ---- 5. matchutil -----------------------------------------------------------------------------------------------------------
def test_matchutil_equals_the_array_forms(ctx, banks):
    Q, T = data(32)
    qb, tb = banks(32)
    opts = {"context": ctx}
    w8 = H2.knn(Q, T, 8)
    for k in (1, 2, 3, 8):
        for a, b in ((Q, T), (qb, tb), (Q, tb)):
            _same(matchutil.hamming2_match_arrays(a, b, k=k, options=opts), (w8[0][:, :k], w8[1][:, :k]), "k = %d" % k)
    _same(matchutil.hamming2_match_arrays(Q, T, k=1, options=dict(opts, crossCheck=True)), H2.xcheck(Q, T), "crossCheck")
    lists = matchutil.hamming2_match(Q, T, k=2, options=opts)
    assert [[(m.queryIdx, m.trainIdx, m.distance) for m in row] for row in lists] == \
           [[(i, int(w8[0][i, j]), float(w8[1][i, j])) for j in range(2)] for i in range(NQ)]
    for a, b in zip(matchutil.hamming2_ratio_match_arrays(Q, T, 0.9, options=opts), H2.ratio_match(Q, T, 0.9)):
        assert np.array_equal(a, b)
    for sym in (False, True):
        for a, b in zip(matchutil.hamming2_mutual_ratio_match_arrays(Q, tb, 0.9, symmetric=sym, options=opts), H2.mutual_ratio(Q, T, 0.9, sym)):
            assert np.array_equal(a, b)
    want = ref(32).cut(np.float32(2.5))
    H2.same_lists(matchutil.hamming2_radius_match_arrays(Q, T, 2.5, options=opts), want, "radius arrays")
    rl = matchutil.hamming2_radius_match(qb, tb, 2.5, options=opts)
    assert [[m.trainIdx for m in row] for row in rl] == [list(want[1][want[0][i]:want[0][i + 1]]) for i in range(NQ)]
    # cv2's factory
    m = matchutil.BFMatcher_create(matchutil.NORM_HAMMING2, options=opts)
    assert [[x.trainIdx for x in row] for row in m.knnMatch(Q, T, k=2)] == [list(w8[0][i, :2]) for i in range(NQ)]
    assert [x.trainIdx for x in m.match(Q, T)] == list(w8[0][:, 0])
    assert [[x.trainIdx for x in row] for row in m.radiusMatch(Q, T, 2.5)] == [[x.trainIdx for x in row] for row in rl]
    mx = matchutil.BFMatcher_create(matchutil.NORM_HAMMING2, crossCheck=True, options=opts)
    xt, _ = H2.xcheck(Q, T)
    assert [(x.queryIdx, x.trainIdx) for x in mx.match(Q, T)] == [(i, int(t)) for i, t in enumerate(xt) if t >= 0]
    # a NORM_HAMMING2 bank in the calls of the other norms, a NORM_HAMMING bank here: ValueError
    hb = ctx.bank_binary(np.array(Q))
    try:
        for call in (lambda: matchutil.bf_match(qb, tb, k=1, options=opts), lambda: matchutil.bf_match(qb, tb, k=1, options=dict(opts, normType=6)),
                     lambda: matchutil.hamming_radius_match(qb, tb, 3.0, options=opts), lambda: matchutil.hamming2_match(hb, tb, options=opts),
                     lambda: matchutil.hamming2_radius_match(qb, hb, 3.0, options=opts)):
            with pytest.raises(ValueError):
                call()
    finally:
        hb.close()


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------
PAIR = ["fm_radius_match", "fm_radius_match_dev", "fm_wide_radius_match", "fm_wide_radius_match_dev", "fm_match_ratio", "fm_match_accepted",
        "fm_match_accepted_async", "fm_match_accepted_dev", "fm_match_accepted_dev_async", "fm_hamming_match_ratio", "fm_hamming_match_accepted",
        "fm_hamming_match_accepted_dev", "fm_wide_match_ratio", "fm_wide_match_accepted", "fm_wide_match_accepted_dev", "fm_xcheck1_keys",
        "fm_xcheck1_keys_dev"]
PAIR_MASKED = ["fm_knn_masked", "fm_knn_masked_dev", "fm_wide_knn_masked", "fm_wide_knn_masked_dev", "fm_radius_match_masked",
               "fm_radius_match_masked_dev"]
ONE = ["fm_self_dist", "fm_bank_set_selfdist", "fm_hamming_self_dist", "fm_hamming_set_selfdist", "fm_wide_self_dist", "fm_wide_set_selfdist",
       "fm_bank_append_u8", "fm_bank_append_f32", "fm_bank_refill_u8_async"]
BATCH_ONE = ["fm_self_dist_batch", "fm_hamming_self_dist_batch", "fm_wide_self_dist_batch"]
BATCH_PAIR = ["fm_match_accepted_batch", "fm_match_accepted_dev_batch"]
COLL = ["fm_collection_knn", "fm_collection_knn_dev", "fm_collection_knn2_ratio", "fm_collection_knn2_ratio_dev", "fm_collection_radius_match",
        "fm_collection_radius_match_dev", "fm_collection_hamming_radius_match", "fm_collection_hamming_radius_match_dev",
        "fm_collection_wide_radius_match", "fm_collection_wide_radius_match_dev", "fm_collection_knn2_each", "fm_collection_votes",
        "fm_collection_wide_knn", "fm_collection_wide_knn_dev", "fm_collection_wide_knn2_ratio", "fm_collection_wide_knn2_ratio_dev",
        "fm_collection_wide_votes", "fm_collection_match_accepted_each", "fm_collection_match_accepted_each_dev",
        "fm_collection_hamming_match_accepted_each", "fm_collection_hamming_match_accepted_each_dev", "fm_collection_wide_match_accepted_each",
        "fm_collection_wide_match_accepted_each_dev", "fm_collection_xcheck1_each", "fm_collection_xcheck1_each_dev",
        "fm_collection_mutual_ratio_each", "fm_collection_mutual_ratio_each_dev", "fm_collection_wide_knn2_each",
        "fm_collection_wide_mutual_ratio_each", "fm_collection_wide_mutual_ratio_each_dev"]
COLL_MASKED = ["fm_collection_knn_masked", "fm_collection_knn_masked_dev", "fm_collection_radius_match_masked",
               "fm_collection_radius_match_masked_dev"]
SERVED = ["fm_knn2", "fm_knn", "fm_xcheck1", "fm_knn2_ratio", "fm_mutual_ratio", "fm_knn_dev", "fm_xcheck1_dev", "fm_knn2_ratio_dev",
          "fm_mutual_ratio_dev", "fm_hamming_radius_match", "fm_hamming_radius_match_dev"]


class _Caller(object):
    """Calls a C entry point by name with the given handles in its first pointer arguments behind ctx; every other pointer gets
    a table of pointers to a scratch buffer (valid as an array and as an array of arrays), every integer `ints`' value or 1 for
    a leading count, every float 0.  A refused call returns before it looks at any of them."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.scratch = ctypes.create_string_buffer(1 << 16)
        self.table = (ctypes.c_void_p * 1024)(*([ctypes.addressof(self.scratch)] * 1024))

    def __call__(self, name, handles, first_int=0):
        _, argtypes = _ffi.SYMBOLS[name]
        args, hs, ints = [self.ctx.handle], list(handles), 0
        for t in argtypes[1:]:
            if t is ctypes.c_void_p or issubclass(t, ctypes._Pointer):
                args.append(ctypes.cast(hs.pop(0) if hs else self.table, t))
            elif t in (ctypes.c_float, ctypes.c_double):
                args.append(0.0)
            else:
                args.append(first_int if ints == 0 else 0)
                ints += 1
        assert not hs, name
        return getattr(self.ctx.lib, name)(*args)


def _last_error(ctx):
    return (ctx.lib.fm_last_error(ctx.handle) or b"").decode()


def test_every_other_entry_point_refuses(ctx, banks):
    Q, T = data(32, 4, 9)
    q2, t2 = ctx.bank_binary2(Q), ctx.bank_binary2(T)
    qh, th = ctx.bank_binary(Q), ctx.bank_binary(T)
    q8, t8 = ctx.bank(np.zeros((4, 32), np.uint8)), ctx.bank(np.zeros((9, 32), np.uint8))
    e2 = ctx.bank_binary2(Q[:0])
    coll = ctx.collection()
    coll.add_binary(T)
    mask, cmask = ctx.mask(4, 9), coll.mask(4)
    call = _Caller(ctx)

    def refused(rc, code, name):
        assert rc == code and "NORM_HAMMING2" in _last_error(ctx), (name, rc, _last_error(ctx))

    def array(*hs):
        return (ctypes.c_void_p * len(hs))(*[h.handle.value for h in hs])
    try:
        for name in PAIR:
            refused(call(name, [q2.handle, t2.handle]), EUNSUPPORTED, name)
        refused(call("fm_xcheck1_batched", [q2.handle, call.table, call.table, t2.handle]), EUNSUPPORTED, "fm_xcheck1_batched")
        for name in PAIR_MASKED:
            refused(call(name, [q2.handle, t2.handle, mask.handle], first_int=1), EUNSUPPORTED, name)
        for name in ONE:
            refused(call(name, [q2.handle]), EUNSUPPORTED, name)
        for name in BATCH_ONE:
            refused(call(name, [array(q2)], first_int=1), EUNSUPPORTED, name)
        for name in BATCH_PAIR:
            refused(call(name, [array(q2), array(t2)], first_int=1), EUNSUPPORTED, name)
        for name in COLL:
            refused(call(name, [coll.handle, q2.handle], first_int=1), EUNSUPPORTED, name)
        for name in COLL_MASKED:
            refused(call(name, [coll.handle, q2.handle, cmask.handle], first_int=1), EUNSUPPORTED, name)
        # fm_collection_add_dev with FM_DT_BIN2: (ctx, c, d_rows, dtype, ...)
        import torch
        d = torch.zeros((9, 32), dtype=torch.uint8, device="cuda")
        rc = ctx.lib.fm_collection_add_dev(ctx.handle, coll.handle, ctypes.c_void_p(d.data_ptr()), _ffi.FM_DT_BIN2, 9, 32, 0, None, None)
        refused(rc, EUNSUPPORTED, "fm_collection_add_dev")
        # a NORM_HAMMING2 bank beside any other kind, empty banks included: FM_EINVAL at the served calls
        for a, b in ((q2, th), (qh, t2), (q2, t8), (q8, t2), (e2, th), (e2, t8)):
            for name in SERVED:
                refused(call(name, [a.handle, b.handle], first_int=1), EINVAL, name)
        # the norm of the same width is served as before, and a served call afterwards still gives the right answer
        _same(ctx.knn2(qh, th), hamming_ref.knn(Q, T, 2), "NORM_HAMMING pair")
        _same(ctx.knn2(q2, t2), H2.knn(Q, T, 2), "NORM_HAMMING2 pair after the refusals")
        _same(ctx.knn(q2, t2, 3), H2.knn(Q, T, 3), "k = 3 after the refusals")
        H2.same_lists(ctx.hamming_radius_match(q2, t2, np.float32(40.5)), H2.radius_match(Q, T, np.float32(40.5)), "radius after the refusals")
    finally:
        for x in (mask, cmask, coll, q2, t2, qh, th, q8, t8, e2):
            x.close()
