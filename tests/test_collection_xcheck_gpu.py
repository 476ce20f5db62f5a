"""GPU: crossCheck on a train collection, image by image (fm_collection_xcheck1_each, its device form, Collection.mutual_votes,
BFMatcher.matchEach, torchmatch.Collection.mutual_nn_each), bit for bit against
  * the NumPy reference (tests/xcheck_each_ref.py: the oracle / hamming_ref per image, the max_dist filter, the compaction),
  * Context.xcheck1(q, bank(image_i)) -- code older than the collection form."""
import os
import sys

import numpy as np
import pytest

from fastmatch_amd import _ffi, matchutil, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f32_regimes                              # noqa: E402
import xcheck_each_ref as ref                   # noqa: E402
from kat import far_banks, SQRT_TIE_MIN         # noqa: E402

pytestmark = pytest.mark.gpu

EINVAL, EUNSUP = -1, -4
BOUNDARY_SIZES = [0, 1, 127, 128, 129, 1000, 5, 0]      # on a stage boundary, one row past it, empty first / middle / last
NQS = (0, 1, 100, 700)              # 700 rows pad to 768: the reverse sweep splits the reduced range in two
KINDS = ("u8", "f32int", "f32", "f32nofilter", "bin1", "bin32", "bin64")
NAN = float("nan")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want, what):
    assert np.array_equal(got[0], want[0]), what + ": train rows"
    assert np.array_equal(_bits(got[1]), _bits(want[1])), what + ": distances"


def _plant(images, Q, rng, noisy):
    """Ties and matches: a row twice in one image, once more in another image, duplicated query rows, and query rows that
    are (noisy) copies of image rows, so that mutual nearest neighbours exist in every non-empty image."""
    big, small = images[5], images[4]
    big[7] = big[3]                  # twice in one image: the lowest row wins
    small[0] = big[3]                # ... and in another image: both images report it
    nq = Q.shape[0]
    for j in range(0, nq, 3):        # one query row in three copies an image row (every non-empty image in turn)
        im = images[(1, 2, 3, 4, 5, 6)[(j // 3) % 6]]
        Q[j] = noisy(im[(j * 7) % im.shape[0]])
    Q[10] = big[3]; Q[20] = big[3]   # duplicated query rows: a train row elects the lower index
    if nq > 1:
        Q[0] = Q[1]


def _data(kind):
    """(images, Q [700], binary, float_route) of a kind; deterministic."""
    rng = np.random.default_rng(2100 + KINDS.index(kind))
    nq = max(NQS)
    if kind.startswith("bin"):
        w = int(kind[3:])
        images = [rng.integers(0, 256, (n, w), dtype=np.uint8) for n in BOUNDARY_SIZES]
        Q = rng.integers(0, 256, (nq, w), dtype=np.uint8)

        def noisy(row):
            out = row.copy()
            out[rng.integers(0, w)] ^= np.uint8(1 << rng.integers(0, 8))
            return out
        _plant(images, Q, rng, noisy)
        return images, Q, True, False
    if kind in ("u8", "f32int"):
        images = [synth.synth_sift(max(n, 1), rng)[:n].copy() for n in BOUNDARY_SIZES]
        Q = synth.synth_sift(nq, rng)
        _plant(images, Q, rng, lambda row: np.clip(row.astype(np.int32) + rng.integers(-3, 4, row.shape), 0, 255).astype(np.uint8))
        if kind == "f32int":         # integer-valued float32: the integer route
            images, Q = [im.astype(np.float32) for im in images], Q.astype(np.float32)
        return images, Q, False, False
    # non-integer float32 (N(0, 1) rows, tests/f32_regimes.py): the float32 route
    images = [f32_regimes._gauss(2200 + i, n).astype(np.float32) for i, n in enumerate(BOUNDARY_SIZES)]
    Q = f32_regimes._gauss(2300, nq).astype(np.float32)
    _plant(images, Q, rng, lambda row: (row + rng.normal(0.0, 0.01, row.shape)).astype(np.float32))
    if kind == "f32nofilter":
        # an image 2^20 times the others' scale (f32_regimes.qt_apart: Q of that pair) leaves fp16's range under the
        # collection's scale and switches the filter off for the collection
        far = f32_regimes.qt_apart(45)[0][:127].copy()
        assert np.abs(far).max() > 60000.0 * np.abs(images[5]).max()
        images[2] = far
    return images, Q, False, True


def _qbank(ctx, Q, binary, float_route):
    return ctx.bank_binary(Q) if binary else ctx.bank(Q, float_route=float_route)


def _collection(ctx, images, binary):
    c = ctx.collection()
    for i, im in enumerate(images):
        assert (c.add_binary(im) if binary else c.add(im)) == i
    return c


def _per_image(ctx, qb, images, binary, float_route):
    """Context.xcheck1 image by image (an empty image: nothing to elect)."""
    tidx, dist = np.full((len(images), qb.n), -1, np.int32), np.full((len(images), qb.n), np.inf, np.float32)
    for i, im in enumerate(images):
        if im.shape[0] == 0 or qb.n == 0:
            continue
        tb = _qbank(ctx, im, binary, float_route)
        tidx[i], dist[i] = ctx.xcheck1(qb, tb)
        tb.close()
    return tidx, dist


class _Case(object):
    pass


_CASES = {}


@pytest.fixture(scope="module")
def case(ctx):
    """kind -> the boundary collection of the kind, its query banks and both references, made once and left unchanged."""
    def get(kind):
        if kind in _CASES:
            return _CASES[kind]
        k = _Case()
        k.images, k.Q, k.binary, k.float_route = _data(kind)
        k.coll = _collection(ctx, k.images, k.binary)
        want_kind = _ffi.FM_BANK_BIN if k.binary else _ffi.FM_BANK_F32 if k.float_route else _ffi.FM_BANK_I8
        assert k.coll.info()[3] == want_kind, kind
        k.qb, k.ref, k.pairs = {}, {}, {}
        for nq in NQS:
            Q = k.Q[:nq]
            k.qb[nq] = _qbank(ctx, Q, k.binary, k.float_route)
            k.ref[nq] = ref.xcheck_each(Q, k.images, k.binary)
        _CASES[kind] = k
        return k
    yield get
    for k in _CASES.values():
        k.coll.close()
        for b in k.qb.values():
            b.close()
    _CASES.clear()


def _filter_option(kind):
    """The fp16 filter forced wherever the banks allow it (the library leaves shapes as small as this file's to the all-pairs
    kernel otherwise): it runs for "f32" and cannot for "f32nofilter"."""
    return 2 if kind in ("f32", "f32nofilter") else 1


def _limit(k, nq):
    """A max_dist that drops about half of the matches of the case: the median of the reported distances."""
    tidx, dist = k.ref[nq]
    return float(np.median(dist[tidx >= 0]))


# ---- image boundaries, kinds, ties --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", NQS)
@pytest.mark.parametrize("kind", KINDS)
def test_image_boundaries(ctx, case, kind, nq):
    k = case(kind)
    qb = k.qb[nq]
    try:
        ctx.set_option("f32_filter", _filter_option(kind))
        before = ctx.f32_filter_stats()[0]
        got = k.coll.xcheck1_each(qb)
        filtered = ctx.f32_filter_stats()[0] - before
        assert got[0].shape == (len(BOUNDARY_SIZES), nq) and got[1].shape == (len(BOUNDARY_SIZES), nq)
        _same(got, k.ref[nq], "%s nq=%d against the reference" % (kind, nq))
        if nq not in k.pairs:
            k.pairs[nq] = _per_image(ctx, qb, k.images, k.binary, k.float_route)
        _same(got, k.pairs[nq], "%s nq=%d against Context.xcheck1 per image" % (kind, nq))
        votes = k.coll.mutual_votes(qb)
    finally:
        ctx.set_option("f32_filter", 1)
    assert np.array_equal(votes, ref.counts(got[0]))
    assert (got[0][0] == -1).all() and np.isinf(got[1][7]).all()           # an empty image keeps its slot, all -1 / inf
    if nq >= 100:
        assert votes[5] > 10 and votes[1] == 1                  # matches exist; the one-row image elects somebody
        if kind == "f32":
            assert filtered > 0                                  # the fp16 filter ran
        if kind == "f32nofilter":
            assert filtered == 0                                 # ... and here it could not
    if nq > 1:
        assert (got[0][:, 1] == -1).all()                       # of two equal query rows (0 and 1) only the first is elected
    if nq == 700 and kind != "bin1":                            # (one byte: a lower query row holds the same value)
        # the planted ties: the duplicated row matches the LOWER of the two equal query rows, at its LOWEST train row, in
        # both images that hold it
        assert got[0][5][10] == 3 and got[0][4][10] == 0 and got[1][5][10] == 0.0 and got[1][4][10] == 0.0
        assert got[0][5][20] != 3 and got[0][5][20] != 7 and got[0][4][20] != 0


def test_float32_root_ties_in_one_image_of_several(ctx):
    """One image in the range where two d2 share a float32 root (kat.far_banks: every distance of the pair lies there) between
    images far below it: the chunk has a tie list, only that image can reach it."""
    rng = np.random.default_rng(2400)
    Q, far = far_banks(300, 500, rng)
    near0 = np.zeros((400, 128), np.uint8)
    near0[:, 101:111] = rng.integers(0, 3, (400, 10), dtype=np.uint8)
    near1 = near0[::-1][:129].copy()
    images = [near0, far, near1]
    assert int((far.astype(np.int64) ** 2).sum(1).max()) >= SQRT_TIE_MIN > int((near0.astype(np.int64) ** 2).sum(1).max()) + 4 * 128
    qb = ctx.bank(Q)
    want = ref.xcheck_each(Q, images)
    with _collection(ctx, images, False) as c:
        got = c.xcheck1_each(qb)
        _same(got, want, "tie range against the reference")
        _same(got, _per_image(ctx, qb, images, False, False), "tie range against Context.xcheck1")
        assert ref.counts(got[0]).min() > 0 and got[1][1][got[0][1] >= 0].min() ** 2 >= SQRT_TIE_MIN - 1
        try:                         # ... and with the far image in a chunk of its own
            ctx.set_option("coll_ws_bytes", 1)
            _same(c.xcheck1_each(qb), want, "tie range, one image per chunk")
        finally:
            ctx.set_option("coll_ws_bytes", 0)
    qb.close()


# ---- chunks -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["u8", "f32", "bin32"])
def test_chunks_of_images(ctx, case, kind):
    k = case(kind)
    nq = 700
    qb = k.qb[nq]
    assert ctx.get_option("coll_ws_bytes") == 0
    per_image = nq * 17 + 3 * 4
    md = _limit(k, nq)
    try:
        for budget, chunk in ((per_image, 1), (3 * per_image + 100, 3)):
            ctx.set_option("coll_ws_bytes", budget)
            assert budget // per_image == chunk
            _same(k.coll.xcheck1_each(qb), k.ref[nq], "%s: %d image(s) per chunk" % (kind, chunk))
            assert np.array_equal(k.coll.mutual_votes(qb), ref.counts(k.ref[nq][0]))
            _same(k.coll.xcheck1_each(qb, md), ref.keep(*k.ref[nq], max_dist=md), "%s: %d image(s) per chunk, max_dist" % (kind, chunk))
    finally:
        ctx.set_option("coll_ws_bytes", 0)


# ---- max_dist -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["u8", "f32", "bin32", "bin1"])
def test_max_dist(ctx, case, kind):
    k = case(kind)
    nq = 700
    qb = k.qb[nq]
    tidx, dist = k.ref[nq]
    reported = np.unique(dist[tidx >= 0])
    equal = float(reported[len(reported) // 2])                 # a reported distance: strict "<" drops it
    assert (dist[tidx >= 0] < equal).any() or kind == "bin1"
    ni = len(k.images)
    for md in (float("inf"), equal, 0.0, NAN, -1.0):
        want = ref.keep(tidx, dist, md)
        got = k.coll.xcheck1_each(qb, md)
        _same(got, want, "%s max_dist=%r" % (kind, md))
        if md == equal:
            assert not (got[1] == np.float32(equal)).any() and (dist == np.float32(equal)).any()
        if md in (0.0, -1.0) or md != md:
            assert (got[0] == -1).all()
        # counts with the dense arrays, and counts only (both arrays NULL)
        n = np.full(ni, -7, np.int64)
        t2, d2 = np.full((ni, nq), -7, np.int32), np.full((ni, nq), -7, np.float32)
        ctx._check(ctx.lib.fm_collection_xcheck1_each(ctx.handle, k.coll.handle, qb.handle, md, t2.ctypes.data, d2.ctypes.data, n.ctypes.data))
        _same((t2, d2), want, "%s max_dist=%r, with counts" % (kind, md))
        assert np.array_equal(n, ref.counts(want[0]))
        n0 = np.full(ni, -7, np.int64)
        ctx._check(ctx.lib.fm_collection_xcheck1_each(ctx.handle, k.coll.handle, qb.handle, md, None, None, n0.ctypes.data))
        assert np.array_equal(n0, n)
        assert np.array_equal(k.coll.mutual_votes(qb, md), n)


# ---- device form --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["u8", "f32", "bin32"])
def test_device_form(ctx, case, kind):
    import torch
    k = case(kind)
    nq = 700
    qb = k.qb[nq]
    ni = len(k.images)
    stream = torch.cuda.current_stream().cuda_stream
    for md in (float("inf"), _limit(k, nq)):
        dense = k.coll.xcheck1_each(qb, md)
        full = ref.counts(dense[0])
        assert full.max() > 3
        for cap in (nq, 3, 0):
            want_rows, want_cnt, want_full = ref.compact(dense[0], dense[1], cap)
            rows = torch.full((ni, max(cap, 1), 3), -7, dtype=torch.int32, device="cuda")
            counts = torch.full((ni,), -7, dtype=torch.int64, device="cuda")
            h = np.full(ni, -7, np.int64)
            k.coll.xcheck1_each_dev(qb, md, rows.data_ptr() if cap else 0, counts.data_ptr(), cap, h_counts=h, consumer_stream=stream)
            assert np.array_equal(h, want_full) and np.array_equal(h, full)
            assert np.array_equal(counts.cpu().numpy(), want_cnt)
            if cap:
                assert np.array_equal(rows.cpu().numpy(), want_rows), "%s cap=%d" % (kind, cap)
            else:
                assert (rows.cpu().numpy() == -7).all()
            # h_counts NULL: enqueued only; the outputs are read behind the call on the same stream
            rows.fill_(-7); counts.fill_(-7)
            k.coll.xcheck1_each_dev(qb, md, rows.data_ptr() if cap else 0, counts.data_ptr(), cap, consumer_stream=stream)
            assert np.array_equal(counts.cpu().numpy(), want_cnt)
            if cap:
                assert np.array_equal(rows.cpu().numpy(), want_rows)
    # nq = 0: zero counts and nothing else
    counts = torch.full((ni,), -7, dtype=torch.int64, device="cuda")
    h = np.full(ni, -7, np.int64)
    k.coll.xcheck1_each_dev(k.qb[0], float("inf"), 0, counts.data_ptr(), 0, h_counts=h, consumer_stream=stream)
    assert (counts.cpu().numpy() == 0).all() and (h == 0).all()


def test_device_outputs_behind_work_on_the_current_stream(ctx, case):
    """The output tensors are still being written by earlier work of a side stream when the call is made; no synchronize()
    between that work, the call and the kernels that consume the results."""
    import torch
    k = case("u8")
    nq = 700
    ni = len(k.images)
    want_rows, want_cnt, _ = ref.compact(*k.ref[nq])
    g = torch.Generator(device="cuda").manual_seed(5)
    A = torch.randn(2048, 2048, device="cuda", generator=g)
    rows = torch.empty((ni, nq, 3), dtype=torch.int32, device="cuda")
    counts = torch.empty(ni, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    s1 = torch.cuda.Stream()
    with torch.cuda.stream(s1):
        B = A
        for _ in range(8):                                     # milliseconds of work in front of the fills below
            B = torch.tanh(B @ A * 0.01)
        rows.fill_(-7); counts.fill_(-7)                       # must land BEFORE the library's rows
        k.coll.xcheck1_each_dev(k.qb[nq], float("inf"), rows.data_ptr(), counts.data_ptr(), nq, consumer_stream=s1.cuda_stream)
        got_rows, got_counts = rows.clone(), counts.clone()    # consumed on s1 with no host synchronisation
    s1.synchronize()
    assert np.array_equal(got_counts.cpu().numpy(), want_cnt) and np.array_equal(got_rows.cpu().numpy(), want_rows)


@pytest.mark.parametrize("kind", ["u8", "f32", "bin32"])
def test_torchmatch_mutual_nn_each_from_tensors(ctx, case, kind):
    import torch
    from fastmatch_amd import torchmatch
    k = case(kind)
    nq = 100
    dense = ref.keep(*k.ref[nq], max_dist=np.inf)
    with torchmatch.Collection(context=ctx) as tc:
        for i, im in enumerate(k.images):
            assert tc.add(torch.from_numpy(im).cuda(), binary=k.binary) == i
        q = torch.from_numpy(k.Q[:nq].copy()).cuda()
        md = _limit(k, nq)
        for cap, limit in ((None, None), (2, None), (None, md)):
            rows, counts = tc.mutual_nn_each(q, max_dist=limit, cap=cap)
            assert rows.is_cuda and rows.dtype == torch.int32 and counts.dtype == torch.int64
            assert tuple(rows.shape) == (len(k.images), nq if cap is None else cap, 3)
            kept = dense if limit is None else ref.keep(*dense, max_dist=limit)
            w, c, _ = ref.compact(kept[0], kept[1], cap)
            cnt = counts.cpu().numpy()
            assert np.array_equal(cnt, c), kind
            r = rows.cpu().numpy()
            for i in range(len(k.images)):
                assert np.array_equal(r[i, :cnt[i]], w[i, :cnt[i]]), "%s image %d" % (kind, i)
        # ... and the _ffi device form on the same collection
        qb = k.qb[nq]
        ni = len(k.images)
        rows2 = torch.full((ni, nq, 3), -7, dtype=torch.int32, device="cuda")
        counts2 = torch.full((ni,), -7, dtype=torch.int64, device="cuda")
        tc._coll.xcheck1_each_dev(qb, float("inf"), rows2.data_ptr(), counts2.data_ptr(), nq,
                                  consumer_stream=torch.cuda.current_stream().cuda_stream)
        rows, counts = tc.mutual_nn_each(qb)
        assert np.array_equal(counts.cpu().numpy(), counts2.cpu().numpy())
        cnt = counts.cpu().numpy()
        for i in range(ni):
            assert np.array_equal(rows[i, :cnt[i]].cpu().numpy(), rows2[i, :cnt[i]].cpu().numpy())


# ---- BFMatcher.matchEach -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cross", [False, True])
@pytest.mark.parametrize("kind", ["u8", "bin32"])
def test_match_each_equals_the_loop_over_images(ctx, case, kind, cross):
    k = case(kind)
    Q = k.Q[:100]
    norm = matchutil.NORM_HAMMING if k.binary else matchutil.NORM_L2
    m = matchutil.BFMatcher(norm, crossCheck=cross)
    m.add(k.images)
    got = m.matchEach(Q)
    tidx, dist = m.matchEach_arrays(Q)
    assert len(got) == len(k.images) and tidx.shape == (len(k.images), 100)
    total = 0
    for i, im in enumerate(k.images):
        if im.shape[0] == 0:
            assert got[i] == [] and (tidx[i] == -1).all()
            continue
        want = [r[0] for r in matchutil.bf_match(Q, im, k=1, options={"normType": norm, "crossCheck": cross}) if r]
        assert [(d.queryIdx, d.trainIdx, d.imgIdx) for d in got[i]] == [(d.queryIdx, d.trainIdx, i) for d in want], (kind, cross, i)
        assert np.array_equal(_bits([d.distance for d in got[i]]), _bits([d.distance for d in want]))
        assert [d.queryIdx for d in got[i]] == np.nonzero(tidx[i] >= 0)[0].tolist()
        total += len(want)
    assert total > 10
    if cross:
        _same((tidx, dist), k.ref[100], "matchEach_arrays")


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_collection_usable(ctx, case):
    import torch
    k = case("u8")
    f = case("f32")
    qb = k.qb[100]
    ni = len(k.images)
    lib, h = ctx.lib, ctx.handle
    t, d = np.zeros((ni, 100), np.int32), np.zeros((ni, 100), np.float32)
    n = np.zeros(ni, np.int64)
    rows = torch.zeros((ni, 4, 3), dtype=torch.int32, device="cuda")
    counts = torch.zeros(ni, dtype=torch.int64, device="cuda")
    inf = float("inf")
    P = lambda a: a.ctypes.data
    # NULL handles
    assert lib.fm_collection_xcheck1_each(h, None, qb.handle, inf, P(t), P(d), P(n)) == EINVAL
    assert lib.fm_collection_xcheck1_each(h, k.coll.handle, None, inf, P(t), P(d), P(n)) == EINVAL
    assert lib.fm_collection_xcheck1_each_dev(h, None, qb.handle, inf, 4, rows.data_ptr(), counts.data_ptr(), None, None) == EINVAL
    # a query of another kind, of another width
    assert lib.fm_collection_xcheck1_each(h, k.coll.handle, f.qb[100].handle, inf, P(t), P(d), P(n)) == EINVAL
    assert lib.fm_collection_xcheck1_each(h, f.coll.handle, qb.handle, inf, P(t), P(d), P(n)) == EINVAL
    narrow = ctx.bank(k.Q[:100, :64].copy())
    assert lib.fm_collection_xcheck1_each(h, k.coll.handle, narrow.handle, inf, P(t), P(d), P(n)) == EINVAL
    assert lib.fm_collection_xcheck1_each_dev(h, k.coll.handle, narrow.handle, inf, 4, rows.data_ptr(), counts.data_ptr(), None, None) == EINVAL
    narrow.close()
    # a float32-route query above FM_COLLECTION_F32_MAX -- refused before cap is looked at
    big = f.Q[:100].copy()
    big[3, 5] = np.float32(2.0 ** 58)
    bq = ctx.bank(big, float_route=True)
    assert lib.fm_collection_xcheck1_each(h, f.coll.handle, bq.handle, inf, P(t), P(d), P(n)) == EUNSUP
    assert lib.fm_collection_xcheck1_each_dev(h, f.coll.handle, bq.handle, inf, -1, rows.data_ptr(), counts.data_ptr(), None, None) == EUNSUP
    bq.close()
    # cap < 0; the output pointers
    assert lib.fm_collection_xcheck1_each_dev(h, k.coll.handle, qb.handle, inf, -1, rows.data_ptr(), counts.data_ptr(), None, None) == EINVAL
    assert lib.fm_collection_xcheck1_each_dev(h, k.coll.handle, qb.handle, inf, 4, rows.data_ptr(), None, None, None) == EINVAL
    assert lib.fm_collection_xcheck1_each_dev(h, k.coll.handle, qb.handle, inf, 4, None, counts.data_ptr(), None, None) == EINVAL
    assert lib.fm_collection_xcheck1_each(h, k.coll.handle, qb.handle, inf, P(t), None, P(n)) == EINVAL
    assert lib.fm_collection_xcheck1_each(h, k.coll.handle, qb.handle, inf, None, None, None) == EINVAL
    # an empty collection is valid and writes nothing
    with ctx.collection() as empty:
        assert empty.xcheck1_each(qb)[0].shape == (0, 100) and empty.mutual_votes(qb).shape == (0,)
    # ... and both collections still work
    _same(k.coll.xcheck1_each(qb), k.ref[100], "after the refusals")
    _same(f.coll.xcheck1_each(f.qb[100]), f.ref[100], "after the refusals, float32 route")
