"""GPU: Fast-Match's accepted-match test of a query against a train collection (fm_collection_match_accepted_each, its
device form, Collection.accepted_votes, BFMatcher.fastMatchEach), bit for bit on all four columns and the counts against
  * Context.match_accepted(q, bank(image_i), tau) with the same self distances attached (code older than the collection form),
  * for integer banks also oracle.bf_xcheck1 plus the oracle's ratio filter, image by image."""
import os
import sys

import numpy as np
import pytest

import fastmatch_amd
from fastmatch_amd import _ffi, matchutil, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oracle                      # noqa: E402
from kat import far_banks, SQRT_TIE_MIN          # noqa: E402

pytestmark = pytest.mark.gpu

BOUNDARY_SIZES = [0, 1, 127, 128, 129, 1000, 5, 0]      # on a stage boundary, one row past it, empty first / middle / last


def _same_rows(got, ref, what):
    """Two lists (one entry per image) of (qidx, tidx, dist, ratio): the same counts and the same bits."""
    assert len(got) == len(ref), what
    for i, (g, r) in enumerate(zip(got, ref)):
        assert [len(a) for a in g] == [len(a) for a in r], "%s: image %d: %d rows, reference %d" % (what, i, len(g[0]), len(r[0]))
        assert np.array_equal(g[0], r[0]), "%s: image %d: query rows" % (what, i)
        assert np.array_equal(g[1], r[1]), "%s: image %d: train rows" % (what, i)
        assert np.array_equal(np.asarray(g[2], np.float32).view(np.uint32), np.asarray(r[2], np.float32).view(np.uint32)), \
            "%s: image %d: distances" % (what, i)
        assert np.array_equal(np.asarray(g[3], np.float64).view(np.uint64), np.asarray(r[3], np.float64).view(np.uint64)), \
            "%s: image %d: ratios" % (what, i)


def _ref_pairs(ctx, qb, images, tau, float_route=False):
    """Context.match_accepted image by image: one bank per image."""
    out = []
    for im in images:
        tb = ctx.bank(im, float_route=float_route)
        out.append(tuple(np.array(a) for a in ctx.match_accepted(qb, tb, tau)))
        tb.close()
    return out


def _ref_oracle(Q, sd, images, tau):
    """oracle.bf_xcheck1 and the oracle's ratio filter image by image (integer banks)."""
    out = []
    for im in images:
        if im.shape[0] == 0 or Q.shape[0] == 0:
            out.append((np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32), np.zeros(0, np.float64)))
            continue
        tidx, dist = oracle.bf_xcheck1(Q, im)
        rows = np.nonzero(tidx >= 0)[0].astype(np.int32)
        ratio, ok = oracle.ratio_filter(dist[rows], sd, tau, qrows=rows)
        out.append((rows[ok], tidx[rows][ok], dist[rows][ok], ratio[ok]))
    return out


def _images_and_query(rng, sizes, nq, noise=3):
    """SIFT-like images, and a query of which two rows in three are noisy copies of image rows (so that rows are accepted
    at the usual tau) and the rest independent."""
    images = [synth.synth_sift(max(n, 1), rng)[:n].copy() for n in sizes]
    pool = np.concatenate(images) if sum(sizes) else synth.synth_sift(4, rng)
    Q = synth.synth_sift(nq, rng)
    take = rng.random(nq) < 0.66
    src = pool[rng.integers(0, pool.shape[0], nq)].astype(np.int32) + rng.integers(-noise, noise + 1, (nq, 128))
    Q[take] = np.clip(src, 0, 255).astype(np.uint8)[take]
    return images, Q


def _collection(ctx, images):
    c = ctx.collection()
    for i, im in enumerate(images):
        assert c.add(im) == i
    return c


def _query_bank(ctx, Q, sd=None, float_route=False):
    qb = ctx.bank(Q, float_route=float_route)
    sd = ctx.self_dist(qb) if sd is None else np.asarray(sd, np.float64)
    qb.set_selfdist(sd)
    return qb, sd


@pytest.fixture(scope="module")
def boundary(ctx):
    """The image-boundary collection and its queries, shared (and left unchanged) by the tests that need it."""
    rng = np.random.default_rng(11)
    images, Q700 = _images_and_query(rng, BOUNDARY_SIZES, 700)
    coll = _collection(ctx, images)
    queries = {}
    for nq in (100, 700):
        Q = Q700[:nq].copy()
        qb, sd = _query_bank(ctx, Q)
        queries[nq] = (Q, qb, sd)
    yield images, coll, queries
    coll.close()
    for _, qb, _ in queries.values():
        qb.close()


@pytest.mark.parametrize("tau", [0.6, 0.9, 10.0])
@pytest.mark.parametrize("nq", [100, 700])
def test_image_boundaries(ctx, boundary, nq, tau):
    images, coll, queries = boundary
    Q, qb, sd = queries[nq]
    got = coll.match_accepted_each(qb, tau)
    _same_rows(got, _ref_pairs(ctx, qb, images, tau), "match_accepted per image")
    _same_rows(got, _ref_oracle(Q, sd, images, tau), "oracle per image")
    assert [len(g[0]) for g in got][0] == 0 and len(got[4][0]) > 0          # an empty image keeps its slot; rows are accepted
    if tau == 10.0:                  # nearly every elected row: every train row of the one-row image elects somebody
        assert len(got[1][0]) == 1


def test_ties_and_duplicates(ctx):
    rng = np.random.default_rng(12)
    A = synth.synth_sift(300, rng)
    B = synth.synth_sift(200, rng)
    A[7] = A[3]                      # a row twice in one image: the lowest train row wins
    B[150] = A[3]                    # ... and once more in another image: both images report it
    B[20] = A[40]
    Q = synth.synth_sift(120, rng)
    Q[10] = A[3]; Q[20] = A[3]       # duplicated query rows: a train row elects the lower query index
    Q[33] = A[40]                    # an exact match whose query row has self distance 0
    images = [A, B]
    sd = np.array(oracle.self_dist(Q), np.float64)
    assert sd[10] == 0 and sd[20] == 0
    sd[10] = 50.0; sd[20] = 50.0; sd[33] = 0.0
    qb, _ = _query_bank(ctx, Q, sd)
    with _collection(ctx, images) as c:
        for tau in (0.8, 10.0):
            got = c.match_accepted_each(qb, tau)
            _same_rows(got, _ref_pairs(ctx, qb, images, tau), "match_accepted per image")
            _same_rows(got, _ref_oracle(Q, sd, images, tau), "oracle per image")
            for i, t in ((0, 3), (1, 150)):
                qi, ti, di, _ = got[i]
                at = np.nonzero(qi == 10)[0]
                assert at.size == 1 and ti[at[0]] == t and di[at[0]] == 0.0      # the lower query row, the lowest train row
                assert 20 not in qi[(ti == 3) | (ti == 7) | (ti == 150)]
                assert 33 not in qi                                            # 0 / 0: never accepted, even at d = 0
    qb.close()


def test_splits_of_the_reduced_range(ctx):
    rng = np.random.default_rng(13)
    images, Q = _images_and_query(rng, [3000, 3000, 3000], 40000)
    qb, sd = _query_bank(ctx, Q)
    with _collection(ctx, images) as c:
        got = c.match_accepted_each(qb, 0.9)
    _same_rows(got, _ref_pairs(ctx, qb, images, 0.9), "match_accepted per image")
    _same_rows(got, _ref_oracle(Q, sd, images, 0.9), "oracle per image")
    assert min(len(g[0]) for g in got) > 100
    qb.close()


def test_float32_root_ties_per_image(ctx):
    """One image in the range where two d2 share a float32 root (kat.far_banks: every distance of the pair lies there), one
    far below it, one more in the range: the tie list is decided image by image."""
    rng = np.random.default_rng(14)
    Q, far0 = far_banks(300, 500, rng)
    _, far1 = far_banks(1, 260, rng, small_max=2)
    near = np.zeros((400, 128), np.uint8)
    near[:, 101:111] = rng.integers(0, 3, (400, 10), dtype=np.uint8)
    images = [far0, near, far1]
    assert int((far0.astype(np.int64) ** 2).sum(1).max()) >= SQRT_TIE_MIN > int((near.astype(np.int64) ** 2).sum(1).max()) + 4 * 128
    sd = rng.uniform(1.0, 4000.0, 300)                 # d ~ 2550 against the far images, d <= 5 against the near one
    qb, _ = _query_bank(ctx, Q, sd)
    with _collection(ctx, images) as c:
        for tau in (1.0, 0.8):                         # (far images: accepted where sd > 2550 / tau)
            got = c.match_accepted_each(qb, tau)
            _same_rows(got, _ref_pairs(ctx, qb, images, tau), "match_accepted per image")
            _same_rows(got, _ref_oracle(Q, sd, images, tau), "oracle per image")
            assert min(len(g[0]) for g in got) > 0        # rows are accepted in the tie range and below it
    qb.close()


def test_cap_and_counts(ctx, boundary):
    images, coll, queries = boundary
    Q, qb, sd = queries[700]
    full = coll.match_accepted_each(qb, 10.0)
    counts = np.array([len(g[0]) for g in full], np.int64)
    assert counts.max() > 3
    # cap below an image's count: the rows are the prefix, the count stays full
    ni, cap = len(images), 3
    qidx, tidx = np.full((ni, cap), -7, np.int32), np.full((ni, cap), -7, np.int32)
    dist, ratio = np.full((ni, cap), -7, np.float32), np.full((ni, cap), -7, np.float64)
    n = np.full(ni, -7, np.int64)
    ctx._check(ctx.lib.fm_collection_match_accepted_each(ctx.handle, coll.handle, qb.handle, 10.0, cap, qidx.ctypes.data, tidx.ctypes.data,
                                                         dist.ctypes.data, ratio.ctypes.data, n.ctypes.data))
    assert np.array_equal(n, counts)
    capped = [(qidx[i, :min(cap, counts[i])], tidx[i, :min(cap, counts[i])], dist[i, :min(cap, counts[i])], ratio[i, :min(cap, counts[i])])
              for i in range(ni)]
    _same_rows(capped, [tuple(a[:cap] for a in g) for g in full], "cap = 3")
    _same_rows(coll.match_accepted_each(qb, 10.0, cap=cap), capped, "Collection.match_accepted_each(cap=3)")
    for i in range(ni):              # nothing is written behind the rows that are there
        assert np.all(qidx[i, min(cap, counts[i]):] == -7)
    # cap = 0: counts only, NULL row arrays; accepted_votes is that call
    n0 = np.full(ni, -7, np.int64)
    ctx._check(ctx.lib.fm_collection_match_accepted_each(ctx.handle, coll.handle, qb.handle, 10.0, 0, None, None, None, None, n0.ctypes.data))
    assert np.array_equal(n0, counts)
    assert np.array_equal(coll.accepted_votes(qb, 10.0), counts)
    assert np.array_equal(coll.accepted_votes(qb, 0.6), [len(g[0]) for g in coll.match_accepted_each(qb, 0.6)])


def test_growth_of_the_allocation(ctx):
    rng = np.random.default_rng(15)
    images, Q = _images_and_query(rng, [1000, 129, 3000, 2000], 500)
    qb, sd = _query_bank(ctx, Q)
    with _collection(ctx, images[:2]) as c:
        got = c.match_accepted_each(qb, 0.9)
        _same_rows(got, _ref_pairs(ctx, qb, images[:2], 0.9), "before the growth")
        c.add(images[2]); c.add(images[3])             # 1280 + 3072 + 2048 physical rows: past the first 4096
        got = c.match_accepted_each(qb, 0.9)
        _same_rows(got, _ref_pairs(ctx, qb, images, 0.9), "after the growth")
        _same_rows(got, _ref_oracle(Q, sd, images, 0.9), "after the growth, oracle")
    qb.close()


def test_chunks_of_images(ctx, boundary):
    """The option "coll_ws_bytes" forced so small that the eight images run in four chunks, then in eight."""
    images, coll, queries = boundary
    Q, qb, sd = queries[700]
    assert ctx.get_option("coll_ws_bytes") == 0
    whole = coll.match_accepted_each(qb, 0.9)
    per_image = 700 * 25 + 3 * 4
    try:
        for budget, chunks in ((2 * per_image + 100, 4), (1, 8)):
            ctx.set_option("coll_ws_bytes", budget)
            assert -(-len(images) // max(1, budget // per_image)) == chunks >= 3
            _same_rows(coll.match_accepted_each(qb, 0.9), whole, "%d chunks" % chunks)
            assert np.array_equal(coll.accepted_votes(qb, 0.9), [len(g[0]) for g in whole])
    finally:
        ctx.set_option("coll_ws_bytes", 0)
    _same_rows(whole, _ref_pairs(ctx, qb, images, 0.9), "match_accepted per image")


@pytest.mark.parametrize("f32_filter", [1, 2])
def test_float32_route(ctx, f32_filter):
    """Integer-valued float32 images, then one image + 0.25: the collection is rebuilt on the float32 route."""
    rng = np.random.default_rng(16)
    sizes = [129, 1000, 0, 64]
    ints, Q = _images_and_query(rng, sizes, 600)
    images = [im.astype(np.float32) for im in ints]
    images[3] = images[3] + np.float32(0.25)
    Qf = Q.astype(np.float32)
    try:
        ctx.set_option("f32_filter", f32_filter)
        qb, sd = _query_bank(ctx, Qf, float_route=True)
        with _collection(ctx, images) as c:
            assert c.info()[3] == _ffi.FM_BANK_F32
            for tau in (0.9, 10.0):
                got = c.match_accepted_each(qb, tau)
                _same_rows(got, _ref_pairs(ctx, qb, images, tau, float_route=True), "match_accepted per float32-route image")
                assert np.array_equal(c.accepted_votes(qb, tau), [len(g[0]) for g in got])
            assert len(got[1][0]) > 0 and len(got[2][0]) == 0
        qb.close()
    finally:
        ctx.set_option("f32_filter", 1)


def test_device_form_on_a_consumer_stream(ctx, boundary):
    import torch
    images, coll, queries = boundary
    Q, qb, sd = queries[700]
    ni, cap = len(images), 64
    host = coll.match_accepted_each(qb, 0.9)
    counts = np.array([len(g[0]) for g in host], np.int64)
    assert counts.max() > cap > counts[counts > 0].min()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        rows = torch.full((ni, cap, 3), -7, dtype=torch.int32, device="cuda")
        cnt = torch.full((ni,), -7, dtype=torch.int64, device="cuda")
        coll.match_accepted_each_dev(qb, 0.9, rows.data_ptr(), cnt.data_ptr(), cap, consumer_stream=side.cuda_stream)
        rows_h, cnt_h = rows.cpu().numpy(), cnt.cpu().numpy()          # (on the consumer stream: ordered behind the fill)
        h_counts = np.full(ni, -7, np.int64)
        coll.match_accepted_each_dev(qb, 0.9, rows.data_ptr(), cnt.data_ptr(), cap, h_counts=h_counts, consumer_stream=side.cuda_stream)
        rows_h2 = rows.cpu().numpy()
    assert np.array_equal(cnt_h, np.minimum(counts, cap))
    assert np.array_equal(h_counts, counts)
    assert np.array_equal(rows_h, rows_h2)
    for i in range(ni):
        m = int(cnt_h[i])
        assert np.array_equal(rows_h[i, :m, 0], host[i][0][:m]) and np.array_equal(rows_h[i, :m, 1], host[i][1][:m])
        assert np.array_equal(rows_h[i, :m, 2].view(np.uint32), np.asarray(host[i][2][:m]).view(np.uint32))
        assert np.all(rows_h[i, m:] == -7)
    # counts only, no consumer stream
    cnt0 = torch.full((ni,), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    h0 = np.full(ni, -7, np.int64)
    coll.match_accepted_each_dev(qb, 0.9, 0, cnt0.data_ptr(), 0, h_counts=h0)
    assert np.array_equal(h0, counts) and np.all(cnt0.cpu().numpy() == 0)


def test_refusals_leave_the_collection_intact(ctx, boundary):
    import torch
    images, coll, queries = boundary
    Q, qb, sd = queries[100]
    before = coll.knn(qb, 2)

    def refused(code, fn, *a, **k):
        with pytest.raises(fastmatch_amd.FastMatchHipError) as e:
            fn(*a, **k)
        assert e.value.code == code, str(e.value)
        return str(e.value)

    EINVAL, EUNSUPPORTED = -1, -4
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fastmatch_hip.h")).read()
    import re
    assert int(re.search(r"#define\s+FM_EINVAL\s+(-?\d+)", hdr).group(1)) == EINVAL
    assert int(re.search(r"#define\s+FM_EUNSUPPORTED\s+(-?\d+)", hdr).group(1)) == EUNSUPPORTED
    bare = ctx.bank(Q)                                              # no self distances
    assert "no self distances" in refused(EINVAL, coll.match_accepted_each, bare, 0.9)
    assert "no self distances" in refused(EINVAL, coll.accepted_votes, bare, 0.9)
    narrow = ctx.bank(Q[:, :64].copy())
    narrow.set_selfdist(ctx.self_dist(narrow))
    refused(EINVAL, coll.match_accepted_each, narrow, 0.9)            # another width
    assert "cap < 0" in refused(EINVAL, coll.match_accepted_each, qb, 0.9, cap=-1)
    # host memory passed to the device form
    hrows, hcnt = np.zeros((len(images), 4, 3), np.int32), np.zeros(len(images), np.int64)
    cnt = torch.zeros(len(images), dtype=torch.int64, device="cuda")
    rows = torch.zeros((len(images), 4, 3), dtype=torch.int32, device="cuda")
    assert "device memory" in refused(EINVAL, coll.match_accepted_each_dev, qb, 0.9, hrows.ctypes.data, cnt.data_ptr(), 4)
    assert "device memory" in refused(EINVAL, coll.match_accepted_each_dev, qb, 0.9, rows.data_ptr(), hcnt.ctypes.data, 4)
    after = coll.knn(qb, 2)
    for a, b in zip(before, after):
        assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
    # an integer query against a float32-route collection
    with ctx.collection() as cf:
        cf.add(images[3].astype(np.float32)); cf.add(images[4].astype(np.float32) + np.float32(0.25))
        assert cf.info()[3] == _ffi.FM_BANK_F32
        refused(EINVAL, cf.match_accepted_each, qb, 0.9)
        qf, _ = _query_bank(ctx, Q.astype(np.float32), float_route=True)
        kf = cf.knn(qf, 2)
        refused(EINVAL, cf.match_accepted_each, qb, 0.9)
        assert all(np.array_equal(a, b) for a, b in zip((x.view(np.uint32) for x in kf), (x.view(np.uint32) for x in cf.knn(qf, 2))))
        qf.close()
    # a binary collection
    rng = np.random.default_rng(17)
    with ctx.collection() as cb:
        cb.add_binary(rng.integers(0, 256, (300, 32), dtype=np.uint8))
        qbin = ctx.bank_binary(rng.integers(0, 256, (50, 32), dtype=np.uint8))
        kb = cb.knn(qbin, 2)
        refused(EUNSUPPORTED, cb.match_accepted_each, qbin, 0.9)
        refused(EUNSUPPORTED, cb.accepted_votes, qbin, 0.9)
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(kb, cb.knn(qbin, 2)))
        qbin.close()
    bare.close(); narrow.close()


def test_empty_query_and_empty_collection(ctx, boundary):
    images, coll, queries = boundary
    q0 = ctx.bank(np.zeros((0, 128), np.uint8))
    got = coll.match_accepted_each(q0, 0.9)
    assert len(got) == len(images) and all(len(g[0]) == 0 for g in got)
    assert np.array_equal(coll.accepted_votes(q0, 0.9), np.zeros(len(images), np.int64))
    Q, qb, sd = queries[100]
    with ctx.collection() as c:
        assert c.match_accepted_each(qb, 0.9) == [] and c.accepted_votes(qb, 0.9).shape == (0,)
        c.add(np.zeros((0, 128), np.uint8)); c.add(np.zeros((0, 128), np.uint8))
        got = c.match_accepted_each(qb, 0.9)
        assert len(got) == 2 and all(len(g[0]) == 0 for g in got)
    q0.close()


def test_bfmatcher_fast_match_each(ctx):
    rng = np.random.default_rng(18)
    images, Q = _images_and_query(rng, [700, 129, 400], 300)
    m = matchutil.BFMatcher(matchutil.NORM_L2, crossCheck=False, options={"context": ctx})
    m.add(images)
    lists = m.fastMatchEach(Q, 0.9)
    qb, sd = _query_bank(ctx, Q)
    with _collection(ctx, images) as c:
        arrays = c.match_accepted_each(qb, 0.9)
    _same_rows(m.fastMatchEach_arrays(Q, 0.9), arrays, "fastMatchEach_arrays")
    _same_rows(arrays, _ref_oracle(Q, np.array(oracle.self_dist(Q), np.float64), images, 0.9), "oracle per image")
    assert len(lists) == 3 and sum(len(l) for l in lists) > 0
    for i, (l, (qi, ti, di, _)) in enumerate(zip(lists, arrays)):
        assert [d.queryIdx for d in l] == list(qi) and [d.trainIdx for d in l] == list(ti)
        assert [d.distance for d in l] == [float(x) for x in di]
        assert all(d.imgIdx == i for d in l)
    # the crossCheck flag changes nothing: the test is cross-checked by definition
    mx = matchutil.BFMatcher(matchutil.NORM_L2, crossCheck=True, options={"context": ctx})
    mx.add(images)
    _same_rows(mx.fastMatchEach_arrays(Q, 0.9), arrays, "crossCheck=True")
    # a resident bank with self distances attached is used as it is
    _same_rows(m.fastMatchEach_arrays(qb, 0.9), arrays, "a Bank as the query")
    qb.close()
