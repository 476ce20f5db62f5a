"""GPU: radiusMatch against a train collection (fm_collection_radius_match, _ffi.Collection.radius_match) -- every row of
the stacked images with dist < r_i per query row, as (img, row inside the image), ascending (distance bits, img, row).

Reference (tests/radius_coll_ref.py): oracle.bf_knn on the concatenated rows with k = all rows, cut at dist < r_i, global rows
turned into (img, row) through the cumulative image sizes.  Indices are compared exactly, distances as uint32 bit patterns.
A collection has padding rows behind every image whose size is no multiple of 128; r = +inf is the case that catches one
let through by its value."""
import ctypes

import numpy as np
import pytest

import fastmatch_amd
from fastmatch_amd import _ffi, synth
import radius_coll_ref as RC

pytestmark = pytest.mark.gpu

P = ctypes.c_void_p


def _ptr(a):
    return a.ctypes.data_as(P)


def _qbank(ctx, Q, route):
    return ctx.bank(Q, float_route=route == "f32")


def _collection(ctx, images):
    c = ctx.collection()
    for i, im in enumerate(images):
        assert c.add(im) == i
    return c


@pytest.fixture(scope="module", params=RC.ROUTES)
def std(ctx, request):
    """(route, query bank, collection, reference) of the standard layout; the collection is left unchanged by every test."""
    route = request.param
    Q, images = RC.layout(route)
    qb, c = _qbank(ctx, Q, route), _collection(ctx, images)
    assert c.info()[:2] == (len(RC.SIZES), 1423) and sum(RC.pad128(n) for n in RC.SIZES) == 1920
    assert c.info()[3] == (_ffi.FM_BANK_F32 if route == "f32" else _ffi.FM_BANK_I8)
    yield route, qb, c, RC.layout_ref(route)
    c.close()
    qb.close()


def test_layout_puts_a_split_boundary_inside_a_stage():
    splits, per = RC.sweep_splits(RC.NQ, 1920)
    assert (splits, per) == (2, 960) and per % 128 == 64
    # ... of the 129-row image: rows [768, 1024), whose second stage [896, 1024) holds one real row
    first = np.concatenate([[0], np.cumsum([RC.pad128(n) for n in RC.SIZES])])
    assert first[5] == 768 and first[6] == 1024


def test_scalar_and_per_row_radius(std):
    route, qb, c, ref = std
    r = ref.kth(4)
    want = ref.cut(r)
    assert 2 * ref.nq < want[0][-1] < 12 * ref.nq                  # a few hits per row
    RC.same_lists(c.radius_match(qb, r), want, "scalar")
    rows = RC.mixed_radii(ref)
    assert np.isnan(rows).any() and np.isinf(rows).any() and (rows == 0).any() and (rows < 0).any()
    RC.same_lists(c.radius_match(qb, rows), ref.cut(rows), "per row")
    # a per-row radius overrides radius_all: the C call with both
    off = np.zeros(ref.nq + 1, np.int64)
    tot = ctypes.c_int64(-1)
    rc = c.ctx.lib.fm_collection_radius_match(c.ctx.handle, c.handle, qb.handle, _ptr(rows), 1e9, 0, _ptr(off), None, None, None,
                                              ctypes.byref(tot))
    assert rc == 0 and np.array_equal(off, ref.cut(rows)[0]) and tot.value == off[-1]


def test_infinite_radius_lists_exactly_the_real_rows(std):
    route, qb, c, ref = std
    got = c.radius_match(qb, np.inf)
    assert np.array_equal(np.diff(got[0]), np.full(ref.nq, 1423))
    RC.same_lists(got, ref.cut(np.inf), "r = inf")
    for r in (0.0, -1.0, np.nan, -np.inf):
        off, img, idx, dist = c.radius_match(qb, np.float32(r))
        assert not off.any() and img.size == idx.size == dist.size == 0


def test_infinite_radius_with_the_fp16_filter_switched_off(ctx):
    """Float32 route, the all-pairs path: the last image leaves fp16's range under the collection's scale."""
    Q, images = RC.layout("f32", "wide")
    ref = RC.layout_ref("f32", "wide")
    qb = _qbank(ctx, Q, "f32")
    with _collection(ctx, images) as c:
        RC.same_lists(c.radius_match(qb, np.inf), ref.cut(np.inf), "r = inf, no filter")
        RC.same_lists(c.radius_match(qb, ref.kth(4)), ref.cut(ref.kth(4)), "scalar, no filter")
        rows = RC.mixed_radii(ref, 2)
        RC.same_lists(c.radius_match(qb, rows), ref.cut(rows), "per row, no filter")
    qb.close()


def test_rebuilt_collection_equals_one_that_was_float32_from_the_start(ctx):
    rng = np.random.default_rng(31)
    ints = [synth.synth_sift(n, rng).astype(np.float32) for n in (130, 0, 65)]
    frac = RC.floaty(synth.synth_sift(200, rng), rng)
    Q = RC.floaty(synth.synth_sift(70, rng), rng)
    qb = ctx.bank(Q, float_route=True)
    ref = RC.Ref(Q, ints + [frac])
    r = ref.kth(3)
    with ctx.collection() as c:
        for im in ints:
            c.add(im)
        assert c.info()[3] == _ffi.FM_BANK_I8
        c.add(frac)                                              # rebuilds on the float32 route
        assert c.info()[3] == _ffi.FM_BANK_F32
        rebuilt = [c.radius_match(qb, x) for x in (r, np.inf)]
    # the same values as float32 from the start: the first image carries a non-integer value, the order is restored below
    with ctx.collection() as f:
        for im in [frac] + ints:
            f.add(im)
        assert f.info()[3] == _ffi.FM_BANK_F32
        fresh_inf = f.radius_match(qb, np.inf)
    for got, x in zip(rebuilt, (r, np.inf)):
        RC.same_lists(got, ref.cut(x), "rebuilt")
    # image i of the rebuilt collection is image (i + 1) % 4 of the fresh one; per row the (distance, image, row) sets agree
    ro, ri, rx, rd = rebuilt[1]
    fo, fi, fx, fd = fresh_inf
    assert np.array_equal(ro, fo)
    fi = (fi + 3) % 4
    for i in (0, 17, 69):
        a = sorted(zip(RC.bits(rd[ro[i]:ro[i + 1]]).tolist(), ri[ro[i]:ro[i + 1]].tolist(), rx[ro[i]:ro[i + 1]].tolist()))
        b = sorted(zip(RC.bits(fd[fo[i]:fo[i + 1]]).tolist(), fi[fo[i]:fo[i + 1]].tolist(), fx[fo[i]:fo[i + 1]].tolist()))
        assert a == b
    qb.close()


@pytest.mark.parametrize("route", RC.ROUTES)
def test_ties_go_to_the_earlier_image_then_the_earlier_row(ctx, route):
    rng = np.random.default_rng(33)
    base = synth.synth_sift(40, rng)
    Q = np.concatenate([base[:25], synth.synth_sift(10, rng)])
    if route == "f32":
        base, Q = base.astype(np.float32) / np.float32(7.0), Q.astype(np.float32) / np.float32(7.0)
    images = [base[rng.permutation(40)] for _ in range(3)]
    images[1] = np.concatenate([images[1], images[1][:9]])       # ties inside one image too
    ref = RC.Ref(Q, images)
    qb = _qbank(ctx, Q, route)
    with _collection(ctx, images) as c:
        for r in (ref.kth(9), np.inf):
            got = c.radius_match(qb, r)
            RC.same_lists(got, ref.cut(r), "ties")
        off, img, idx, dist = got
        for i in range(25):                                       # the query's own descriptor: distance 0, images 0, 1, 1, 2
            z = dist[off[i]:off[i + 1]] == 0
            zi, zx = img[off[i]:off[i + 1]][z], idx[off[i]:off[i + 1]][z]
            assert list(zip(zi, zx)) == sorted(zip(zi, zx)) and set(zi) == {0, 1, 2}
    qb.close()


@pytest.mark.parametrize("route", RC.ROUTES)
def test_lists_beyond_2048_keys(ctx, route):
    rng = np.random.default_rng(35)
    images = [synth.synth_sift(n, rng) for n in (70, 2150, 3)]
    Q = synth.synth_sift(5, rng)
    if route == "f32":
        images, Q = [RC.floaty(im, rng) for im in images], RC.floaty(Q, rng)
    ref = RC.Ref(Q, images)
    qb = _qbank(ctx, Q, route)
    with _collection(ctx, images) as c:
        got = c.radius_match(qb, np.inf)
        assert np.all(np.diff(got[0]) == 2223)
        RC.same_lists(got, ref.cut(np.inf), "long lists")
    qb.close()


def test_many_chunks_give_the_same_bits(ctx, std):
    route, qb, c, ref = std
    old = ctx.get_option("radius_ws_bytes")
    ctx.set_option("radius_ws_bytes", 65536)                      # 2340 candidates (28 B each) per chunk
    try:
        for r in (ref.kth(4), RC.mixed_radii(ref, 3), np.inf):
            RC.same_lists(c.radius_match(qb, r), ref.cut(r), "chunked")
    finally:
        ctx.set_option("radius_ws_bytes", old)


def _raw(c, qb, r, cap, nq, size, with_lists=True):
    """The C call with sentinel-filled arrays of `size` entries: (rc, offsets, img, idx, dist, n_total)."""
    off = np.full(nq + 1, -7, np.int64)
    img, idx = np.full(size, -77, np.int32), np.full(size, -78, np.int32)
    dist = np.full(size, -79.0, np.float32)
    tot = ctypes.c_int64(-1)
    rows = None if np.ndim(r) == 0 else np.ascontiguousarray(r, np.float32)
    rc = c.ctx.lib.fm_collection_radius_match(c.ctx.handle, c.handle, qb.handle, _ptr(rows) if rows is not None else None,
                                              float(np.float32(r)) if rows is None else 0.0, cap, _ptr(off),
                                              _ptr(img) if with_lists else None, _ptr(idx) if with_lists else None,
                                              _ptr(dist) if with_lists else None, ctypes.byref(tot))
    return rc, off, img, idx, dist, tot.value


def test_cap_counts_only_and_the_prefix_of_whole_rows(ctx, std):
    route, qb, c, ref = std
    r = RC.mixed_radii(ref, 4)
    woff, wimg, widx, wdist, _ = ref.cut(r)
    total = int(woff[-1])
    rc, off, _, _, _, tot = _raw(c, qb, r, 0, ref.nq, 1, with_lists=False)          # counts only, NULL lists
    assert rc == 0 and np.array_equal(off, woff) and tot == total
    k = ref.nq // 2
    assert 0 < woff[k] < total
    old = ctx.get_option("radius_ws_bytes")
    try:
        for ws in (old, 65536):
            ctx.set_option("radius_ws_bytes", ws)
            for cap in (total - 1, int(woff[k]), total):
                rc, off, img, idx, dist, tot = _raw(c, qb, r, cap, ref.nq, total + 5)
                assert rc == 0 and np.array_equal(off, woff) and tot == total
                m = int(woff[np.searchsorted(woff, cap, side="right") - 1])         # the longest prefix of whole rows within cap
                assert m <= cap and (cap < total) == (m < total)
                assert np.array_equal(img[:m], wimg[:m]) and np.array_equal(idx[:m], widx[:m])
                assert np.array_equal(RC.bits(dist[:m]), RC.bits(wdist[:m]))
                assert np.all(img[m:] == -77) and np.all(idx[m:] == -78) and np.all(dist[m:] == -79.0), "written beyond the prefix"
    finally:
        ctx.set_option("radius_ws_bytes", old)


@pytest.mark.parametrize("route", RC.ROUTES)
def test_degenerate_inputs(ctx, route):
    Q, images = RC.layout(route)
    qb, q0 = _qbank(ctx, Q, route), _qbank(ctx, Q[:0], route)
    with _collection(ctx, images) as c:
        off, img, idx, dist = c.radius_match(q0, np.inf)          # nq = 0
        assert off.shape == (1,) and off[0] == 0 and img.size == idx.size == dist.size == 0
    for imgs in ([], [Q[:0], Q[:0], Q[:0]]):                      # an empty collection; empty images only
        with _collection(ctx, imgs) as c:
            for r in (np.inf, np.full(len(Q), np.inf, np.float32)):
                off, img, idx, dist = c.radius_match(qb, r)
                assert off.shape == (len(Q) + 1,) and not off.any() and img.size == idx.size == dist.size == 0
            rc, off, _, _, _, tot = _raw(c, qb, np.inf, 0, len(Q), 1, with_lists=False)
            assert rc == 0 and not off.any() and tot == 0
    qb.close()
    q0.close()


def test_refusals_with_their_codes_leave_the_context_working(ctx, std):
    route, qb, c, ref = std
    rng = np.random.default_rng(37)

    def still_answers():
        RC.same_lists(c.radius_match(qb, ref.kth(2)), ref.cut(ref.kth(2)), "after a refusal")

    def refused(call, code):
        with pytest.raises(fastmatch_amd.FastMatchHipError) as e:
            call()
        assert e.value.code == code, e.value
        still_answers()

    with ctx.collection() as b:                                   # a binary collection: FM_EUNSUPPORTED
        b.add_binary(rng.integers(0, 256, (50, 32), dtype=np.uint8))
        qbin = ctx.bank_binary(rng.integers(0, 256, (9, 32), dtype=np.uint8))
        refused(lambda: b.radius_match(qbin, 40.0), -4)
        qbin.close()
    Q, _ = RC.layout(route)
    narrow = _qbank(ctx, np.ascontiguousarray(Q[:, :64]), route)  # another width: FM_EINVAL
    refused(lambda: c.radius_match(narrow, np.inf), -1)
    narrow.close()
    other = _qbank(ctx, RC.layout("i8" if route == "f32" else "f32")[0], "i8" if route == "f32" else "f32")
    refused(lambda: c.radius_match(other, np.inf), -1)            # another kind: FM_EINVAL
    other.close()
    if route == "f32":
        big = np.array(Q[:4])
        big[1, 3] = np.float32(2.0 ** 58)                         # above FM_COLLECTION_F32_MAX = 2^57: FM_EUNSUPPORTED
        qbig = _qbank(ctx, big, route)
        refused(lambda: c.radius_match(qbig, np.inf), -4)
        qbig.close()
    assert _raw(c, qb, np.inf, -1, ref.nq, 4)[0] == -1                           # cap < 0: FM_EINVAL
    still_answers()
    assert _raw(c, qb, np.inf, 8, ref.nq, 8, with_lists=False)[0] == -1           # NULL lists with cap > 0: FM_EINVAL
    still_answers()


def test_accounted_in_the_stats_with_the_real_rows(std):
    route, qb, c, ref = std
    before = c.ctx.stats()
    _raw(c, qb, np.float32(ref.kth(2)), 0, ref.nq, 1, with_lists=False)
    after = c.ctx.stats()
    assert after["calls"] - before["calls"] == 1 and after["pairs"] - before["pairs"] == ref.nq * 1423


@pytest.mark.parametrize("route", RC.ROUTES)
def test_plain_pairs_are_unchanged(ctx, route):
    """Context.radius_match on a plain bank pair of the same sizes: the null-table path of the changed kernels."""
    Q, images = RC.layout(route)
    T = np.concatenate(images)
    ref = RC.layout_ref(route)
    qb, tb = _qbank(ctx, Q, route), _qbank(ctx, T, route)
    for r in (ref.kth(4), RC.mixed_radii(ref), np.inf):
        off, idx, dist = ctx.radius_match(qb, tb, r)
        woff, _, _, wdist, wglobal = ref.cut(r)
        assert np.array_equal(off, woff) and np.array_equal(idx, wglobal) and np.array_equal(RC.bits(dist), RC.bits(wdist))
    qb.close()
    tb.close()
