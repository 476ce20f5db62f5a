"""GPU: train collections (fm_collection_*, matchutil.BFMatcher.add / train / clear) bit for bit against references that
exist already: oracle.bf_knn on the stacked rows mapped through NumPy offsets, and Context.knn2 image by image.
uint8, non-integer float32 (oracle order 1: the device's fma chain) and binary images (tests/hamming_ref.py)."""
import os
import sys

import numpy as np
import pytest

import fastmatch_amd
from fastmatch_amd import _ffi, matchutil, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oracle                      # noqa: E402
from kat import far_banks          # noqa: E402
import hamming_ref as H            # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 2, 15, 127, 128, 129, 1000, 4099]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    if a.dtype == np.float32 or b.dtype == np.float32:
        assert np.array_equal(_bits(a), _bits(b))
    else:
        assert np.array_equal(a, b)


KINDS = ["u8", "f32", "bin1", "bin32", "bin61", "bin64"]


def _knn_ref(kind, Q, T, k):
    if kind.startswith("bin"):
        return H.knn(Q, T, k)
    return oracle.bf_knn(Q, T, k, order=1 if kind == "f32" else 0)


def _stacked_ref(Q, images, k, kind="u8"):
    """The reference on the concatenated rows, every hit mapped to (image, row) through NumPy offsets."""
    dim = Q.shape[1]
    T = np.concatenate([im.reshape(-1, dim) for im in images]) if images else np.zeros((0, dim), Q.dtype)
    idx, dist = _knn_ref(kind, Q, T, k)
    fr = np.concatenate([[0], np.cumsum([im.shape[0] for im in images])]).astype(np.int64)
    img = np.searchsorted(fr, idx, side="right") - 1
    img = np.where(idx >= 0, img, -1).astype(np.int32)
    loc = np.where(idx >= 0, idx - fr[np.maximum(img, 0)], -1).astype(np.int32)
    return img, loc, dist


def _rows(rng, n, kind, dim=128):
    if kind.startswith("bin"):
        w = int(kind[3:])
        hi = 4 if w == 1 else 256                                # one-byte rows of few values: masses of ties
        return rng.integers(0, hi, (n, w), dtype=np.uint8)
    a = synth.synth_sift(max(n, 1), rng)[:n, :dim].copy()
    if kind == "f32":
        a = (a + rng.uniform(-0.5, 0.5, a.shape)).astype(np.float32)
    return a


def _images(rng, sizes, dim=128, kind="u8"):
    return [_rows(rng, n, kind, dim) for n in sizes]


def _qbank(ctx, Q, kind):
    return ctx.bank_binary(Q) if kind.startswith("bin") else ctx.bank(Q)


def _collection(ctx, images, kind="u8"):
    c = ctx.collection()
    for i, im in enumerate(images):
        assert (c.add_binary(im) if kind.startswith("bin") else c.add(im)) == i
    return c


def _check_stacked(ctx, Q, images, ks=range(1, 9), kind="u8"):
    qb = _qbank(ctx, Q, kind)
    with _collection(ctx, images, kind) as c:
        assert c.info()[:2] == (len(images), sum(im.shape[0] for im in images))
        if c.info()[1]:
            assert c.info()[3] == {"u8": _ffi.FM_BANK_I8, "f32": _ffi.FM_BANK_F32}.get(kind, _ffi.FM_BANK_BIN)
        _same(c.image_rows(), [im.shape[0] for im in images])
        for k in ks:
            img, idx, dist = c.knn(qb, k)
            rimg, ridx, rdist = _stacked_ref(Q, images, k, kind)
            _same(img, rimg); _same(idx, ridx); _same(dist, rdist)
    qb.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("sizes", [
    [0, 0, 129, 0, 0, 1000, 1, 2, 15, 127, 128, 4099, 0],        # empty images first, last and adjacent
    [1000, 4099, 129],
    [2, 0, 1, 0, 2],                                             # fewer than k rows in total for k > 5
    [0, 1, 0],
    [0, 0],
    [],
], ids=lambda s: "sizes" + "_".join(map(str, s)))
def test_stacked_knn_equals_the_reference_on_the_concatenated_rows(ctx, sizes, kind):
    rng = np.random.default_rng(len(sizes) + sum(sizes))
    assert set(sizes) <= set(SIZES)
    images = _images(rng, sizes, kind=kind)
    Q = _rows(rng, 777, kind)
    _check_stacked(ctx, Q, images, kind=kind)


def test_stacked_knn_short_rows_and_empty_query(ctx):
    rng = np.random.default_rng(5)
    images = _images(rng, [129, 0, 15, 1000], dim=61)
    _check_stacked(ctx, synth.synth_sift(300, rng)[:, :61].copy(), images)
    with _collection(ctx, images) as c:
        q0 = ctx.bank(np.zeros((0, 61), np.uint8))
        img, idx, dist = c.knn(q0, 3)
        assert img.shape == idx.shape == dist.shape == (0, 3)
        assert c.knn2_each(q0)[0].shape == (4, 0, 2)
        assert c.votes(q0, 0.8).tolist() == [0, 0, 0, 0]
        q0.close()


def test_ties_go_to_the_earliest_image_then_row(ctx):
    rng = np.random.default_rng(6)
    images = _images(rng, [129, 127, 1000, 128])
    Q = synth.synth_sift(200, rng)
    for j in range(0, 200, 3):                                   # the query row itself in several images, twice inside one
        images[0][j % 129] = Q[j]
        images[2][5 + j] = Q[j]
        images[2][500 + j] = Q[j]
        images[3][j % 128] = Q[j]
    low = [np.asarray(rng.integers(0, 2, im.shape), np.uint8) for im in images]     # and masses of ties
    _check_stacked(ctx, Q, images)
    _check_stacked(ctx, np.asarray(rng.integers(0, 2, (300, 128)), np.uint8), low)
    # the same plants in float32 (non-integer) and binary images
    fimgs = [(im + np.float32(0.25)).astype(np.float32) for im in images]
    _check_stacked(ctx, (Q + np.float32(0.25)).astype(np.float32), fimgs, kind="f32")
    bimgs = [np.ascontiguousarray(im[:, :32]) for im in images]
    _check_stacked(ctx, np.ascontiguousarray(Q[:, :32]), bimgs, kind="bin32")


def test_float32_root_tie_range_spread_over_images(ctx):
    rng = np.random.default_rng(7)
    Q, T = far_banks(400, 1500, rng)
    images = [T[:700], T[700:701], np.zeros((0, 128), np.uint8), T[701:]]
    _check_stacked(ctx, Q, images)
    qb = ctx.bank(Q)
    with _collection(ctx, images) as c:
        idx, dist = c.knn2_each(qb)
        for i, im in enumerate(images):
            ridx, rdist = oracle.bf_knn(Q, im, 2, order=0)
            _same(idx[i], ridx); _same(dist[i], rdist)
    qb.close()


def _check_each(ctx, c, qb, Q, images, kind="u8"):
    idx, dist = c.knn2_each(qb)
    assert idx.shape == (len(images), Q.shape[0], 2)
    for i, im in enumerate(images):
        if kind == "f32":
            tb = ctx.bank(im, float_route=True)
        else:
            tb = _qbank(ctx, im, kind)
        gidx, gdist = ctx.knn2(qb, tb)
        tb.close()
        _same(idx[i], gidx); _same(dist[i], gdist)
        ridx, rdist = _knn_ref(kind, Q, im, 2)
        _same(idx[i], ridx); _same(dist[i], rdist)
    return idx, dist


@pytest.mark.parametrize("kind", ["u8", "f32", "bin32", "bin61"])
def test_knn2_each_equals_knn2_image_by_image(ctx, kind):
    rng = np.random.default_rng(8)
    sizes = [int(s) for s in rng.choice(SIZES, 40)]
    sizes[0], sizes[1], sizes[-1] = 0, 1, 0
    sizes[2] = 4099
    images = _images(rng, sizes, kind=kind)
    Q = _rows(rng, 1300, kind)
    qb = _qbank(ctx, Q, kind)
    with _collection(ctx, images, kind) as c:
        idx, dist = _check_each(ctx, c, qb, Q, images, kind)     # 40 images: several batched launches on the integer route
        old = ctx.get_option("batch_group")
        try:
            ctx.set_option("batch_group", 3)
            idx3, dist3 = c.knn2_each(qb)
        finally:
            ctx.set_option("batch_group", old)
        _same(idx3, idx); _same(dist3, dist)
    qb.close()


def _ratio_ref(d0, d1, has2, tau):
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(has2, d0.astype(np.float64) / d1.astype(np.float64), np.nan)
    return r, r < tau


@pytest.mark.parametrize("kind", ["u8", "f32", "bin32"])
def test_ratio_and_votes_equal_numpy_on_the_reference_lists(ctx, kind):
    rng = np.random.default_rng(9)
    images = _images(rng, [1000, 0, 129, 1, 4099, 2], kind=kind)
    Q = _rows(rng, 900, kind)
    for j in range(0, 900, 2):
        if kind == "bin32":
            images[j % 2 * 4][j] = Q[j] ^ np.uint8(1 << (j % 8))
        else:
            images[j % 2 * 4][j] = np.clip(Q[j].astype(np.float64) + rng.integers(-3, 4, 128), 0, 255).astype(Q.dtype)
    images[4][7] = images[4][8] = Q[11]                          # a zero second distance: rejected
    tau = 0.8
    qb = _qbank(ctx, Q, kind)
    with _collection(ctx, images, kind) as c:
        rimg, ridx, rdist = _stacked_ref(Q, images, 2, kind)
        r, p = _ratio_ref(rdist[:, 0], rdist[:, 1], ridx[:, 1] >= 0, tau)
        qidx, img, tidx, dist, ratio = c.knn2_ratio(qb, tau)
        s = np.nonzero(p)[0]
        assert len(s) > 50
        _same(qidx, s.astype(np.int32)); _same(img, rimg[s, 0]); _same(tidx, ridx[s, 0]); _same(dist, rdist[s, 0])
        assert np.array_equal(ratio, r[s])
        v0 = c.votes(qb, tau, 0)
        _same(v0, np.bincount(rimg[s, 0], minlength=len(images)).astype(np.int64))
        assert v0.sum() == len(s)
        v1 = c.votes(qb, tau, 1)
        ref1 = []
        for im in images:
            ei, ed = _knn_ref(kind, Q, im, 2)
            ref1.append(int(_ratio_ref(ed[:, 0], ed[:, 1], ei[:, 1] >= 0, tau)[1].sum()))
        _same(v1, np.asarray(ref1, np.int64))
    qb.close()


def test_growth_clear_and_integer_valued_float32(ctx):
    rng = np.random.default_rng(10)
    images = _images(rng, [129, 1000, 0, 4099, 127, 1000, 2])
    Q = synth.synth_sift(500, rng)
    qb = ctx.bank(Q)

    def fresh(imgs, k=2):
        with _collection(ctx, imgs) as f:
            return f.knn(qb, k), f.knn2_each(qb)

    def same_as_fresh(c, imgs):
        (a, b) = (c.knn(qb, 2), c.knn2_each(qb))
        (fa, fb) = fresh(imgs)
        for x, y in zip(a + b, fa + fb):
            _same(x, y)
        rimg, ridx, rdist = _stacked_ref(Q, imgs, 2)
        _same(a[0], rimg); _same(a[1], ridx); _same(a[2], rdist)

    with ctx.collection() as c:
        for im in images[:2]:
            c.add(im)
        same_as_fresh(c, images[:2])
        for im in images[2:]:                                    # grows past the first allocation
            c.add(im)
        same_as_fresh(c, images)
        c.clear()
        assert c.info()[:2] == (0, 0)
        for im in images[3:6]:
            c.add(im)
        same_as_fresh(c, images[3:6])
    # float32 images with integer values take the integer route; the first non-integer image rebuilds the collection on the
    # float32 route (on the device); every answer equals a collection built fresh from the same images
    f0 = [im.astype(np.float32) for im in images[:3]]
    f1 = [(images[3] + np.float32(0.25)).astype(np.float32), images[4].astype(np.float32),
          (images[5] * np.float32(1.5)).astype(np.float32)]
    qi, qf = ctx.bank(Q.astype(np.float32)), ctx.bank(Q.astype(np.float32), float_route=True)
    assert qi.kind == _ffi.FM_BANK_I8 and qf.kind == _ffi.FM_BANK_F32
    with ctx.collection() as c:
        for im in f0:
            c.add(im)
        assert c.info()[3] == _ffi.FM_BANK_I8
        img, idx, dist = c.knn(qi, 2)
        rimg, ridx, rdist = _stacked_ref(Q, images[:3], 2)
        _same(img, rimg); _same(idx, ridx); _same(dist, rdist)
        with pytest.raises(fastmatch_amd.FastMatchHipError) as e:
            c.add(images[1])                                     # uint8 after float32
        assert e.value.code == -1
        for im in f1:
            c.add(im)
        assert c.info()[:2] == (6, sum(im.shape[0] for im in f0 + f1)) and c.info()[3] == _ffi.FM_BANK_F32
        with pytest.raises(fastmatch_amd.FastMatchHipError) as e:
            c.knn(qi, 2)                                         # an integer-route query against a float32-route collection
        assert e.value.code == -1
        Qf = Q.astype(np.float32)
        for k in (1, 2, 5):
            img, idx, dist = c.knn(qf, k)
            rimg, ridx, rdist = _stacked_ref(Qf, f0 + f1, k, "f32")
            _same(img, rimg); _same(idx, ridx); _same(dist, rdist)
        eidx, edist = c.knn2_each(qf)
        with ctx.collection() as f:
            for im in [(f1[0])] + f0 + f1[1:]:                   # fresh, float32 route from the first image on
                f.add(im)
            fidx, fdist = f.knn2_each(qf)
        order = [1, 2, 3, 0, 4, 5]
        _same(eidx, fidx[order]); _same(edist, fdist[order])
        for i, im in enumerate(f0 + f1):
            ridx2, rdist2 = oracle.bf_knn(Qf, im, 2, order=1)
            _same(eidx[i], ridx2); _same(edist[i], rdist2)
    qi.close(); qf.close(); qb.close()


def test_bfmatcher_collection_and_two_argument_forms(ctx):
    rng = np.random.default_rng(11)
    images = _images(rng, [129, 0, 1000])
    Q = synth.synth_sift(150, rng)
    opts = {"context": ctx}
    m = matchutil.BFMatcher(options=opts)
    m.add(images[:2])
    m.add(images[2:])
    img, idx, dist = m.knnMatch_arrays(Q, 2)
    rimg, ridx, rdist = _stacked_ref(Q, images, 2)
    _same(img, rimg); _same(idx, ridx); _same(dist, rdist)
    lists = m.knnMatch(Q, 2)
    assert len(lists) == 150 and all(len(r) == 2 for r in lists)
    for qi, row in enumerate(lists):
        for j, d in enumerate(row):
            assert (d.queryIdx, d.trainIdx, d.imgIdx) == (qi, idx[qi, j], img[qi, j])
            assert np.float32(d.distance) == dist[qi, j]
    best = m.match(Q)
    assert [(d.imgIdx, d.trainIdx) for d in best] == list(zip(img[:, 0].tolist(), idx[:, 0].tolist()))
    eidx, edist = m.knnMatchEach_arrays(Q)
    for i, im in enumerate(images):
        ridx2, rdist2 = oracle.bf_knn(Q, im, 2, order=0)
        _same(eidx[i], ridx2); _same(edist[i], rdist2)
    assert m.votes(Q, 0.9).sum() == int((_ratio_ref(rdist[:, 0], rdist[:, 1], ridx[:, 1] >= 0, 0.9)[1]).sum())
    m.clear()
    assert m.empty()
    m.add([images[2]])
    _same(m.knnMatch_arrays(Q, 1)[1], oracle.bf_knn(Q, images[2], 1, order=0)[0])
    # with a train argument: bf_match / bf_radius_match unchanged
    for cross in (False, True):
        mm = matchutil.BFMatcher(crossCheck=cross, options=opts)
        got = mm.knnMatch(Q, images[2], 1)
        ref = matchutil.bf_match(Q, images[2], k=1, options=dict(opts, crossCheck=cross))
        assert [[(d.queryIdx, d.trainIdx, d.imgIdx, d.distance) for d in r] for r in got] == \
               [[(d.queryIdx, d.trainIdx, d.imgIdx, d.distance) for d in r] for r in ref]
        flat = mm.match(Q, images[2])
        assert [(d.queryIdx, d.trainIdx) for d in flat] == [(r[0].queryIdx, r[0].trainIdx) for r in ref if r]
    got = matchutil.BFMatcher(options=opts).radiusMatch(Q[:40], images[2], 300.0)
    ref = matchutil.bf_radius_match(Q[:40], images[2], 300.0, options=opts)
    assert [[(d.trainIdx, d.distance) for d in r] for r in got] == [[(d.trainIdx, d.distance) for d in r] for r in ref]
    # NORM_HAMMING and non-integer float32 collections
    bimgs = [rng.integers(0, 256, (n, 32), dtype=np.uint8) for n in (129, 0, 700)]
    bq = rng.integers(0, 256, (90, 32), dtype=np.uint8)
    hm = matchutil.BFMatcher(matchutil.NORM_HAMMING, options=opts)
    hm.add(bimgs)
    himg, hidx, hdist = hm.knnMatch_arrays(bq, 3)
    rimg, ridx, rdist = _stacked_ref(bq, bimgs, 3, "bin32")
    _same(himg, rimg); _same(hidx, ridx); _same(hdist, rdist)
    assert [d.imgIdx for d in hm.match(bq)] == rimg[:, 0].tolist()
    fimgs = [(im + np.float32(0.5)).astype(np.float32) for im in images]
    fm_ = matchutil.BFMatcher(options=opts)
    fm_.add(fimgs)
    Qf = (Q + np.float32(0.5)).astype(np.float32)
    fimg, fidx, fdist = fm_.knnMatch_arrays(Qf, 2)
    rimg, ridx, rdist = _stacked_ref(Qf, fimgs, 2, "f32")
    _same(fimg, rimg); _same(fidx, ridx); _same(fdist, rdist)
    # crossCheck on a collection of ONE image is that image's cross-checked 1-NN
    mc = matchutil.BFMatcher(crossCheck=True, options=opts)
    mc.add([images[2]])
    ci, ct, cd = mc.knnMatch_arrays(Q, 1)
    xt, xd = oracle.bf_xcheck1(Q, images[2])
    _same(ct[:, 0], xt); _same(cd[:, 0], xd)


def test_refusals_leave_the_collection_answering(ctx):
    rng = np.random.default_rng(12)
    images = _images(rng, [129, 1000])
    Q = synth.synth_sift(100, rng)
    qb = ctx.bank(Q)
    with _collection(ctx, images) as c:
        ref = c.knn(qb, 2)
        codes = []
        for call in (lambda: c.knn(qb, 0), lambda: c.knn(qb, 9), lambda: c.votes(qb, 0.8, 2),
                     lambda: c.add(np.zeros((3, 64), np.uint8)), lambda: c.add_binary(np.zeros((3, 32), np.uint8)),
                     lambda: c.knn(ctx.bank(Q[:, :64].copy()), 2), lambda: c.knn(ctx.bank_binary(Q[:, :32].copy()), 2),
                     lambda: c.knn(ctx.bank(Q + np.float32(0.5)), 2)):
            with pytest.raises(fastmatch_amd.FastMatchHipError) as e:
                call()
            codes.append(e.value.code)
        assert codes == [-1, -4, -1, -1, -1, -1, -1, -1]
        assert c.info()[:2] == (2, 1129)
        for a, b in zip(c.knn(qb, 2), ref):
            _same(a, b)
    qb.close()


def test_collection_cycles_give_the_memory_back():
    c = fastmatch_amd.Context(0)
    rng = np.random.default_rng(13)
    images = _images(rng, [1000, 129, 0, 4099])
    Q = synth.synth_sift(600, rng)
    qb = c.bank(Q)

    fimg = (images[0] + np.float32(0.5)).astype(np.float32)
    qf = c.bank(Q.astype(np.float32), float_route=True)
    bimg = rng.integers(0, 256, (1500, 32), dtype=np.uint8)
    qbin = c.bank_binary(bimg[:300])

    def free():
        c.sync()
        return c.mem_info()[0]

    def cycle(k):
        with c.collection() as col:
            for im in images[:2 + k % 3]:
                col.add(im)
            col.knn(qb, 1 + k % 4)
            if k % 3 == 0:
                col.knn2_each(qb)
                col.votes(qb, 0.8, k % 2)
            if k % 5 == 0:
                col.clear()
                col.add(images[3])
                col.knn2_ratio(qb, 0.8)
        if k % 4 == 0:                                           # float32 route (with the rebuild) and binary
            with c.collection() as col:
                col.add(images[1].astype(np.float32))
                col.add(fimg)
                col.knn(qf, 2)
                col.knn2_each(qf)
            with c.collection() as col:
                col.add_binary(bimg)
                col.knn(qbin, 3)
                col.votes(qbin, 0.8, 1)
    for k in range(30):
        cycle(k)
    base = free()
    for k in range(300):
        cycle(k)
    after = free()
    assert base - after <= 4 << 20, (base, after)
    qb.close()
    c.close()


def test_full_size_500_images_of_2000_rows(ctx):
    """1M train rows in 500 images against a 10 000-row query: knn(k = 2) and knn2_each on 1 024 sampled query rows."""
    rng = np.random.default_rng(14)
    T = synth.synth_sift(1000000, rng)
    Q = synth.synth_sift(10000, rng)
    Q[:2000] = np.clip(T[rng.permutation(1000000)[:2000]].astype(int) + rng.integers(-2, 3, (2000, 128)), 0, 255)
    images = [T[2000 * i:2000 * (i + 1)] for i in range(500)]
    s = np.sort(rng.permutation(10000)[:1024])
    qb = ctx.bank(Q)
    with _collection(ctx, images) as c:
        img, idx, dist = c.knn(qb, 2)
        rimg, ridx, rdist = _stacked_ref(Q[s], images, 2)
        _same(img[s], rimg); _same(idx[s], ridx); _same(dist[s], rdist)
        eidx, edist = c.knn2_each(qb)
        for i in range(0, 500, 7):
            ridx2, rdist2 = oracle.bf_knn(Q[s], images[i], 2, order=0)
            _same(eidx[i][s], ridx2); _same(edist[i][s], rdist2)
        # the stacked first neighbour is the best of the per-image first neighbours, earliest image on a tie
        best = np.argmin(edist[:, :, 0].astype(np.float64), axis=0)
        _same(best.astype(np.int32), img[:, 0])
    qb.close()
