"""GPU: every consumer of the float32 route -- knn (k = 1, 2 on K8 / K5; k = 3 .. 8 on K9), xcheck1, self_dist, radius_match
and float32 train collections -- on value regimes far off the SIFT range (tests/f32_regimes.py), bit for bit against the
oracle's fma chain (order 1), on three private contexts: the fp16 filter forced, K5 only, and the default.  Every
comparison is np.array_equal on raw bits; the three contexts agree with each other because each equals the same oracle
arrays (and, where a call is refused, each refuses with the same code).

What failed on the parent commit's library (ids [context-regime]; everything else passed unchanged):
  * test_knn_xcheck1_selfdist[filter-overflow] (knn2): K8's rescoring packed the distance inf of an overflowed chain into a
    key (index >= 0, dist inf) where K5 and the oracle have -1 / inf;
  * test_knn_xcheck1_selfdist[*-overflow], [*-nonfinite] (k = 3, 8) and test_collection[*-nonfinite] (k = 8): K9 did the same
    with inf and NaN distances;
  * test_knn_xcheck1_selfdist[filter-underflow23], [filter-underflow30] (knn2), test_collection[filter-underflow23],
    [filter-underflow30] and test_radius_match[*-underflow23], [*-underflow30] (its fp16 filter does not follow the
    f32_filter option): the filters ranked by accumulators that still tell rows apart whose exact distances are 0 or tied;
  * [filter-tiny] of test_knn_xcheck1_selfdist and test_collection: the values were equal; only the route assertion fails
    there, because the filter now declines that scale (filter_usable's window keeps a margin of 2^10);
  * test_padding_trap[*], test_collection_limit_just_below_and_just_above[*], test_collection[*-huge], [*-overflow]: nothing
    refused magnitudes beyond what masking a collection's padding rows by value can carry (test_f32_regimes_host.py shows
    on the CPU that rows of 1e18 enter the lists there)."""
import functools

import numpy as np
import pytest

import fastmatch_amd
import oracle
import f32_regimes as R
from test_radius_match_gpu import _check as _check_radius, _ref as _radius_ref

pytestmark = pytest.mark.gpu

MODES = {"filter": 2, "k5": 0, "default": None}
NAMES = list(R.REGIMES)
REFUSED = ("huge", "overflow")               # beyond FM_COLLECTION_F32_MAX: a float32 collection refuses them


@pytest.fixture(scope="module", params=list(MODES))
def mctx(request):
    """(mode, private context): f32_filter = 2 (every float32 call filters), 0 (K5 only), or untouched."""
    c = fastmatch_amd.Context(0)
    if MODES[request.param] is not None:
        c.set_option("f32_filter", MODES[request.param])
    yield request.param, c
    c.close()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else (a.view(np.uint64) if a.dtype == np.float64 else a)


def _same(a, b, what=""):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    assert np.array_equal(_bits(a), _bits(b)), what


@functools.lru_cache(maxsize=None)
def _data(name):
    Q, T = R.REGIMES[name][0]()
    Q.setflags(write=False); T.setflags(write=False)
    return Q, T


@functools.lru_cache(maxsize=None)
def _ref_knn(name, k):
    return oracle.bf_knn(*_data(name), k, order=1)


@functools.lru_cache(maxsize=None)
def _ref_x1_sd(name):
    Q, T = _data(name)
    return oracle.bf_xcheck1(Q, T, order=1), oracle.self_dist(Q, order=1)


def _stacked(Q, images, k):
    """_stacked_ref of test_collection_gpu.py: the oracle on the concatenated rows, hits mapped through the offsets."""
    T = np.concatenate(images)
    idx, dist = oracle.bf_knn(Q, T, k, order=1)
    fr = np.concatenate([[0], np.cumsum([im.shape[0] for im in images])]).astype(np.int64)
    img = np.searchsorted(fr, idx, side="right") - 1
    img = np.where(idx >= 0, img, -1).astype(np.int32)
    loc = np.where(idx >= 0, idx - fr[np.maximum(img, 0)], -1).astype(np.int32)
    return img, loc, dist


def _collection(c, images):
    col = c.collection()
    for i, im in enumerate(images):
        assert col.add(im) == i
    return col


def _check_collection(c, qb, Q, images, ks=(1, 2, 8)):
    with _collection(c, images) as col:
        for k in ks:
            got = col.knn(qb, k)
            for g, r, what in zip(got, _stacked(Q, images, k), ("img", "idx", "dist")):
                _same(g, r, "stacked k=%d %s" % (k, what))
        idx, dist = col.knn2_each(qb)
        for i, im in enumerate(images):
            ridx, rdist = oracle.bf_knn(Q, im, 2, order=1)
            _same(idx[i], ridx, "each idx, image %d" % i); _same(dist[i], rdist, "each dist, image %d" % i)


def _refused(call):
    with pytest.raises(fastmatch_amd.FastMatchHipError) as e:
        call()
    assert e.value.code == -4, e.value                       # FM_EUNSUPPORTED
    assert "2^57" in str(e.value)


# ---- 1. knn, xcheck1, self_dist ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_knn_xcheck1_selfdist(mctx, name):
    mode, c = mctx
    Q, T = _data(name)
    qb, tb = c.bank(Q), c.bank(T)
    assert qb.kind == tb.kind == fastmatch_amd._ffi.FM_BANK_F32
    before = c.f32_filter_stats()[0]
    idx, dist = c.knn2(qb, tb)
    after = c.f32_filter_stats()[0]
    oidx, odist = _ref_knn(name, 2)
    _same(idx, oidx, "knn2 idx"); _same(dist, odist, "knn2 dist")
    for k in (1, 2, 3, 8):
        idx, dist = c.knn(qb, tb, k)
        oidx, odist = _ref_knn(name, k)
        _same(idx, oidx, "knn k=%d idx" % k); _same(dist, odist, "knn k=%d dist" % k)
    (otidx, oxd), osd = _ref_x1_sd(name)
    tidx, xd = c.xcheck1(qb, tb)
    _same(tidx, otidx, "xcheck1 idx"); _same(xd, oxd, "xcheck1 dist")
    _same(c.self_dist(qb), osd, "self_dist")
    if mode == "filter":                                      # the knn2 call took the route the context names
        assert (after == before + 1) if R.REGIMES[name][1] else (after == before), (before, after)
    elif mode == "k5":
        assert after == before and c.f32_filter_stats()[0] == before
    if name == "nonfinite":                                   # what the oracle defines: inf / NaN distances are -1 / inf, last
        idx, dist = c.knn(qb, tb, 8)
        assert (idx[33] == -1).all() and np.isposinf(dist[33]).all() and not (idx == 17).any()
    qb.close(); tb.close()


# ---- 2. radius_match -----------------------------------------------------------------------------------------------------
def _radius_cases(name):
    _, full = _ref_knn(name, R.NT)
    cases = [("median5", np.float32(np.median(full[:, 5])))]
    for col in (0, 5, 40):
        cases.append(("col%d" % col, full[:, col].copy()))
    cases.append(("col5_next", np.nextafter(full[:, 5], np.float32(np.inf))))
    if name in ("overflow", "nonfinite"):
        cases.append(("inf", np.float32(np.inf)))
    return cases


@functools.lru_cache(maxsize=None)
def _radius_refs(name):
    Q, T = _data(name)
    return [(what, r, _radius_ref(Q, T, r)) for what, r in _radius_cases(name)]


@pytest.mark.parametrize("name", NAMES)
def test_radius_match(mctx, name):
    mode, c = mctx
    Q, T = _data(name)
    qb, tb = c.bank(Q), c.bank(T)
    for what, r, ref in _radius_refs(name):
        res = c.radius_match(qb, tb, r)
        _check_radius(res, ref)
        if what == "col5_next" and name not in ("overflow",):
            assert res[0][-1] >= 5 * (R.NQ - 1)              # (the lists are not empty: at least 6 rows lie within the 6th distance)
    qb.close(); tb.close()


# ---- 3. collections ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_collection(mctx, name):
    mode, c = mctx
    Q, T = _data(name)
    images = R.split_images(T)
    assert [im.shape[0] for im in images[:6]] == R.COLLECTION_SIZES and sum(im.shape[0] for im in images) == R.NT
    qb = c.bank(Q)
    if name in REFUSED:
        # never a silently different answer: the image is refused and the collection stays as it was, on every context
        with c.collection() as col:
            _refused(lambda: col.add(images[0]))
            assert col.info()[:2] == (0, 0)
            small = (images[0] * np.float32(2.0 ** -10)).astype(np.float32)
            assert col.add(small) == 0
            _refused(lambda: col.knn(qb, 2))
            _refused(lambda: col.knn2_each(qb))
            _refused(lambda: col.knn2_ratio(qb, 0.8))
            _refused(lambda: col.votes(qb, 0.8, 0))
            assert col.info()[:2] == (1, 129)
    else:
        before = c.f32_filter_stats()[0]
        _check_collection(c, qb, Q, images)
        after = c.f32_filter_stats()[0]
        if mode == "k5" or (mode == "filter" and not R.REGIMES[name][1]):
            assert after == before
        elif mode == "filter":
            assert after > before
    qb.close()


def _plant(Q, T, rng, sigma):
    """Near copies of every second query row among the train rows (accepted at tau 0.8) and one exact duplicate pair."""
    T = T.copy()
    for j in range(0, R.NQ, 2):
        T[3 * j + 1] = (Q[j].astype(np.float64) + rng.normal(0.0, sigma, Q.shape[1])).astype(np.float32)
    T[7] = T[8] = Q[11]                                       # a zero second distance: rejected
    return T


@pytest.mark.parametrize("name", ["signed", "offset"])
def test_collection_ratio_and_votes(mctx, name):
    mode, c = mctx
    Q, T = _data(name)
    images = R.split_images(_plant(Q, T, np.random.default_rng(7), 0.05))
    tau = 0.8

    def ratio(d0, d1, has2):
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(has2, d0.astype(np.float64) / d1.astype(np.float64), np.nan)
        return r, r < tau

    qb = c.bank(Q)
    with _collection(c, images) as col:
        rimg, ridx, rdist = _stacked(Q, images, 2)
        r, p = ratio(rdist[:, 0], rdist[:, 1], ridx[:, 1] >= 0)
        s = np.nonzero(p)[0]
        assert len(s) > 50 and not p[11]
        qidx, img, tidx, dist, rat = col.knn2_ratio(qb, tau)
        _same(qidx, s.astype(np.int32)); _same(img, rimg[s, 0]); _same(tidx, ridx[s, 0]); _same(dist, rdist[s, 0])
        _same(rat, r[s])
        _same(col.votes(qb, tau, 0), np.bincount(rimg[s, 0], minlength=len(images)).astype(np.int64))
        ref1 = []
        for im in images:
            ei, ed = oracle.bf_knn(Q, im, 2, order=1)
            ref1.append(int(ratio(ed[:, 0], ed[:, 1], ei[:, 1] >= 0)[1].sum()))
        _same(col.votes(qb, tau, 1), np.asarray(ref1, np.int64))
    qb.close()


def test_collection_rebuilt_under_a_new_scale_equals_a_fresh_one(mctx):
    """A first integer-valued float32 image starts the collection on the integer route; the next (signed) image rebuilds it
    on the float32 route, on the device, under the scale of both."""
    mode, c = mctx
    Q, T = _data("signed")
    first = np.random.default_rng(8).integers(0, 256, (130, R.DIM)).astype(np.float32)
    images = [first] + R.split_images(T)
    qb = c.bank(Q)
    with c.collection() as col:
        assert col.add(first) == 0 and col.info()[3] == fastmatch_amd._ffi.FM_BANK_I8
        for im in images[1:]:
            col.add(im)
        assert col.info()[3] == fastmatch_amd._ffi.FM_BANK_F32
        got = [col.knn(qb, k) for k in (1, 2, 8)]
        eidx, edist = col.knn2_each(qb)
    order = [1, 0] + list(range(2, len(images)))              # fresh: the float32 route from the first image on
    with _collection(c, [images[i] for i in order]) as fresh:
        fidx, fdist = fresh.knn2_each(qb)
    _same(eidx[order], fidx); _same(edist[order], fdist)
    for k, g in zip((1, 2, 8), got):
        for a, b in zip(g, _stacked(Q, images, k)):
            _same(a, b, "rebuilt, stacked k=%d" % k)
    for i, im in enumerate(images):
        ridx, rdist = oracle.bf_knn(Q, im, 2, order=1)
        _same(eidx[i], ridx); _same(edist[i], rdist)
    qb.close()


# ---- 4. the limit of a float32 collection (masking its padding rows by value) ------------------------------------------------
def test_padding_trap(mctx):
    """Query rows near 1e18 are closer to a collection's padding rows than to its real rows (test_f32_regimes_host.py): the
    match calls refuse the bank, the collection keeps answering, and query rows within the limit equal the oracle."""
    mode, c = mctx
    Q, images = R.padding_trap()
    h = R.NQ // 2
    qb, qlo = c.bank(Q), c.bank(Q[h:])
    with _collection(c, images) as col:
        for call in (lambda: col.knn(qb, 1), lambda: col.knn(qb, 2), lambda: col.knn(qb, 8), lambda: col.knn2_each(qb),
                     lambda: col.knn2_ratio(qb, 0.8), lambda: col.votes(qb, 0.8, 0), lambda: col.votes(qb, 0.8, 1)):
            _refused(call)
        assert col.info()[:2] == (3, 257)
    _check_collection(c, qlo, Q[h:], images)
    # image by image the plain entry points answer the whole bank: the oracle has two real rows for every query row
    for im in images[::2]:
        tb = c.bank(im, float_route=True)
        idx, dist = c.knn2(qb, tb)
        oidx, odist = oracle.bf_knn(Q, im, 2, order=1)
        assert (oidx >= 0).all()
        _same(idx, oidx); _same(dist, odist)
        tb.close()
    qb.close(); qlo.close()


def test_collection_limit_just_below_and_just_above(mctx):
    """Magnitudes of exactly 2^57 (FM_COLLECTION_F32_MAX), in images and in the query bank, equal the oracle; the next float32
    above is refused.  A non-finite value does not hide a finite one beyond the limit, nor count as one."""
    mode, c = mctx
    L = R.COLL_F32_MAX
    above = np.nextafter(L, np.float32(np.inf))
    rng = np.random.default_rng(9)
    T = np.clip(rng.normal(0, 1, (260, R.DIM)) * 1e17, -float(L), float(L)).astype(np.float32)
    T[5, 3], T[200, 127] = L, -L
    Q = np.clip(rng.normal(0, 1, (130, R.DIM)) * 1e16 + float(L) * rng.choice([-1.0, 1.0], (130, 1)), -float(L), float(L)).astype(np.float32)
    assert np.abs(T).max() == L and np.abs(Q).max() == L and (np.abs(Q) == L).sum() > 1000
    images = R.split_images(T, [129, 0, 1, 2], rest=True)
    qb = c.bank(Q)
    _check_collection(c, qb, Q, images)
    Qa, Ta = Q.copy(), images[0].copy()
    Qa[77, 9] = above
    Ta[128, 0] = -above
    Qi = Qa.copy(); Qi[3, 3] = np.inf                         # an inf beside the finite value beyond the limit
    Qf = Q.copy(); Qf[3, 3] = np.inf; Qf[4, 4] = np.nan       # non-finite values alone are not beyond it
    qa, qi, qf = c.bank(Qa), c.bank(Qi), c.bank(Qf)
    with _collection(c, images) as col:
        ref = col.knn(qb, 2)
        _refused(lambda: col.add(Ta))
        _refused(lambda: col.knn(qa, 2))
        _refused(lambda: col.knn(qi, 3))
        _refused(lambda: col.knn2_each(qi))
        assert col.info()[:2] == (len(images), 260)
        for a, b in zip(col.knn(qb, 2), ref):
            _same(a, b)
        for k in (2, 8):
            for a, b in zip(col.knn(qf, k), _stacked(Qf, images, k)):
                _same(a, b, "non-finite query values, k=%d" % k)
        Ti = images[0].copy(); Ti[0, 0] = np.inf              # an image with an inf (largest finite magnitude within the limit)
        assert col.add(Ti) == len(images)
        for a, b in zip(col.knn(qb, 8), _stacked(Q, images + [Ti], 8)):
            _same(a, b, "an image with an inf")
    for b in (qb, qa, qi, qf):
        b.close()
