"""GPU: masked radiusMatch against a train collection -- fm_collection_radius_match_masked(_dev), torchmatch's masks= -- on an
integer, a float32 and a binary collection of the images 700 / 1 / 130 / 0 / 1269 rows (padding behind four images, an empty
one), 300 query rows.  One image is left all-permitted, one all-forbidden.  The img / idx / dist lists are compared bit for bit
with tests/radius_masked_ref.py: the filtered lists of radius_coll_ref / hamming_radius_ref."""
import ctypes

import numpy as np
import pytest

from fastmatch_amd import _ffi
import radius_masked_ref as M

pytestmark = pytest.mark.gpu

P = ctypes.c_void_p
EINVAL, EUNSUPPORTED = -1, -4
INF = np.float32(np.inf)


def _ptr(a):
    return a.ctypes.data_as(P)


def _qbank(ctx, name, Q):
    return ctx.bank_binary(Q) if M.kind(name) == "ham" else ctx.bank(Q, float_route=name == "f32")


def _collection(ctx, name):
    c = ctx.collection()
    for i, im in enumerate(M.images(name)):
        assert (c.add_binary(im) if M.kind(name) == "ham" else c.add(im)) == i
    return c


def _set(mk, Mfull):
    for i, m in enumerate(M.per_image(Mfull)):
        if m is None:
            mk.set_all(True, img=i)
        else:
            mk.set(m, img=i)
    return mk


@pytest.fixture(scope="module", params=M.COLL_SETS)
def std(ctx, request):
    name = request.param
    qb, c = _qbank(ctx, name, M.data(name)[0]), _collection(ctx, name)
    assert c.info()[:2] == (len(M.SIZES), M.NT)
    yield name, qb, c
    c.close()
    qb.close()


def test_patterns_and_radii(std):
    name, qb, c = std
    for pattern in ("random", "band", "third", "walk", "first", "last", "zeros"):
        Mc = M.coll_mask(pattern)
        with c.mask(M.NQ) as mk:
            _set(mk, Mc)
            for what, r in M.radii(name) + [("inf", INF)]:
                M.same_coll(c.radius_match_masked(qb, mk, r), M.want(name, r, Mc), (name, pattern, what))


def test_all_ones_is_the_unmasked_call_and_all_zeros_is_empty(std):
    name, qb, c = std
    plain_call = c.hamming_radius_match if M.kind(name) == "ham" else c.radius_match
    with c.mask(M.NQ) as mk:
        for i in range(len(M.SIZES)):
            mk.set_all(True, img=i)
        for what, r in M.radii(name) + [("inf", INF)]:
            got, plain = c.radius_match_masked(qb, mk, r), plain_call(qb, r)
            for a, b in zip(got, plain):
                assert a.dtype == b.dtype and np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a,
                                                             b.view(np.uint32) if b.dtype == np.float32 else b), (name, what)
            M.same_coll(got, M.want(name, r, M.mask("ones")), (name, "ones", what))
        assert np.array_equal(np.diff(c.radius_match_masked(qb, mk, INF)[0]), np.full(M.NQ, M.NT))      # never a padding row
    with c.mask(M.NQ) as mk:                                                                              # a new mask forbids everything
        off, img, idx, dist = c.radius_match_masked(qb, mk, INF)
        assert not off.any() and img.size == idx.size == dist.size == 0


def test_device_form_and_torchmatch(ctx, std):
    import torch
    from fastmatch_amd import torchmatch
    name, qb, _ = std
    Mc = M.coll_mask("random")
    tc = torchmatch.Collection(context=ctx)
    try:
        for im in M.images(name):
            tc.add(torch.from_numpy(im.copy()).cuda(), **({"binary": True} if M.kind(name) == "ham" else {}))
        call = tc.hamming_radius_match if M.kind(name) == "ham" else tc.radius_match
        masks = [None if m is None else torch.from_numpy(m.copy()).cuda() for m in M.per_image(Mc)]
        for what, r in M.radii(name):
            rt = r if np.ndim(r) == 0 else torch.from_numpy(r).cuda()
            got = tuple(x.cpu().numpy() for x in call(qb, rt, masks=masks))
            M.same_coll(got, M.want(name, r, Mc), (name, "torch", what))
        with tc.mask(M.NQ) as mk:
            _set(mk, M.coll_mask("band"))
            got = tuple(x.cpu().numpy() for x in call(qb, float(M.radius(name)), masks=mk))
            M.same_coll(got, M.want(name, M.radius(name), M.coll_mask("band")), (name, "torch, resident"))
        with pytest.raises(ValueError, match="masks"):
            call(qb, 1.0, masks=masks[:-1])
    finally:
        tc.close()


def test_cap_and_errors(ctx, std):
    name, qb, c = std
    lib, h = ctx.lib, ctx.handle
    fn = lib.fm_collection_radius_match_masked
    r = M.radius(name)
    Mc = M.coll_mask("random")
    want = M.want(name, r, Mc)
    woff, total = want[0], int(want[0][-1])
    off = np.full(M.NQ + 1, -7, np.int64)
    tot = ctypes.c_int64(-5)

    def msg():
        m = lib.fm_last_error(h)
        return m.decode() if m else ""

    other = ctx.collection()
    other.add(M.images(name)[2]) if M.kind(name) != "ham" else other.add_binary(M.images(name)[2])
    try:
        with c.mask(M.NQ) as mk, ctx.mask(M.NQ, M.NT) as pm, other.mask(M.NQ) as om, c.mask(M.NQ + 1) as bad_nq:
            _set(mk, Mc)
            # counts only, a cap inside a row, cap = total
            assert fn(h, c.handle, qb.handle, mk.handle, None, float(r), 0, _ptr(off), None, None, None, ctypes.byref(tot)) == 0
            assert np.array_equal(off, woff) and tot.value == total
            row = int(np.searchsorted(woff, total // 2, side="right")) - 1
            cap = int(woff[row]) + 1 if woff[row + 1] - woff[row] > 1 else int(woff[row])
            fit = int(np.searchsorted(woff, cap, side="right")) - 1
            for cp, nfit in ((cap, fit), (total, M.NQ)):
                img, idx, dist = np.full(total + 3, -9, np.int32), np.full(total + 3, -9, np.int32), np.full(total + 3, -9.0, np.float32)
                assert fn(h, c.handle, qb.handle, mk.handle, None, float(r), cp, _ptr(off), _ptr(img), _ptr(idx), _ptr(dist), ctypes.byref(tot)) == 0
                n = int(woff[nfit])
                assert np.array_equal(off, woff) and tot.value == total
                assert np.array_equal(img[:n], want[1][:n]) and np.array_equal(idx[:n], want[2][:n])
                assert np.array_equal(M.bits(dist[:n]), M.bits(want[3][:n]))
                assert (img[max(n, cp):] == -9).all() and (idx[max(n, cp):] == -9).all() and (dist[max(n, cp):] == -9.0).all()
            # errors, in order; refused calls write nothing
            off[:] = -7
            tot.value = -5
            img, idx, dist = np.full(4, -9, np.int32), np.full(4, -9, np.int32), np.full(4, -9.0, np.float32)
            args = lambda m, cap=4, o=off: (h, c.handle, qb.handle, m, None, float(r), cap, _ptr(o) if o is not None else None,
                                            _ptr(img), _ptr(idx), _ptr(dist), ctypes.byref(tot))
            assert fn(*args(None)) == EINVAL and "mask is NULL" in msg()
            assert fn(h, None, qb.handle, mk.handle, None, float(r), 4, _ptr(off), _ptr(img), _ptr(idx), _ptr(dist), ctypes.byref(tot)) == EINVAL
            for m, word in ((pm, "made for a bank pair"), (om, "another collection"), (bad_nq, "query rows")):
                assert fn(*args(m.handle, cap=-1, o=None)) == EINVAL and word in msg(), (word, msg())
            assert fn(*args(mk.handle, cap=-1)) == EINVAL and "cap is negative" in msg()
            assert fn(*args(mk.handle, o=None)) == EINVAL and "offsets is NULL" in msg()
            assert lib.fm_collection_radius_match_masked_dev(*(args(mk.handle) + (None,))) == EINVAL and "d_offsets" in msg()
            assert (off == -7).all() and (img == -9).all() and (idx == -9).all() and (dist == -9.0).all() and tot.value == -5
    finally:
        other.close()


def test_a_stale_mask_and_a_wide_collection_are_refused(ctx):
    import wide_ref
    Q, T = M.data("i8")
    qb = ctx.bank(Q)
    c = ctx.collection()
    off = np.full(M.NQ + 1, -7, np.int64)
    tot = ctypes.c_int64(-5)
    try:
        c.add(T[:100].copy())
        with c.mask(M.NQ) as mk:
            mk.set_all(True, img=0)
            assert c.radius_match_masked(qb, mk, INF)[0][-1] == 100 * M.NQ
            c.add(T[100:130].copy())                                      # a later add: the mask is stale
            rc = ctx.lib.fm_collection_radius_match_masked(ctx.handle, c.handle, qb.handle, mk.handle, None, 1.0, 0, _ptr(off), None, None, None,
                                                           ctypes.byref(tot))
            assert rc == EINVAL and "has changed" in ctx.lib.fm_last_error(ctx.handle).decode()
        Qw, Tw = wide_ref.clustered(8, 40, 160, 3)
        w, qw = ctx.collection(), ctx.bank(np.ascontiguousarray(Qw))
        try:
            w.add_wide(np.ascontiguousarray(Tw))
            with ctx.mask(8, 40) as pm:
                for fn, extra in ((ctx.lib.fm_collection_radius_match_masked, ()), (ctx.lib.fm_collection_radius_match_masked_dev, (None,))):
                    rc = fn(ctx.handle, w.handle, qw.handle, pm.handle, None, 1.0, 0, _ptr(off), None, None, None, ctypes.byref(tot), *extra)
                    assert rc == EUNSUPPORTED and "wide" in ctx.lib.fm_last_error(ctx.handle).decode()
        finally:
            w.close()
            qw.close()
        assert (off == -7).all() and tot.value == -5
    finally:
        c.close()
        qb.close()
