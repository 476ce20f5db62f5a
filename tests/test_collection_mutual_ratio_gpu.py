"""GPU: mutual nearest neighbours + ratio test on a train collection, image by image (fm_collection_mutual_ratio_each, its
device form, Collection.mutual_ratio_votes, BFMatcher.mutualRatioMatchEach, torchmatch.Collection.mutual_ratio_each): slot i
equals Context.mutual_ratio(q, bank(image i)), bit for bit, and the NumPy reference (tests/mutual_ratio_ref.py)."""
import os
import sys

import numpy as np
import pytest

from fastmatch_amd import _ffi, matchutil, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f32_regimes                              # noqa: E402
import mutual_ratio_ref as ref                  # noqa: E402
from kat import far_banks, SQRT_TIE_MIN         # noqa: E402

pytestmark = pytest.mark.gpu

EINVAL, EUNSUP = -1, -4
INF = float("inf")
BOUNDARY_SIZES = [0, 1, 127, 128, 129, 1000, 5, 0]
NQS = (0, 1, 100, 700)
KINDS = ("u8", "f32int", "f32", "f32nofilter", "bin1", "bin32", "bin64")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want, what):
    assert np.array_equal(got[0], want[0]), what + ": query rows"
    assert np.array_equal(got[1], want[1]), what + ": train rows"
    assert np.array_equal(_bits(got[2]), _bits(want[2])), what + ": distances"
    assert np.array_equal(np.asarray(got[3]).view(np.uint64), np.asarray(want[3]).view(np.uint64)), what + ": ratios"


def _plant(images, Q, noisy):
    """A row twice in one image and once more in another, and query rows that are noisy copies of image rows -- some image rows
    with two views -- so that accepted rows, shared first neighbours and failed reverse ratios exist in every larger image."""
    big, small = images[5], images[4]
    big[7] = big[3]
    small[0] = big[3]
    nq = Q.shape[0]
    for j in range(0, nq, 3):
        im = images[(2, 3, 4, 5, 6)[(j // 3) % 5]]
        Q[j] = noisy(im[(j * 7) % im.shape[0]])
    for j in range(1, nq, 15):
        im = images[(2, 3, 4, 5, 6)[((j - 1) // 3) % 5]]
        Q[j] = noisy(im[((j - 1) * 7) % im.shape[0]])
    Q[10] = big[3]; Q[20] = big[3]


def _data(kind):
    """(images, Q [700], binary, float_route) of a kind; deterministic."""
    rng = np.random.default_rng(4100 + KINDS.index(kind))
    nq = max(NQS)
    if kind.startswith("bin"):
        w = int(kind[3:])
        images = [rng.integers(0, 256, (n, w), dtype=np.uint8) for n in BOUNDARY_SIZES]
        Q = rng.integers(0, 256, (nq, w), dtype=np.uint8)

        def noisy(row):
            out = row.copy()
            out[rng.integers(0, w)] ^= np.uint8(1 << rng.integers(0, 8))
            return out
        _plant(images, Q, noisy)
        return images, Q, True, False
    if kind in ("u8", "f32int"):
        images = [synth.synth_sift(max(n, 1), rng)[:n].copy() for n in BOUNDARY_SIZES]
        Q = synth.synth_sift(nq, rng)
        _plant(images, Q, lambda row: np.clip(row.astype(np.int32) + rng.integers(-3, 4, row.shape), 0, 255).astype(np.uint8))
        if kind == "f32int":
            images, Q = [im.astype(np.float32) for im in images], Q.astype(np.float32)
        return images, Q, False, False
    images = [f32_regimes._gauss(4200 + i, n).astype(np.float32) for i, n in enumerate(BOUNDARY_SIZES)]
    Q = f32_regimes._gauss(4300, nq).astype(np.float32)
    _plant(images, Q, lambda row: (row + rng.normal(0.0, 0.01, row.shape)).astype(np.float32))
    if kind == "f32nofilter":
        far = f32_regimes.qt_apart(45)[0][:127].copy()     # leaves fp16's range under the collection's scale: no filter
        images[2] = far
    return images, Q, False, True


def _qbank(ctx, Q, binary, float_route):
    return ctx.bank_binary(Q) if binary else ctx.bank(Q, float_route=float_route)


def _collection(ctx, images, binary):
    c = ctx.collection()
    for i, im in enumerate(images):
        assert (c.add_binary(im) if binary else c.add(im)) == i
    return c


def _per_image(ctx, qb, images, binary, float_route, tau, sym):
    out = []
    for im in images:
        tb = _qbank(ctx, im, binary, float_route)
        out.append(ctx.mutual_ratio(qb, tb, tau, sym))
        tb.close()
    return out


@pytest.mark.parametrize("nq", NQS)
@pytest.mark.parametrize("kind", KINDS)
def test_slot_i_equals_the_pair_call(ctx, kind, nq):
    images, Qall, binary, float_route = _data(kind)
    coll = _collection(ctx, images, binary)
    qb = _qbank(ctx, Qall[:nq], binary, float_route)
    try:
        ctx.set_option("f32_filter", 2 if kind in ("f32", "f32nofilter") else 1)
        assert coll.info()[3] == (_ffi.FM_BANK_BIN if binary else _ffi.FM_BANK_F32 if float_route else _ffi.FM_BANK_I8)
        for tau in (0.8, INF):
            for sym in (False, True):
                got = coll.mutual_ratio_each(qb, tau, sym)
                want = _per_image(ctx, qb, images, binary, float_route, tau, sym)
                assert len(got) == len(images)
                for i in range(len(images)):
                    _same(got[i], want[i], "%s nq=%d tau=%s sym=%d image %d" % (kind, nq, tau, sym, i))
                votes = coll.mutual_ratio_votes(qb, tau, sym)
                assert votes.tolist() == [g[0].shape[0] for g in got]
                assert votes[0] == 0 and votes[7] == 0 and votes[1] == 0       # empty images; a one-row image has no ratio
        if not float_route and kind != "bin1":
            r = ref.mutual_ratio_each(Qall[:nq].astype(np.uint8) if kind == "f32int" else Qall[:nq],
                                      [im.astype(np.uint8) if kind == "f32int" else im for im in images], 0.8, True, binary)
            got = coll.mutual_ratio_each(qb, 0.8, True)
            for i in range(len(images)):
                _same(got[i], r[i], "%s nq=%d image %d against the reference" % (kind, nq, i))
        if nq == 700 and kind != "bin1":
            assert coll.mutual_ratio_votes(qb, 0.8)[5] >= 10
    finally:
        ctx.set_option("f32_filter", 1)
        qb.close()
        coll.close()


def test_a_descriptor_in_two_images_is_accepted_in_both(ctx):
    rng = np.random.default_rng(4400)
    A, B = synth.synth_sift(300, rng), synth.synth_sift(200, rng)
    Q = synth.synth_sift(50, rng)
    B[17] = A[5]
    Q[9] = A[5]
    coll = _collection(ctx, [A, B], False)
    qb = ctx.bank(Q)
    try:
        got = coll.mutual_ratio_each(qb, 0.8, True)
        for i, row in ((0, 5), (1, 17)):
            at = np.nonzero(got[i][0] == 9)[0]
            assert at.shape[0] == 1 and got[i][1][at[0]] == row and got[i][2][at[0]] == 0.0 and got[i][3][at[0]] == 0.0
        m = matchutil.BFMatcher()
        m.add([A, B])
        lists = m.mutualRatioMatchEach(Q, 0.8, symmetric=True)
        assert [[(d.queryIdx, d.trainIdx, d.imgIdx) for d in l] for l in lists] == \
               [[(int(q), int(t), i) for q, t in zip(got[i][0], got[i][1])] for i in range(2)]
        arr = matchutil.mutual_ratio_match_arrays(Q, B, 0.8, symmetric=True)
        _same(arr, got[1], "matchutil.mutual_ratio_match_arrays")
    finally:
        qb.close()
        coll.close()


def test_float32_root_ties_in_one_image_of_several(ctx):
    rng = np.random.default_rng(4500)
    Q, far = far_banks(300, 500, rng)
    near0 = np.zeros((400, 128), np.uint8)
    near0[:, 101:111] = rng.integers(0, 3, (400, 10), dtype=np.uint8)
    near1 = near0[::-1][:129].copy()
    images = [near0, far, near1]
    assert int((far.astype(np.int64) ** 2).sum(1).max()) >= SQRT_TIE_MIN
    coll = _collection(ctx, images, False)
    qb = ctx.bank(Q)
    try:
        for sym in (False, True):
            got = coll.mutual_ratio_each(qb, INF, sym)
            want = ref.mutual_ratio_each(Q, images, INF, sym)
            pair = _per_image(ctx, qb, images, False, False, INF, sym)
            for i in range(3):
                _same(got[i], want[i], "image %d sym=%d against the reference" % (i, sym))
                _same(got[i], pair[i], "image %d sym=%d against the pair call" % (i, sym))
        assert got[1][0].shape[0] > 0
    finally:
        qb.close()
        coll.close()


@pytest.mark.parametrize("kind", ("u8", "f32", "bin32"))
def test_candidate_chunks_do_not_change_the_result(ctx, kind):
    """"coll_ws_bytes" small enough for at least three chunks of candidates: the header states the gathered bytes per
    candidate (132 integer route, 776 float32 route, 80 per 16 bytes of a binary row), chunks are whole 128-row stages."""
    images, Qall, binary, float_route = _data(kind)
    per = {"u8": 132, "f32": 776, "bin32": 160}[kind]
    coll = _collection(ctx, images, binary)
    qb = _qbank(ctx, Qall, binary, float_route)
    try:
        want = coll.mutual_ratio_each(qb, INF, True)
        n_cand = int(coll.votes(qb, INF, 1).sum())            # the (image, query row) entries that pass the forward test
        for budget in (65536, 1):                             # 65536 bytes: 384 / 0 -> 128 / 384 rows per chunk; 1 byte: one stage
            rows = max(128, budget // per // 128 * 128)
            assert n_cand >= 3 * rows
            ctx.set_option("coll_ws_bytes", budget)
            got = coll.mutual_ratio_each(qb, INF, True)
            for i in range(len(images)):
                _same(got[i], want[i], "%s budget %d image %d" % (kind, budget, i))
    finally:
        ctx.set_option("coll_ws_bytes", 0)
        qb.close()
        coll.close()


def test_refusals_in_order(ctx):
    import ctypes
    rng = np.random.default_rng(4600)
    coll = _collection(ctx, [synth.synth_sift(200, rng)], False)
    qb, wide = ctx.bank(synth.synth_sift(10, rng)), ctx.bank(rng.integers(0, 255, (10, 64), dtype=np.uint8))
    bb = ctx.bank_binary(np.zeros((4, 32), np.uint8))
    lib, h = ctx.lib, ctx.handle
    n = np.zeros(1, np.int64)
    a = [_ffi._ptr(np.zeros(10, t)) for t in (np.int32, np.int32, np.float32, np.float64)]
    try:
        assert lib.fm_collection_mutual_ratio_each(h, None, qb.handle, 0.8, 0, 10, *a, _ffi._ptr(n)) == EINVAL
        assert lib.fm_collection_mutual_ratio_each(h, coll.handle, None, 0.8, 0, 10, *a, _ffi._ptr(n)) == EINVAL
        assert lib.fm_collection_mutual_ratio_each(h, coll.handle, bb.handle, 0.8, 0, -1, *a, _ffi._ptr(n)) == EINVAL      # kind first
        assert "kind" in lib.fm_last_error(h).decode()
        assert lib.fm_collection_mutual_ratio_each(h, coll.handle, wide.handle, 0.8, 0, -1, *a, _ffi._ptr(n)) == EINVAL
        assert "width" in lib.fm_last_error(h).decode()
        assert lib.fm_collection_mutual_ratio_each(h, coll.handle, qb.handle, 0.8, 0, -1, *a, _ffi._ptr(n)) == EINVAL
        assert lib.fm_collection_mutual_ratio_each(h, coll.handle, qb.handle, 0.8, 0, 10, *a, None) == EINVAL
        assert lib.fm_collection_mutual_ratio_each(h, coll.handle, qb.handle, 0.8, 0, 10, a[0], None, a[2], a[3], _ffi._ptr(n)) == EINVAL
        NOS = _ffi._stream_arg(None)
        assert lib.fm_collection_mutual_ratio_each_dev(h, coll.handle, qb.handle, 0.8, 0, 10, None, None, None, NOS) == EINVAL
        assert lib.fm_collection_mutual_ratio_each_dev(h, coll.handle, qb.handle, 0.8, 0, 10, a[0], a[1], None, NOS) == EINVAL   # host memory
        assert coll.mutual_ratio_votes(qb, INF).shape == (1,)
    finally:
        for b in (qb, wide, bb):
            b.close()
        coll.close()


@pytest.mark.parametrize("kind", ("u8", "f32", "bin32"))
def test_device_forms_equal_the_host_form(ctx, kind):
    import torch
    from fastmatch_amd import torchmatch
    images, Qall, binary, float_route = _data(kind)
    coll = _collection(ctx, images, binary)
    qb = _qbank(ctx, Qall, binary, float_route)
    ni, nq = len(images), qb.n
    try:
        for tau, sym in ((0.8, False), (INF, True), (0.0, False)):
            want = coll.mutual_ratio_each(qb, tau, sym)
            full = np.array([w[0].shape[0] for w in want])
            small = max(1, int(full[5]) // 2)                          # below the largest image's count
            for cap in (nq, small, 0):
                rows = torch.full((ni, cap, 3), -7, dtype=torch.int32, device="cuda")
                counts = torch.full((ni,), -7, dtype=torch.int64, device="cuda")
                hc = np.full(ni, -7, np.int64)
                coll.mutual_ratio_each_dev(qb, tau, sym, rows.data_ptr() if cap else 0, counts.data_ptr(), cap, h_counts=hc,
                                           consumer_stream=torch.cuda.current_stream().cuda_stream)
                assert hc.tolist() == full.tolist()
                assert counts.cpu().numpy().tolist() == np.minimum(full, cap).tolist()
                got = rows.cpu().numpy()
                for i in range(ni):
                    k = min(int(full[i]), cap)
                    assert np.array_equal(got[i, :k, 0], want[i][0][:k]) and np.array_equal(got[i, :k, 1], want[i][1][:k])
                    assert np.array_equal(got[i, :k, 2].view(np.uint32), _bits(want[i][2][:k])) and (got[i, k:] == -7).all()
        # torchmatch: a collection fed from tensors, the query a tensor, on a non-default current stream
        side = torch.cuda.Stream()
        with torch.cuda.stream(side), torchmatch.Collection(context=ctx) as tc:
            for im in images:
                tc.add(torch.from_numpy(im).cuda(), binary=binary)
            want = coll.mutual_ratio_each(qb, 0.8, True)
            rows, counts = tc.mutual_ratio_each(torch.from_numpy(Qall).cuda(), 0.8, symmetric=True)
            assert rows.shape == (ni, nq, 3) and counts.cpu().numpy().tolist() == [w[0].shape[0] for w in want]
            got = rows.cpu().numpy()
            for i in range(ni):
                k = want[i][0].shape[0]
                assert np.array_equal(got[i, :k, 0], want[i][0]) and np.array_equal(got[i, :k, 1], want[i][1])
                assert np.array_equal(got[i, :k, 2].view(np.uint32), _bits(want[i][2]))
        side.synchronize()
    finally:
        qb.close()
        coll.close()
