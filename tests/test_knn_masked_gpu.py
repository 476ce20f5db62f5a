"""GPU: knnMatch under a mask (fm_mask_*, fm_knn_masked(_dev), fm_collection_knn_masked(_dev), matchutil's ``mask`` / ``masks``,
torchmatch's ``mask=`` / ``masks=``), bit for bit against references that do not come from the code under test: fm_knn on the
permitted rows (the existing, oracle-tested path), ``oracle.bf_knn`` on the CPU, and the NumPy brute force of
tests/masked_ref.py.  Sizes are chosen where the kernels can go wrong: word and stage edges, more than one workgroup, several
splits of the train range, both sides of the k = 2 / k = 3 kernel switch, all three bank kinds."""
import os
import sys

import numpy as np
import pytest

import fastmatch_amd
from fastmatch_amd import _ffi, matchutil, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oracle                                    # noqa: E402
import hamming_ref as H                          # noqa: E402
import masked_ref as R                           # noqa: E402
from kat import far_banks, sqrt_tie_knn2_cases   # noqa: E402

pytestmark = pytest.mark.gpu

KINDS = ["u8", "f32", "bin"]
FM_EINVAL, FM_EUNSUPPORTED = -1, -4


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want, what=""):
    for g, w in zip(got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, (what, g.shape, w.shape)
        if g.dtype == np.float32 or w.dtype == np.float32:
            bad = np.nonzero(_bits(g) != _bits(w))
        else:
            bad = np.nonzero(g != w)
        assert bad[0].size == 0, (what, [b[:5] for b in bad], g[bad][:5], w[bad][:5])


def _rows(rng, n, kind):
    if kind == "bin":
        return rng.integers(0, 256, (n, 32), dtype=np.uint8)
    a = synth.synth_sift(max(n, 1), rng)[:n].copy()
    if kind == "f32":
        a = (a + rng.uniform(-0.5, 0.5, a.shape)).astype(np.float32)
    return a


def _bank(ctx, a, kind):
    return ctx.bank_binary(a) if kind == "bin" else ctx.bank(a)


def _ref_knn(kind, Q, T, k):
    if kind == "bin":
        i, d = H.knn(Q, T, k)
        return np.asarray(i, np.int32), np.asarray(d, np.float32)
    return oracle.bf_knn(Q, T, k, order=1 if kind == "f32" else 0)


def _masked(ctx, qb, tb, m, k):
    with ctx.mask(qb.n, tb.n) as mk:
        return ctx.knn_masked(qb, tb, mk.set(m), k)


def _ascending(idx, dist):
    """every list ascends strictly by (float32 bits, index) up to its -1 / +inf tail"""
    key = (_bits(dist).astype(np.int64) << 32) | (idx.astype(np.int64) & 0xffffffff)
    for i in range(idx.shape[0]):
        n = int((idx[i] >= 0).sum())
        assert (idx[i, n:] == -1).all() and np.isinf(dist[i, n:]).all()
        assert (np.diff(key[i, :n]) > 0).all(), (i, idx[i], dist[i])


# 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", [(1, 1), (5, 3), (17, 15), (127, 129), (129, 127), (257, 1100)])
def test_all_ones_mask_equals_fm_knn_bit_for_bit(ctx, kind, shape):
    rng = np.random.default_rng(shape[0] * 7 + shape[1])
    nq, nt = shape
    qb, tb = _bank(ctx, _rows(rng, nq, kind), kind), _bank(ctx, _rows(rng, nt, kind), kind)
    with ctx.mask(nq, nt) as by_bytes, ctx.mask(nq, nt) as by_fill:
        by_bytes.set(np.ones((nq, nt), np.uint8))
        by_fill.set_all(True)
        assert by_bytes.info() == (nq, nt, 0, nq * (R.pad128(nt) // 64) * 8)
        for k in range(1, 9):
            want = ctx.knn(qb, tb, k)
            _same(ctx.knn_masked(qb, tb, by_bytes, k), want, (kind, shape, k))
            _same(ctx.knn_masked(qb, tb, by_fill, k), want, (kind, shape, k, "set_all"))
        if kind == "u8":                # the masked vector-ALU instantiations K = 1, 2 serve the same answer
            ctx.set_option("masked_mfma", 0)
            try:
                for k in (1, 2):
                    _same(ctx.knn_masked(qb, tb, by_bytes, k), ctx.knn(qb, tb, k), (shape, k, "K9"))
            finally:
                ctx.set_option("masked_mfma", 1)
        by_fill.set_all(False)
        idx, dist = ctx.knn_masked(qb, tb, by_fill, 2)
        assert (idx == -1).all() and np.isinf(dist).all()
    qb.close(), tb.close()


def test_host_masks_in_chunks_and_with_a_row_pitch(ctx):
    """fm_mask_set_u8 stages at most 64 MiB of query rows at a time: 1000 x 70 000 bytes go up in two chunks (958 + 42 rows).
    Every row permits one train row of its own, so a row's only neighbour says where its bits landed."""
    rng = np.random.default_rng(12)
    nq, nt = 1000, 70000
    Q, T = rng.integers(0, 256, (nq, 128), dtype=np.uint8), rng.integers(0, 256, (nt, 128), dtype=np.uint8)
    cols = rng.integers(0, nt, nq)
    cols[[0, 957, 958, 999]] = [nt - 1, 0, nt - 1, 63]            # the chunk border's rows, the mask's corners
    m = np.zeros((nq, nt), np.uint8)
    m[np.arange(nq), cols] = 1
    d = np.sqrt(((Q.astype(np.int64) - T[cols].astype(np.int64)) ** 2).sum(1).astype(np.float32))
    qb, tb = ctx.bank(Q), ctx.bank(T)
    for k in (2, 3):
        idx, dist = _masked(ctx, qb, tb, m, k)
        _same((idx[:, 0], dist[:, 0]), (cols.astype(np.int32), d), ("chunks", k))
        assert (idx[:, 1:] == -1).all() and np.isinf(dist[:, 1:]).all()
    qb.close(), tb.close()
    # a column slice of a wider host array: rows `pitch` bytes apart, read without a dense copy
    nq, nt = 37, 300
    Q, T = _rows(rng, nq, "u8"), _rows(rng, nt, "u8")
    wide = (rng.random((nq, nt + 50)) < 0.3).astype(np.uint8)
    sl = wide[:, 20:20 + nt]
    assert not sl.flags.c_contiguous
    qb, tb = ctx.bank(Q), ctx.bank(T)
    _same(_masked(ctx, qb, tb, sl, 2), R.knn_u8(Q, T, sl, 2), "pitch")
    qb.close(), tb.close()


def test_masks_larger_than_one_launch_are_packed_in_several(ctx):
    """A launch of the pack / fill kernels covers at most "mask_pack_words" words (2^26 - 4: fewer than 2^32 work-items); with
    the option at 64 a 37 x 300 mask (6 words per row) takes 4 launches of 10 rows, a 2 x 5000 one (80 words per row) one row
    per launch.  Host bytes, device bytes and set_all must leave the bits a single launch leaves."""
    import torch
    assert ctx.get_option("mask_pack_words") == (1 << 26) - 4
    rng = np.random.default_rng(14)
    dev = torch.device("cuda", ctx.device)
    for nq, nt in ((37, 300), (2, 5000)):
        Q, T = _rows(rng, nq, "u8"), _rows(rng, nt, "u8")
        m = (rng.random((nq, nt)) < 0.1).astype(np.uint8)
        qb, tb = ctx.bank(Q), ctx.bank(T)
        want, full = R.knn_u8(Q, T, m, 3), ctx.knn(qb, tb, 3)
        ctx.set_option("mask_pack_words", 64)
        try:
            with ctx.mask(nq, nt) as mk:
                _same(ctx.knn_masked(qb, tb, mk.set(m), 3), want, (nq, nt, "host"))
                _same(ctx.knn_masked(qb, tb, mk.set_all(True), 3), full, (nq, nt, "set_all"))
                tm = torch.from_numpy(m).to(dev)
                mk.set_dev(tm.data_ptr(), pitch=tm.stride(0), stream=torch.cuda.current_stream().cuda_stream)
                _same(ctx.knn_masked(qb, tb, mk, 3), want, (nq, nt, "device"))
                idx, _ = ctx.knn_masked(qb, tb, mk.set_all(False), 3)
                assert (idx == -1).all()
        finally:
            ctx.set_option("mask_pack_words", (1 << 26) - 4)
        qb.close(), tb.close()
    with pytest.raises(fastmatch_amd.FastMatchHipError):
        ctx.set_option("mask_pack_words", 1 << 26)          # 2^32 work-items: not a launch


# 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_column_subsets_equal_fm_knn_on_the_subset_and_the_oracle(ctx, kind):
    rng = np.random.default_rng(21)
    nq, nt = 300, 2500
    Q, T = _rows(rng, nq, kind), _rows(rng, nt, kind)
    groups = [(np.arange(0, 100), np.sort(rng.choice(nt, 1200, replace=False))),
              (np.arange(100, 170), np.sort(rng.choice(nt, 5, replace=False))),
              (np.arange(170, 300), np.arange(1900, 2500))]
    m = np.zeros((nq, nt), np.uint8)
    for rows, S in groups:
        m[np.ix_(rows, S)] = 1
    qb, tb = _bank(ctx, Q, kind), _bank(ctx, T, kind)
    with ctx.mask(nq, nt) as mk:
        mk.set(m)
        for k in (1, 2, 3, 8):
            idx, dist = ctx.knn_masked(qb, tb, mk, k)
            for rows, S in groups:
                qg, tg = _bank(ctx, Q[rows], kind), _bank(ctx, T[S], kind)
                gi, gd = ctx.knn(qg, tg, k)
                oi, od = _ref_knn(kind, Q[rows], T[S], k)
                qg.close(), tg.close()
                for (si, sd), who in (((gi, gd), "fm_knn"), ((oi, od), "oracle")):
                    _same((idx[rows], dist[rows]), (np.where(si >= 0, S[np.maximum(si, 0)], -1).astype(np.int32), sd), (kind, k, who))
    qb.close(), tb.close()


# 3 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("density", [0.5, 0.02])
def test_per_row_random_masks_against_the_reference(ctx, kind, density):
    rng = np.random.default_rng(int(density * 100) + 31)
    nq, nt = (70 if kind == "f32" else 257), 1100
    Q, T = _rows(rng, nq, kind), _rows(rng, nt, kind)
    m = (rng.random((nq, nt)) < density).astype(np.uint8)
    ri, rd = R.knn(kind, Q, T, m, 8)                 # (a k-NN list is a prefix of the (k + 1)-NN list: one reference for every k)
    qb, tb = _bank(ctx, Q, kind), _bank(ctx, T, kind)
    with ctx.mask(nq, nt) as mk:
        mk.set(m)
        for k in (1, 2, 3, 8):
            got = ctx.knn_masked(qb, tb, mk, k)
            _same(got, (ri[:, :k], rd[:, :k]), (kind, density, k))
            _ascending(*got)
    qb.close(), tb.close()


# 4 ---------------------------------------------------------------------------------------------------------------------
def _edge_mask(nq, nt):
    m = np.zeros((nq, nt), np.uint8)
    for i in range(nq):
        c = i % 6
        if c == 1:
            m[i, nt // 2] = 1                        # exactly one train row
        elif c == 2:
            m[i, 0] = 1                              # only bit 0 of word 0
        elif c == 3:
            m[i, min(63, nt - 1)] = 1                # only bit 63 (or the last row of a shorter bank)
        elif c == 4:
            m[i, nt - 1] = 1                         # only the last real row
        elif c == 5:
            m[i, [0, nt - 1]] = 1
    return m                                         # (rows 0, 6, ...: nothing permitted)


@pytest.mark.parametrize("nt", [63, 64, 65, 127, 128, 129])
def test_word_and_stage_edges(ctx, nt):
    rng = np.random.default_rng(nt)
    T = {kind: _rows(rng, nt, kind) for kind in KINDS}
    tb = {kind: _bank(ctx, T[kind], kind) for kind in KINDS}
    for nq in (1, 15, 17, 255, 257):
        m = _edge_mask(nq, nt)
        for kind in (KINDS if nq == 17 else ["u8"]):
            Q = _rows(rng, nq, kind)
            qb = _bank(ctx, Q, kind)
            for k in (1, 2, 3):
                got = _masked(ctx, qb, tb[kind], m, k)
                _same(got, R.knn(kind, Q, T[kind], m, k), (kind, nq, nt, k))
            idx, dist = _masked(ctx, qb, tb[kind], m, 2)
            assert (idx[0] == -1).all() and np.isinf(dist[0]).all()                    # nothing permitted
            if nq > 1:
                assert idx[1, 0] == nt // 2 and idx[1, 1] == -1 and np.isinf(dist[1, 1])   # one row: the second slot is empty
            qb.close()
    for b in tb.values():
        b.close()


# 5 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_answers_come_out_of_other_splits(ctx, kind):
    rng = np.random.default_rng(55)
    nq, nt = 10, 5000
    Q, T = _rows(rng, nq, kind), _rows(rng, nt, kind)
    qb, tb = _bank(ctx, Q, kind), _bank(ctx, T, kind)
    best, _ = ctx.knn(qb, tb, 2)
    m = np.ones((nq, nt), np.uint8)
    m[np.arange(nq)[:, None], best] = 0              # the unmasked best and second best of every row are forbidden
    for k in (1, 2, 3):
        got = _masked(ctx, qb, tb, m, k)
        _same(got, R.knn(kind, Q, T, m, k), (kind, k))
        assert not (got[0][:, :, None] == best[:, None, :]).any()
    qb.close(), tb.close()


# 6 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_identical_train_rows_win_in_index_order_under_a_mask(ctx, kind):
    rng = np.random.default_rng(66)
    nt = 200
    T = _rows(rng, nt, kind)
    j1, j2, j3 = 5, 70, 133
    T[j2] = T[j1]
    T[j3] = T[j1]
    Q = T[[j1]].copy()
    qb, tb = _bank(ctx, Q, kind), _bank(ctx, T, kind)
    for forbidden, first in (((), [j1, j2, j3]), ((j1,), [j2, j3]), ((j1, j2), [j3]), ((j2,), [j1, j3])):
        m = np.ones((1, nt), np.uint8)
        m[0, list(forbidden)] = 0
        for k in (2, 3):
            idx, dist = _masked(ctx, qb, tb, m, k)
            n = min(k, len(first))
            assert idx[0, :n].tolist() == first[:n] and (dist[0, :n] == 0).all(), (kind, forbidden, k, idx)
            _same((idx, dist), R.knn(kind, Q, T, m, k), (kind, forbidden, k))
    qb.close(), tb.close()


def test_float32_root_ties_under_a_mask(ctx):
    for name, Q, T, _, _ in sqrt_tie_knn2_cases():
        qb, tb = ctx.bank(Q), ctx.bank(T)
        for f in range(T.shape[0]):
            m = np.ones((1, T.shape[0]), np.uint8)
            m[0, f] = 0
            for mfma in (1, 0):
                ctx.set_option("masked_mfma", mfma)
                try:
                    for k in (1, 2):
                        got = _masked(ctx, qb, tb, m, k)
                        _same(got, R.knn_u8(Q, T, m, k), (name, f, k, mfma))
                        _ascending(*got)
                finally:
                    ctx.set_option("masked_mfma", 1)
        qb.close(), tb.close()
    # every distance in the tie range, many candidates on both sides of a tie, half of them forbidden
    rng = np.random.default_rng(67)
    Q, T = far_banks(40, 700, rng)
    m = (rng.random((40, 700)) < 0.5).astype(np.uint8)
    qb, tb = ctx.bank(Q), ctx.bank(T)
    ri, rd = R.knn_u8(Q, T, m, 8)
    for k in (1, 2, 3, 8):
        got = _masked(ctx, qb, tb, m, k)
        _same(got, (ri[:, :k], rd[:, :k]), ("far", k))
        _ascending(*got)
    qb.close(), tb.close()


# 7 ---------------------------------------------------------------------------------------------------------------------
SIZES = [300, 0, 128, 1, 65, 129, 700]


def _coll(ctx, images, kind):
    c = ctx.collection()
    for im in images:
        c.add_binary(im) if kind == "bin" else c.add(im)
    return c


def _coll_masks(rng, nq):
    masks = [(rng.random((nq, n)) < 0.3).astype(np.uint8) for n in SIZES]
    masks[2] = None                                  # everything permitted
    masks[4] = np.zeros((nq, SIZES[4]), np.uint8)    # an all-forbidden image
    return masks


def _fill(mk, masks):
    for i, m in enumerate(masks):
        if m is None:
            mk.set_all(True, img=i)
        else:
            mk.set(m, img=i)
    return mk


def _to_img_row(idx):
    fr = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    img = np.where(idx >= 0, np.searchsorted(fr, idx, side="right") - 1, -1).astype(np.int32)
    return img, np.where(idx >= 0, idx - fr[np.maximum(img, 0)], -1).astype(np.int32)


@pytest.mark.parametrize("kind", KINDS)
def test_collections_equal_the_stacked_pair_form(ctx, kind):
    rng = np.random.default_rng(77)
    nq = 33
    images = [_rows(rng, n, kind) for n in SIZES]
    Q = _rows(rng, nq, kind)
    masks = _coll_masks(rng, nq)
    dense = np.concatenate([np.ones((nq, n), np.uint8) if m is None else m for m, n in zip(masks, SIZES)], axis=1)
    T = np.concatenate(images)
    qb, tb = _bank(ctx, Q, kind), _bank(ctx, T, kind)
    if kind == "f32":
        qb.close()
        qb = ctx.bank(Q, float_route=True)
    c = _coll(ctx, images, kind)
    with c.mask(nq) as mk, c.mask(nq) as ones:
        assert mk.info()[:3] == (nq, sum(SIZES), len(SIZES))
        _fill(mk, masks)
        for i in range(len(SIZES)):
            ones.set_all(True, img=i)
        for k in (1, 2, 3, 8):
            img, idx, dist = c.knn_masked(qb, mk, k)
            pi, pd = _masked(ctx, qb, tb, dense, k)
            wi, wr = _to_img_row(pi)
            _same((img, idx, dist), (wi, wr, pd), (kind, k))
            assert not (img == 4).any()
            _same(c.knn_masked(qb, ones, k), c.knn(qb, k), (kind, k, "all ones"))
        # setting one image again touches no other image's words
        mk.set_all(False, img=0)
        mk.set(masks[0], img=0)
        _same(c.knn_masked(qb, mk, 2)[1:], (_to_img_row(_masked(ctx, qb, tb, dense, 2)[0])[1], _masked(ctx, qb, tb, dense, 2)[1]), "reset")
        c.add_binary(images[3]) if kind == "bin" else c.add(images[3])
        with pytest.raises(fastmatch_amd.FastMatchHipError, match="changed") as e:
            c.knn_masked(qb, mk, 2)
        assert e.value.code == FM_EINVAL
    c.close(), qb.close(), tb.close()


# 8 ---------------------------------------------------------------------------------------------------------------------
def test_device_forms_and_torchmatch(ctx):
    import torch
    from fastmatch_amd import torchmatch
    rng = np.random.default_rng(88)
    nq, nt = 130, 1000
    dev = torch.device("cuda", ctx.device)
    for kind in ("u8", "f32"):
        Q, T = _rows(rng, nq, kind), _rows(rng, nt, kind)
        m = (rng.random((nq, nt)) < 0.2).astype(np.uint8)
        wide = np.zeros((nq, nt + 77), np.uint8)
        wide[:, 40:40 + nt] = m
        wide[:, :40] = 1
        wide[:, 40 + nt:] = 1
        qb, tb = ctx.bank(Q), ctx.bank(T)
        tq, tt = torch.from_numpy(Q).to(dev), torch.from_numpy(T).to(dev)
        tensors = {"uint8 dense": torch.from_numpy(m).to(dev), "bool dense": torch.from_numpy(m.astype(bool)).to(dev),
                   "uint8 slice": torch.from_numpy(wide).to(dev)[:, 40:40 + nt],
                   "bool slice": torch.from_numpy(wide.astype(bool)).to(dev)[:, 40:40 + nt]}
        for k in ((1, 2, 5) if kind == "u8" else (2,)):
            want = _masked(ctx, qb, tb, m, k)
            for what, tm in tensors.items():
                # the raw device form: the mask from device memory, the lists into device tensors
                with ctx.mask(nq, nt) as mk:
                    mk.set_dev(tm.data_ptr(), pitch=tm.stride(0), stream=torch.cuda.current_stream().cuda_stream)
                    d_idx = torch.full((nq, k), 7, dtype=torch.int32, device=dev)
                    d_dist = torch.zeros((nq, k), dtype=torch.float32, device=dev)
                    ctx.knn_masked_dev(qb, tb, mk, k, d_idx.data_ptr(), d_dist.data_ptr(),
                                       consumer_stream=torch.cuda.current_stream().cuda_stream)
                    _same((d_idx.cpu().numpy(), d_dist.cpu().numpy()), want, (kind, k, what, "dev"))
                ti, td = torchmatch.knn(tq, tt, k, mask=tm)
                _same((ti.cpu().numpy(), td.cpu().numpy()), want, (kind, k, what, "torchmatch"))
        _same([x.cpu().numpy() for x in torchmatch.knn(tq, tt, 2)], ctx.knn(qb, tb, 2), "no mask")
        with pytest.raises(ValueError):
            torchmatch.knn(tq, tt, 2, mask=torch.from_numpy(m))                 # a CPU tensor
        with pytest.raises(ValueError):
            torchmatch.knn(tq, tt, 2, mask=tensors["uint8 dense"][:, :-1])      # the wrong shape
        qb.close(), tb.close()
    # collections
    images = [_rows(rng, n, "u8") for n in SIZES]
    Q = _rows(rng, 33, "u8")
    masks = _coll_masks(rng, 33)
    c = _coll(ctx, images, "u8")
    qb = ctx.bank(Q)
    with c.mask(33) as mk:
        _fill(mk, masks)
        with torchmatch.Collection(context=ctx) as tc:
            for im in images:
                tc.add(torch.from_numpy(im).to(dev))
            wide = [None if m is None else torch.from_numpy(np.concatenate([m, m], axis=1).astype(bool)).to(dev)[:, :m.shape[1]] for m in masks]
            for k in (1, 2, 4):
                want = c.knn_masked(qb, mk, k)
                d = [torch.empty((33, k), dtype=dt, device=dev) for dt in (torch.int32, torch.int32, torch.float32)]
                c.knn_masked_dev(qb, mk, k, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(),
                                 consumer_stream=torch.cuda.current_stream().cuda_stream)
                _same([x.cpu().numpy() for x in d], want, (k, "coll dev"))
                got = tc.knn(torch.from_numpy(Q).to(dev), k, masks=wide)
                _same([x.cpu().numpy() for x in got], want, (k, "torchmatch coll"))
            _same([x.cpu().numpy() for x in tc.knn(torch.from_numpy(Q).to(dev), 2)], c.knn(qb, 2), "coll no mask")
    c.close(), qb.close()


# 9 ---------------------------------------------------------------------------------------------------------------------
def _dm(lists):
    return [[(m.queryIdx, m.trainIdx, m.imgIdx, np.float32(m.distance).view(np.uint32)) for m in row] for row in lists]


def test_python_surface(ctx):
    rng = np.random.default_rng(99)
    nq, nt = 40, 300
    Q, T = _rows(rng, nq, "u8"), _rows(rng, nt, "u8")
    m = (rng.random((nq, nt)) < 0.05).astype(np.uint8)
    m[3] = 0
    opts = {"context": ctx, "mask": m}
    for k in (1, 2, 3):
        idx, dist = matchutil.bf_match_arrays(Q, T, k=k, options=opts)
        _same((idx, dist), R.knn_u8(Q, T, m, k), k)
        want = _dm(matchutil.matches_from_arrays(idx, dist))
        assert _dm(matchutil.bf_match(Q, T, k=k, options=opts)) == want
        assert _dm(matchutil.flann_match(Q, T, k=k, options=dict(opts, crossCheck=True))) == want
        assert _dm(matchutil.BFMatcher(options={"context": ctx}).knnMatch(Q, T, k=k, mask=m.astype(bool))) == want
        assert want[3] == []
        _same(matchutil.flann_match_arrays(Q, T, k=k, options=opts), (idx, dist), k)
    with ctx.mask(nq, nt) as mk:
        _same(matchutil.bf_match_arrays(Q, T, k=2, options={"context": ctx, "mask": mk.set(m)}), R.knn_u8(Q, T, m, 2), "resident")
    # without a mask: what the calls return on the parent commit's path
    qb, tb = ctx.bank(Q), ctx.bank(T)
    _same(matchutil.bf_match_arrays(Q, T, k=2, options={"context": ctx}), ctx.knn2(qb, tb), "no mask")
    qb.close(), tb.close()
    # a train collection and cv2's masks
    images = [_rows(rng, n, "u8") for n in SIZES]
    masks = _coll_masks(rng, nq)
    bf = matchutil.BFMatcher(options={"context": ctx})
    bf.add(images)
    for k in (1, 2, 3):
        img, idx, dist = bf.knnMatch_arrays(Q, k, masks=masks)
        want = [[(qi, int(idx[qi, j]), int(img[qi, j]), np.float32(dist[qi, j]).view(np.uint32)) for j in range(k) if idx[qi, j] >= 0]
                for qi in range(nq)]
        assert _dm(bf.knnMatch(Q, k=k, masks=masks)) == want
        dense = np.concatenate([np.ones((nq, n), np.uint8) if mm is None else mm for mm, n in zip(masks, SIZES)], axis=1)
        pi, pd = R.knn_u8(Q, np.concatenate(images), dense, k)
        _same((img, idx, dist), _to_img_row(pi) + (pd,), ("BFMatcher", k))
    assert _dm([[x] for x in bf.match(Q, masks=masks)]) == [r[:1] for r in _dm(bf.knnMatch(Q, k=1, masks=masks)) if r]
    plain = bf.knnMatch_arrays(Q, 2)
    _same(plain, bf._coll.knn(ctx.bank(Q), 2), "collection, no mask")
    assert _dm(bf.knnMatch(Q, 2)) == _dm(bf.knnMatch(Q, k=2, masks=[None] * len(SIZES)))


# 10 --------------------------------------------------------------------------------------------------------------------
def _code(ctx, call):
    with pytest.raises(fastmatch_amd.FastMatchHipError) as e:
        call()
    return e.value.code, str(e.value)


def test_errors_in_the_documented_order(ctx):
    import torch
    rng = np.random.default_rng(10)
    Q, T = _rows(rng, 9, "u8"), _rows(rng, 70, "u8")
    qb, tb = ctx.bank(Q), ctx.bank(T)
    narrow, q32 = ctx.bank(T[:, :64]), ctx.bank(Q[:, :32])          # (q32: as wide as the binary bank's 32 bytes)
    binb = ctx.bank_binary(_rows(rng, 70, "bin"))
    lib, h = ctx.lib, ctx.handle
    idx, dist = np.empty((9, 9), np.int32), np.empty((9, 9), np.float32)
    ip, dp = idx.ctypes.data, dist.ctypes.data
    with ctx.mask(9, 70) as mk, ctx.mask(8, 70) as short, ctx.mask(9, 71) as wide_t:
        # 1. NULL handles, before anything else (here: together with a bad k and a bad mask geometry)
        assert lib.fm_knn_masked(None, qb.handle, tb.handle, mk.handle, 99, ip, dp) == FM_EINVAL
        assert lib.fm_knn_masked(h, None, tb.handle, short.handle, 99, ip, dp) == FM_EINVAL
        assert lib.fm_knn_masked(h, qb.handle, None, short.handle, 99, ip, dp) == FM_EINVAL
        assert lib.fm_knn_masked(h, qb.handle, tb.handle, None, 99, ip, dp) == FM_EINVAL
        assert b"mask is NULL" in lib.fm_last_error(h)
        # 2. check_pair's rules before k
        assert lib.fm_knn_masked(h, qb.handle, narrow.handle, short.handle, 99, ip, dp) == FM_EINVAL
        assert b"dim mismatch" in lib.fm_last_error(h)
        assert lib.fm_knn_masked(h, q32.handle, binb.handle, short.handle, 99, ip, dp) == FM_EINVAL
        assert b"kind mismatch" in lib.fm_last_error(h)
        # 3. k before the mask's geometry
        assert lib.fm_knn_masked(h, qb.handle, tb.handle, short.handle, 0, ip, dp) == FM_EINVAL
        assert lib.fm_knn_masked(h, qb.handle, tb.handle, short.handle, 9, ip, dp) == FM_EUNSUPPORTED
        # 4. the mask's geometry before the output pointers
        assert lib.fm_knn_masked(h, qb.handle, tb.handle, short.handle, 2, None, None) == FM_EINVAL
        assert b"8 query rows" in lib.fm_last_error(h)                      # nq off by one
        assert lib.fm_knn_masked(h, qb.handle, tb.handle, wide_t.handle, 2, None, None) == FM_EINVAL
        assert b"71 train rows" in lib.fm_last_error(h)
        # 5. the output pointers
        assert lib.fm_knn_masked(h, qb.handle, tb.handle, mk.handle, 2, None, dp) == FM_EINVAL
        assert b"output pointer" in lib.fm_last_error(h)
        # the device form: the same order, then fm_knn_dev's pointer checks (host memory is refused)
        ns = _ffi._stream_arg(None)
        assert lib.fm_knn_masked_dev(h, qb.handle, tb.handle, short.handle, 9, ip, dp, ns) == FM_EUNSUPPORTED
        assert lib.fm_knn_masked_dev(h, qb.handle, tb.handle, short.handle, 2, ip, dp, ns) == FM_EINVAL
        assert b"8 query rows" in lib.fm_last_error(h)
        assert lib.fm_knn_masked_dev(h, qb.handle, tb.handle, mk.handle, 2, ip, dp, ns) == FM_EINVAL
        assert b"device memory" in lib.fm_last_error(h)
        # fm_mask_set_*: image index, pitch, NULL source, host memory handed to the device form
        m = np.ones((9, 70), np.uint8)
        assert lib.fm_mask_set_u8(h, mk.handle, 1, m.ctypes.data, 0) == FM_EINVAL
        assert lib.fm_mask_set_u8(h, mk.handle, -1, m.ctypes.data, 0) == FM_EINVAL
        assert lib.fm_mask_set_u8(h, mk.handle, 0, m.ctypes.data, 69) == FM_EINVAL
        assert lib.fm_mask_set_u8(h, mk.handle, 0, None, 0) == FM_EINVAL
        assert lib.fm_mask_set_all(h, mk.handle, 1, 1) == FM_EINVAL
        assert lib.fm_mask_set_dev(h, mk.handle, 0, m.ctypes.data, 0, ns) == FM_EINVAL
        assert b"device memory" in lib.fm_last_error(h)
        assert lib.fm_mask_set_dev(h, mk.handle, 0, None, 0, ns) == FM_EINVAL
        # a collection: a pair mask is refused there, a collection's mask by the pair form
        c = ctx.collection()
        c.add(T)
        with c.mask(9) as cm:
            code, msg = _code(ctx, lambda: c.knn_masked(qb, mk, 2))
            assert code == FM_EINVAL and "bank pair" in msg
            code, msg = _code(ctx, lambda: ctx.knn_masked(qb, tb, cm, 2))
            assert code == FM_EINVAL and "collection" in msg
            assert _code(ctx, lambda: c.knn_masked(qb, cm, 0))[0] == FM_EINVAL
            assert _code(ctx, lambda: c.knn_masked(qb, cm, 9))[0] == FM_EUNSUPPORTED
            assert lib.fm_collection_knn_masked(h, c.handle, qb.handle, None, 2, ip, ip, dp) == FM_EINVAL
            assert lib.fm_collection_knn_masked(h, c.handle, qb.handle, cm.handle, 2, None, ip, dp) == FM_EINVAL
            assert lib.fm_mask_set_u8(h, cm.handle, 1, m.ctypes.data, 0) == FM_EINVAL
            c.clear()
            c.add(T)
            code, msg = _code(ctx, lambda: c.knn_masked(qb, cm, 2))
            assert code == FM_EINVAL and "changed" in msg
        with c.mask(8) as cs:
            code, msg = _code(ctx, lambda: c.knn_masked(qb, cs, 2))
            assert code == FM_EINVAL and "8 query rows" in msg
        c.close()
    # empty operands are valid
    eq, et = ctx.bank(np.zeros((0, 128), np.uint8)), ctx.bank(np.zeros((0, 128), np.uint8))
    with ctx.mask(0, 70) as m0, ctx.mask(9, 0) as m1:
        assert ctx.knn_masked(eq, tb, m0.set(np.zeros((0, 70), np.uint8)), 2)[0].shape == (0, 2)
        i1, d1 = ctx.knn_masked(qb, et, m1.set(np.zeros((9, 0), np.uint8)).set_all(True), 3)
        assert (i1 == -1).all() and np.isinf(d1).all()
    dev_out = torch.empty((9, 2), dtype=torch.int32, device=torch.device("cuda", ctx.device))
    assert dev_out.is_cuda
    for b in (qb, tb, narrow, q32, binb, eq, et):
        b.close()
