"""GPU: the match graph of a WIDE collection (fm_collection_add_wide / _add_wide_dev, then fm_collection_pairs_mutual_ratio and
its device form on images of 129 .. 256 float values per row).  Pair (a, b) equals Context.mutual_ratio on wide banks made
from the same arrays AND the NumPy reference (tests/wide_pairs_ref.py: the oracle's order-1 chain), bit for bit -- no
tolerance anywhere."""
import ctypes
import os
import sys

import numpy as np
import pytest

from fastmatch_amd import _ffi, matchutil

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wide_pairs_ref as ref                    # noqa: E402
import wide_ref                                 # noqa: E402

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -4
INF = float("inf")
SIZES = [0, 1, 127, 128, 129, 1000, 5, 0]
LISTED = [(5, 5), (2, 3), (3, 2), (2, 3), (0, 7), (7, 0), (1, 1)]
_MEMO = {}                                      # dim -> (images, the reference's memo): computed once, never changed


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want, what):
    assert np.array_equal(got[0], want[0]), what + ": rows of a"
    assert np.array_equal(got[1], want[1]), what + ": rows of b"
    assert np.array_equal(_bits(got[2]), _bits(want[2])), what + ": distances"
    assert np.array_equal(np.asarray(got[3]).view(np.uint64), np.asarray(want[3]).view(np.uint64)), what + ": ratios"


def _data(dim):
    if dim not in _MEMO:
        _MEMO[dim] = (ref.images(SIZES, dim, 7100 + dim, big=5), {})
    return _MEMO[dim]


def _collection(ctx, images):
    c = ctx.collection()
    for i, im in enumerate(images):
        assert c.add_wide(im) == i
    return c


def _loop(ctx, banks, pairs, tau, sym):
    return [ctx.mutual_ratio(banks[a], banks[b], tau, sym) for a, b in pairs]


@pytest.mark.parametrize("dim", [129, 161, 200, 256])
def test_every_pair_equals_the_pair_call_and_the_reference(ctx, dim):
    images, memo = _data(dim)
    coll = _collection(ctx, images)
    banks = [ctx.bank(im) for im in images]
    old = ctx.get_option("f32_filter")
    try:
        assert coll.info() == (8, sum(SIZES), dim, _ffi.FM_BANK_F32W)
        assert coll.image_rows().tolist() == SIZES
        assert all(b.kind == _ffi.FM_BANK_F32W for b in banks)
        accepted = 0
        for pairs in (None, LISTED):
            plist = ref.all_pairs(len(images)) if pairs is None else pairs
            assert len(plist) == (28 if pairs is None else 7)
            for tau in (0.8, INF):
                for sym in (False, True):
                    ctx.set_option("f32_filter", old)
                    loop = _loop(ctx, banks, plist, tau, sym)
                    want = ref.pairs_mutual_ratio(images, plist, tau, sym, memo=memo)
                    for mode in (0, 2):
                        ctx.set_option("f32_filter", mode)
                        l0, f0 = ctx.f32_filter_stats()
                        got = coll.pairs_mutual_ratio(pairs, tau, sym)
                        l1, f1 = ctx.f32_filter_stats()
                        if mode == 2:
                            assert l1 > l0 and f1 == f0, (l1 - l0, f1 - f0)       # the filter answers every chunk itself
                        else:
                            assert l1 == l0                                        # the exact kernel alone
                        assert len(got) == len(plist)
                        for p, ab in enumerate(plist):
                            what = "dim %d filter %d tau=%s sym=%d pair %s" % (dim, mode, tau, sym, ab)
                            _same(got[p], loop[p], what + " against the pair call")
                            _same(got[p], want[p], what + " against the reference")
                            if min(images[ab[0]].shape[0], images[ab[1]].shape[0]) == 0:
                                assert got[p][0].shape[0] == 0
                        counts = coll.pairs_mutual_ratio_counts(pairs, tau, sym)
                        assert np.diff(counts).tolist() == [g[0].shape[0] for g in got] and counts[0] == 0
                        if pairs is LISTED:
                            _same(got[1], got[3], "a pair listed twice")
                            assert got[0][0].tolist() == got[0][1].tolist() == list(range(1000))      # (5, 5): every row is its own
                        accepted += sum(g[0].shape[0] for g in got)
        ctx.set_option("f32_filter", 2)
        assert coll.pairs_mutual_ratio([(4, 5)], 0.8, True)[0][0].shape[0] >= 10          # the planted views are found
        assert accepted > 0
    finally:
        ctx.set_option("f32_filter", old)
        for b in banks:
            b.close()
        coll.close()


def test_more_than_1024_slots(ctx):
    """48 images of 1 .. 40 rows, exhaustive: 1 128 pairs, 2 256 slots in one chunk -- the search over the prefix arrays has
    depth -- against the reference, through the filter and through the exact kernel."""
    sizes = [1 + (i * 7) % 40 for i in range(48)]
    assert sorted(set(sizes)) == list(range(1, 41))
    rng = np.random.default_rng(7300)
    base = ref.images([40], 129, 7301)[0]
    images = [ref.unit(base[rng.permutation(40)[:n]].astype(np.float64) + 0.02 / np.sqrt(129) * rng.standard_normal((n, 129)))
              for n in sizes]
    coll = _collection(ctx, images)
    old = ctx.get_option("f32_filter")
    try:
        want = ref.pairs_mutual_ratio(images, None, 0.8, True)
        assert len(want) == 1128 and sum(w[0].shape[0] for w in want) >= 1128
        for mode in (2, 0):
            ctx.set_option("f32_filter", mode)
            l0, f0 = ctx.f32_filter_stats()
            counts = coll.pairs_mutual_ratio_counts(None, 0.8, True)               # (one C call; pairs_mutual_ratio makes two)
            l1, f1 = ctx.f32_filter_stats()
            assert (l1 - l0, f1 - f0) == ((1, 0) if mode == 2 else (0, 0))           # ONE launch for the one chunk
            got = coll.pairs_mutual_ratio(None, 0.8, True)
            assert np.diff(counts).tolist() == [g[0].shape[0] for g in got]
            for p, ab in enumerate(ref.all_pairs(48)):
                _same(got[p], want[p], "filter %d pair %s" % (mode, ab))
    finally:
        ctx.set_option("f32_filter", old)
        coll.close()


def test_chunks_do_not_change_the_result(ctx):
    images, _ = _data(161)
    coll = _collection(ctx, images)
    old = ctx.get_option("f32_filter")
    before = ctx.get_option("coll_ws_bytes")
    try:
        ctx.set_option("f32_filter", 2)
        want_all, off_all = coll.pairs_mutual_ratio(None, INF, True), coll.pairs_mutual_ratio_counts(None, INF, True)
        want_l, off_l = coll.pairs_mutual_ratio(LISTED, 0.8, False), coll.pairs_mutual_ratio_counts(LISTED, 0.8, False)
        assert off_all[-1] > 0 and off_l[-1] > 0
        for budget in (1, 4 << 20):                    # one pair per chunk; a middle value: several small pairs per chunk
            ctx.set_option("coll_ws_bytes", budget)
            for pairs, want, off in ((None, want_all, off_all), (LISTED, want_l, off_l)):
                tau, sym = (INF, True) if pairs is None else (0.8, False)
                l0 = ctx.f32_filter_stats()[0]
                assert np.array_equal(coll.pairs_mutual_ratio_counts(pairs, tau, sym), off)      # (one C call)
                chunks = ctx.f32_filter_stats()[0] - l0
                got = coll.pairs_mutual_ratio(pairs, tau, sym)
                if budget == 1:                        # a chunk per pair of two non-empty images
                    plist = ref.all_pairs(8) if pairs is None else pairs
                    assert chunks == sum(1 for a, b in plist if SIZES[a] and SIZES[b])
                else:
                    assert 1 < chunks < 15
                for p in range(len(want)):
                    _same(got[p], want[p], "budget %d pair %d" % (budget, p))
    finally:
        ctx.set_option("coll_ws_bytes", before)
        ctx.set_option("f32_filter", old)
        coll.close()


def test_growth_and_rescale(ctx):
    """Small images at magnitudes ~1e-3 fix the scale; a 4099-row image at ~1e3 outgrows the first allocation (doubling, device
    copies) and lifts the maximum out of the scale's range (the fp16 planes of every image are rewritten on the device)."""
    rng = np.random.default_rng(7400)
    small = [(1e-3 * rng.standard_normal((n, 200))).astype(np.float32) for n in (100, 200, 300)]
    big = (1e3 * rng.standard_normal((4099, 200))).astype(np.float32)
    big[::5][:300] = 1e6 * small[2]                     # shared content across the scales
    images = small + [big]
    grown = _collection(ctx, images)
    fresh = _collection(ctx, [big] + small)             # the large image first: the scale is right from the start
    perm = [1, 2, 3, 0]
    banks = [ctx.bank(im) for im in images]
    old = ctx.get_option("f32_filter")
    try:
        ctx.set_option("f32_filter", 2)
        plist = ref.all_pairs(4) + [(3, 2), (0, 0)]
        l0 = ctx.f32_filter_stats()[0]
        grown.pairs_mutual_ratio_counts(plist, INF, True)
        assert ctx.f32_filter_stats()[0] == l0 + 1      # the filter still launches: one chunk, one launch
        got = grown.pairs_mutual_ratio(plist, INF, True)
        other = fresh.pairs_mutual_ratio([(perm[a], perm[b]) for a, b in plist], INF, True)
        loop = _loop(ctx, banks, plist, INF, True)
        want = ref.pairs_mutual_ratio(images, plist, INF, True)
        for p, ab in enumerate(plist):
            _same(got[p], other[p], "pair %s against a fresh collection" % (ab,))
            _same(got[p], loop[p], "pair %s against the pair call" % (ab,))
            _same(got[p], want[p], "pair %s against the reference" % (ab,))
        assert sum(g[0].shape[0] for g in got) > 0
    finally:
        ctx.set_option("f32_filter", old)
        for b in banks:
            b.close()
        grown.close()
        fresh.close()


def test_values_that_are_not_finite(ctx):
    Q, T = wide_ref.nonfinite(300, 257, 192, 7500)
    images = [Q, T, wide_ref.gaussian(100, 1, 192, 7501)[0]]
    coll = _collection(ctx, images)
    old = ctx.get_option("f32_filter")
    try:
        ctx.set_option("f32_filter", 2)
        plist = ref.all_pairs(3) + [(1, 0), (0, 0)]
        l0, f0 = ctx.f32_filter_stats()
        got = coll.pairs_mutual_ratio(plist, INF, True)
        assert ctx.f32_filter_stats() == (l0, f0)       # the exact kernel alone, for the whole collection
        want = ref.pairs_mutual_ratio(images, plist, INF, True)
        for p, ab in enumerate(plist):
            _same(got[p], want[p], "pair %s" % (ab,))
        assert sum(g[0].shape[0] for g in got) > 0
    finally:
        ctx.set_option("f32_filter", old)
        coll.close()


def test_the_list_overflow_redoes_the_chunk(ctx):
    """One cluster of exact copies: 2100 identical rows are all inside every row's margin, 600 rows next to them make 1.26M
    records in the forward slot alone against the chunk's 2^20; the exact kernel redoes the chunk and the fallback is counted
    once."""
    rng = np.random.default_rng(11)
    T = np.repeat(rng.standard_normal((1, 192)).astype(np.float32), 2100, axis=0)
    Q = (T[:600] + 1e-3 * rng.standard_normal((600, 192))).astype(np.float32)
    coll = _collection(ctx, [Q, T])
    qb, tb = ctx.bank(Q), ctx.bank(T)
    old = ctx.get_option("f32_filter")
    try:
        ctx.set_option("f32_filter", 2)
        l0, f0 = ctx.f32_filter_stats()
        counts = coll.pairs_mutual_ratio_counts([(0, 1)], INF, True)
        l1, f1 = ctx.f32_filter_stats()
        assert (l1 - l0, f1 - f0) == (1, 1)
        got = coll.pairs_mutual_ratio([(0, 1)], INF, True)
        assert counts.tolist() == [0, got[0][0].shape[0]]
        _same(got[0], ctx.mutual_ratio(qb, tb, INF, True), "against the pair call")
    finally:
        ctx.set_option("f32_filter", old)
        qb.close(); tb.close()
        coll.close()


def test_host_and_device_adds_build_the_same_collection(ctx):
    import torch
    images, _ = _data(200)
    images = [images[i] for i in (4, 0, 5, 2)]          # 129, 0, 1000, 127 rows
    stream = torch.cuda.current_stream().cuda_stream

    def dev_add(c, t):
        n, dim = t.shape
        dt = {torch.float32: _ffi.FM_DT_F32, torch.float16: _ffi.FM_DT_F16, torch.bfloat16: _ffi.FM_DT_BF16}[t.dtype]
        return c.add_wide_from_device(t.data_ptr() if n else 0, dt, n, dim, t.stride(0) * t.element_size(), stream=stream)

    def pitched(im):                                    # a column slice of a wider tensor
        wide = torch.full((im.shape[0], 300), 7.0, device="cuda")
        wide[:, 36:236] = torch.from_numpy(im).cuda()
        return wide[:, 36:236]

    def results(c):
        return c.info(), c.image_rows().tolist(), c.pairs_mutual_ratio(None, 0.8, True) + c.pairs_mutual_ratio([(2, 2), (3, 0)], INF, False)

    def check(a, b, what):
        assert a[0] == b[0] and a[1] == b[1], what
        for p in range(len(a[2])):
            _same(a[2][p], b[2][p], "%s pair %d" % (what, p))
    made = []
    old = ctx.get_option("f32_filter")
    try:
        ctx.set_option("f32_filter", 2)
        host = _collection(ctx, images); made.append(host)
        want = results(host)
        assert sum(w[0].shape[0] for w in want[2]) > 0
        dev = ctx.collection(); made.append(dev)
        keep = [pitched(im) for im in images]
        assert keep[0].stride(0) == 300
        for i, t in enumerate(keep):
            assert dev_add(dev, t) == i
        check(results(dev), want, "device adds of pitched float32 slices")
        mixed = ctx.collection(); made.append(mixed)
        for i, (im, t) in enumerate(zip(images, keep)):
            assert (mixed.add_wide(im) if i % 2 else dev_add(mixed, t)) == i
        check(results(mixed), want, "alternating host and device adds")
        for dt in (torch.float16, torch.bfloat16):
            src = [torch.from_numpy(im).cuda().to(dt) for im in images]
            widened = [t.float().cpu().numpy() for t in src]
            h = _collection(ctx, widened); made.append(h)
            d = ctx.collection(); made.append(d)
            for i, t in enumerate(src):
                assert dev_add(d, t) == i
            check(results(d), results(h), "%s source against the host add of its widened values" % dt)
    finally:
        ctx.set_option("f32_filter", old)
        for c in made:
            c.close()


def test_device_form_and_torchmatch(ctx):
    import torch
    from fastmatch_amd import torchmatch
    images, _ = _data(256)
    coll = _collection(ctx, images)
    try:
        for pairs, tau, sym in ((None, 0.8, True), (LISTED, INF, False)):
            want = coll.pairs_mutual_ratio(pairs, tau, sym)
            offsets = coll.pairs_mutual_ratio_counts(pairs, tau, sym)
            total, n = int(offsets[-1]), len(want)
            mid = int(offsets[n // 2 + 1]) - 1
            for cap in (total + 3, max(mid, 0), 0):
                rows = torch.full((cap, 3), -7, dtype=torch.int32, device="cuda")
                d_off = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
                got_total = coll.pairs_mutual_ratio_dev(pairs, tau, sym, d_off.data_ptr(), rows.data_ptr() if cap else 0, cap, want_total=True,
                                                        consumer_stream=torch.cuda.current_stream().cuda_stream)
                h_off, got = d_off.cpu().numpy(), rows.cpu().numpy()
                assert got_total == total and h_off.tolist() == offsets.tolist()
                whole = ref.pack(want, cap)[1]
                at = 0
                for p in range(n):
                    k = want[p][0].shape[0]
                    if at + k > whole:
                        break
                    assert np.array_equal(got[at:at + k, 0], want[p][0]) and np.array_equal(got[at:at + k, 1], want[p][1])
                    assert np.array_equal(got[at:at + k, 2].view(np.uint32), _bits(want[p][2]))
                    at += k
                assert at == whole and (got[whole:] == -7).all()          # the longest prefix of WHOLE pairs
        # torchmatch: images from tensors, a counts-then-fill call and a capped one
        with torchmatch.Collection(context=ctx) as tc:
            for i, im in enumerate(images):
                assert tc.add_wide(torch.from_numpy(im).cuda()) == i
            assert tc.info() == coll.info()
            packed = ref.pack(coll.pairs_mutual_ratio(LISTED, 0.8, True), 1 << 40)
            for cap in (None, packed[1] + 4):
                offsets, rows = tc.match_pairs(LISTED, 0.8, symmetric=True, cap=cap)
                assert offsets.cpu().numpy().tolist() == packed[0].tolist()
                got = rows.cpu().numpy()[:packed[1]]
                assert np.array_equal(got[:, 0], packed[2][0]) and np.array_equal(got[:, 1], packed[2][1])
                assert np.array_equal(got[:, 2].view(np.uint32), _bits(packed[2][2]))
            x = torch.from_numpy(images[2]).cuda()
            with pytest.raises(ValueError, match="wide"):
                tc.knn(x, 2)
            with pytest.raises(ValueError, match="wide"):
                tc.add(x[:, :128].contiguous())
            tc.clear()
            assert tc.add(x[:, :128].contiguous()) == 0           # clear resets the kind
        # matchutil: BFMatcher.add_wide, matchPairs
        m = matchutil.BFMatcher()
        m.add_wide(images)
        arr, lists = m.matchPairs_arrays(LISTED, 0.8, True)
        want = coll.pairs_mutual_ratio(LISTED, 0.8, True)
        for p in range(len(LISTED)):
            _same(lists[p], want[p], "BFMatcher pair %d" % p)
        assert sum(len(v) for v in m.matchPairs().values()) == int(coll.pairs_mutual_ratio_counts(None, 0.8, False)[-1])
    finally:
        coll.close()


def test_stats_account_two_sweeps_per_pair(ctx):
    images, _ = _data(129)
    coll = _collection(ctx, images)
    try:
        ctx.sync()
        before = ctx.stats()
        coll.pairs_mutual_ratio_counts([(2, 3), (5, 4), (0, 5)], 0.8)          # (one C call)
        assert ctx.stats()["pairs"] - before["pairs"] == 2 * (127 * 128 + 1000 * 129)
    finally:
        coll.close()


def test_refusals(ctx):
    rng = np.random.default_rng(7600)
    w = rng.standard_normal((50, 256)).astype(np.float32)
    narrow = rng.standard_normal((50, 128)).astype(np.float32)
    lib, h = ctx.lib, ctx.handle
    P = _ffi._ptr
    NOS = _ffi._stream_arg(None)
    i = ctypes.c_int32(-7)

    def err():
        return lib.fm_last_error(h).decode()
    coll, other = ctx.collection(), ctx.collection()
    q = ctx.bank(narrow, float_route=True)
    try:
        add, add_dev = lib.fm_collection_add_wide, lib.fm_collection_add_wide_dev
        # the width, on a collection that stays empty and without a kind
        assert add(h, coll.handle, P(narrow), 50, 128, ctypes.byref(i)) == EINVAL and "fm_collection_add_f32" in err()
        assert add(h, coll.handle, P(w), 50, 257, ctypes.byref(i)) == EUNSUPPORTED
        assert add(None, coll.handle, P(w), 50, 256, ctypes.byref(i)) == EINVAL
        assert add(h, None, P(w), 50, 256, ctypes.byref(i)) == EINVAL
        assert add(h, coll.handle, None, 50, 256, ctypes.byref(i)) == EINVAL
        for dt in (_ffi.FM_DT_U8, _ffi.FM_DT_BIN, 99):
            assert add_dev(h, coll.handle, None, dt, 0, 256, 0, NOS, ctypes.byref(i)) == EINVAL and "dtype" in err()
        assert add_dev(h, coll.handle, None, _ffi.FM_DT_F16, 0, 128, 0, NOS, ctypes.byref(i)) == EINVAL
        assert add_dev(h, coll.handle, None, _ffi.FM_DT_F32, 0, 300, 0, NOS, ctypes.byref(i)) == EUNSUPPORTED
        assert add_dev(h, coll.handle, None, _ffi.FM_DT_F32, 5, 256, 0, NOS, ctypes.byref(i)) == EINVAL           # d_rows NULL
        assert add_dev(h, coll.handle, P(w), _ffi.FM_DT_F32, 5, 256, 0, NOS, ctypes.byref(i)) == EINVAL           # host memory
        assert i.value == -7 and coll.info() == (0, 0, 0, 0)
        # the first wide add fixes kind and width, even without rows
        assert coll.add_wide(np.zeros((0, 200), np.float32)) == 0
        assert coll.info() == (1, 0, 200, _ffi.FM_BANK_F32W)
        assert add(h, coll.handle, P(w), 50, 256, ctypes.byref(i)) == EINVAL and "width" in err()
        # mixing, in both directions; the refused collection is unchanged
        for call in (lambda: coll.add(narrow), lambda: coll.add(narrow.astype(np.uint8)), lambda: coll.add_binary(np.zeros((3, 32), np.uint8)),
                     lambda: coll.add(np.zeros((0, 128), np.float32))):
            with pytest.raises(_ffi.FastMatchHipError) as e:
                call()
            assert e.value.code == EINVAL and "wide" in str(e.value)
        with pytest.raises(_ffi.FastMatchHipError) as e:      # the existing adds keep their own refusal of wide rows
            coll.add(w)
        assert e.value.code == EUNSUPPORTED and "wide" in str(e.value)
        assert coll.info() == (1, 0, 200, _ffi.FM_BANK_F32W)
        other.add(np.zeros((0, 128), np.uint8))
        with pytest.raises(_ffi.FastMatchHipError) as e:
            other.add_wide(w)
        assert e.value.code == EINVAL and "mix" in str(e.value) and other.info() == (1, 0, 0, 0)
        coll.add_wide(w[:, :200].copy())
        assert coll.info() == (2, 50, 200, _ffi.FM_BANK_F32W) and coll.image_rows().tolist() == [0, 50]
        coll.train()
        # every call that is not served says so, before it looks at anything else
        wq = ctx.bank(w[:, :200].copy())
        mk = other.mask(4)                                # some mask: the refusal comes before the mask is looked at
        z = np.zeros(4096, np.int64)
        A = [P(z)] * 6
        m = ctypes.c_void_p()
        calls = [
            lambda b: lib.fm_collection_knn(h, coll.handle, b, 1, *A[:3]),
            lambda b: lib.fm_collection_knn_dev(h, coll.handle, b, 1, None, None, None, NOS),
            lambda b: lib.fm_collection_knn2_ratio(h, coll.handle, b, 0.8, 10, *A[:5], None),
            lambda b: lib.fm_collection_knn2_ratio_dev(h, coll.handle, b, 0.8, 10, None, None, None, NOS),
            lambda b: lib.fm_collection_knn2_each(h, coll.handle, b, *A[:2]),
            lambda b: lib.fm_collection_votes(h, coll.handle, b, 0.8, 0, A[0]),
            lambda b: lib.fm_collection_knn_masked(h, coll.handle, b, mk.handle, 1, *A[:3]),       # (a NULL mask counts as a NULL handle)
            lambda b: lib.fm_collection_knn_masked_dev(h, coll.handle, b, mk.handle, 1, None, None, None, NOS),
            lambda b: lib.fm_collection_radius_match(h, coll.handle, b, None, 1.0, 0, A[0], None, None, None, None),
            lambda b: lib.fm_collection_radius_match_dev(h, coll.handle, b, None, 1.0, 0, None, None, None, None, None, NOS),
            lambda b: lib.fm_collection_match_accepted_each(h, coll.handle, b, 0.8, 10, *A[:6]),
            lambda b: lib.fm_collection_match_accepted_each_dev(h, coll.handle, b, 0.8, 10, None, None, None, NOS),
            lambda b: lib.fm_collection_xcheck1_each(h, coll.handle, b, 1.0, *A[:3]),
            lambda b: lib.fm_collection_xcheck1_each_dev(h, coll.handle, b, 1.0, 10, None, None, None, NOS),
            lambda b: lib.fm_collection_mutual_ratio_each(h, coll.handle, b, 0.8, 0, 10, *A[:6]),
            lambda b: lib.fm_collection_mutual_ratio_each_dev(h, coll.handle, b, 0.8, 0, 10, None, None, None, NOS),
        ]
        for n, call in enumerate(calls):
            for b in (q, wq):
                rc = call(b.handle)
                assert rc == EUNSUPPORTED and "wide" in err(), (n, rc, err())
        assert lib.fm_mask_create_coll(h, 4, coll.handle, ctypes.byref(m)) == EUNSUPPORTED and "wide" in err() and not m.value
        wq.close()
        mk.close()
        assert coll.info() == (2, 50, 200, _ffi.FM_BANK_F32W)
        assert coll.pairs_mutual_ratio([(1, 1)], INF)[0][0].tolist() == list(range(50))
        # clear resets kind and width
        coll.clear()
        assert coll.info() == (0, 0, 0, 0)
        assert coll.add(narrow) == 0 and coll.info()[2:] == (128, _ffi.FM_BANK_F32)
        coll.clear()
        assert coll.add_wide(w) == 0 and coll.info() == (1, 50, 256, _ffi.FM_BANK_F32W)
    finally:
        q.close()
        coll.close()
        other.close()
