"""GPU: a wide query bank against every image of a WIDE collection (fm_collection_wide_knn2_each,
fm_collection_wide_mutual_ratio_each and its device form).  Image i equals Context.mutual_ratio / Context.knn2 on wide banks
made from the same arrays AND the NumPy reference (tests/wide_query_ref.py: the oracle's order-1 chain), bit for bit -- no
tolerance anywhere."""
import ctypes
import os
import sys

import numpy as np
import pytest

from fastmatch_amd import _ffi, matchutil

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wide_query_ref as ref                    # noqa: E402
import wide_pairs_ref                           # noqa: E402
import wide_ref                                 # noqa: E402

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -4
INF = float("inf")
SIZES = ref.SIZES
_MEMO = {}                                      # dim -> (images, query, {(tau, sym): reference}): computed once, never changed


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want, what):
    assert np.array_equal(got[0], want[0]), what + ": query rows"
    assert np.array_equal(got[1], want[1]), what + ": rows of the image"
    assert np.array_equal(_bits(got[2]), _bits(want[2])), what + ": distances"
    assert np.array_equal(np.asarray(got[3]).view(np.uint64), np.asarray(want[3]).view(np.uint64)), what + ": ratios"


def _data(dim):
    if dim not in _MEMO:
        images, Q = ref.data(dim)
        _MEMO[dim] = (images, Q, {})
    return _MEMO[dim]


def _want(dim, tau, sym):
    images, Q, memo = _data(dim)
    if (tau, sym) not in memo:
        memo[(tau, sym)] = ref.mutual_ratio_each(Q, images, tau, sym)
    return memo[(tau, sym)]


def _collection(ctx, images):
    c = ctx.collection()
    for i, im in enumerate(images):
        assert c.add_wide(im) == i
    return c


def _check_all(ctx, coll, qb, Q, images, tau, sym, what, banks=None):
    """Every image against the reference (and the loop of pair calls, given the banks); the counts form; the knn2 form."""
    want = ref.mutual_ratio_each(Q, images, tau, sym)
    got = coll.wide_mutual_ratio_each(qb, tau, sym)
    assert len(got) == len(images)
    for i in range(len(images)):
        _same(got[i], want[i], "%s image %d against the reference" % (what, i))
        if banks is not None:
            _same(got[i], ctx.mutual_ratio(qb, banks[i], tau, sym), "%s image %d against the pair call" % (what, i))
    counts = coll.wide_mutual_ratio_each_counts(qb, tau, sym)
    assert counts[0] == 0 and np.diff(counts).tolist() == [g[0].shape[0] for g in got]
    k_idx, k_dist = coll.wide_knn2_each(qb)
    w_idx, w_dist = ref.knn2_each(Q, images)
    assert np.array_equal(k_idx, w_idx) and np.array_equal(_bits(k_dist), _bits(w_dist)), what + ": knn2 against the reference"
    return got


@pytest.mark.parametrize("dim", [129, 161, 200, 256])
def test_every_image_equals_the_pair_call_and_the_reference(ctx, dim):
    images, Q, _ = _data(dim)
    coll = _collection(ctx, images)
    banks = [ctx.bank(im) for im in images]
    qb = ctx.bank(Q)
    old = ctx.get_option("f32_filter")
    try:
        assert coll.info() == (8, sum(SIZES), dim, _ffi.FM_BANK_F32W) and qb.kind == _ffi.FM_BANK_F32W
        ctx.set_option("f32_filter", old)
        k_loop = [ctx.knn2(qb, b) for b in banks]
        k_want = ref.knn2_each(Q, images)
        for tau in (0.8, INF):
            for sym in (False, True):
                ctx.set_option("f32_filter", old)
                loop = [ctx.mutual_ratio(qb, b, tau, sym) for b in banks]
                want = _want(dim, tau, sym)
                # the recipe: the planted views are found in images 2 .. 6, the empty and the one-row image accept nothing
                assert all(want[i][0].shape[0] > 0 for i in range(2, 7)) and all(want[i][0].shape[0] == 0 for i in (0, 1, 7))
                # the copy loses the reverse tie to the lower index (symmetric: the two equal distances make the reverse ratio 1)
                assert 7 not in want[5][0] and (6 in want[5][0]) == (not sym or tau == INF)
                for mode in (0, 2):
                    ctx.set_option("f32_filter", mode)
                    l0, f0 = ctx.f32_filter_stats()
                    got = coll.wide_mutual_ratio_each(qb, tau, sym)
                    l1, f1 = ctx.f32_filter_stats()
                    if mode == 2:
                        assert l1 > l0 and f1 == f0, (l1 - l0, f1 - f0)       # the filter answers every chunk itself
                    else:
                        assert l1 == l0                                        # the exact kernel alone
                    assert len(got) == len(images)
                    for i in range(len(images)):
                        what = "dim %d filter %d tau=%s sym=%d image %d" % (dim, mode, tau, sym, i)
                        _same(got[i], loop[i], what + " against the pair call")
                        _same(got[i], want[i], what + " against the reference")
                    counts = coll.wide_mutual_ratio_each_counts(qb, tau, sym)
                    assert counts[0] == 0 and np.diff(counts).tolist() == [g[0].shape[0] for g in got]
        for mode in (0, 2):
            ctx.set_option("f32_filter", mode)
            l0, f0 = ctx.f32_filter_stats()
            k_idx, k_dist = coll.wide_knn2_each(qb)
            l1, f1 = ctx.f32_filter_stats()
            assert (l1 > l0 and f1 == f0) if mode == 2 else l1 == l0
            assert k_idx.shape == (8, 300, 2)
            assert np.array_equal(k_idx, k_want[0]) and np.array_equal(_bits(k_dist), _bits(k_want[1]))
            for i, (li, ld) in enumerate(k_loop):
                assert np.array_equal(k_idx[i], li) and np.array_equal(_bits(k_dist[i]), _bits(ld)), (mode, i)
    finally:
        ctx.set_option("f32_filter", old)
        qb.close()
        for b in banks:
            b.close()
        coll.close()


def test_two_scales_and_values_that_are_not_finite(ctx):
    dim = 161
    images, Q, _ = _data(dim)
    coll = _collection(ctx, images)
    banks = [ctx.bank(im) for im in images]
    old = ctx.get_option("f32_filter")
    made = []
    try:
        ctx.set_option("f32_filter", 2)
        # one row times 8: the query's scale exponent moves by 3 (cscale = 2^-3 forward, 2^3 reverse), the filter still runs
        Q8 = Q.copy()
        Q8[11] *= 8
        q8 = ctx.bank(Q8); made.append(q8)
        l0, f0 = ctx.f32_filter_stats()
        got = _check_all(ctx, coll, q8, Q8, images, 0.8, True, "one row times 8", banks)
        l1, f1 = ctx.f32_filter_stats()
        assert l1 > l0 and f1 == f0
        assert all(got[i][0].shape[0] > 0 for i in range(2, 7))
        # one row times 1024: the exponents differ by more than 8, no filter is launched and the results stand
        Qk = Q.copy()
        Qk[11] *= 1024
        qk = ctx.bank(Qk); made.append(qk)
        l0, f0 = ctx.f32_filter_stats()
        got = _check_all(ctx, coll, qk, Qk, images, 0.8, True, "one row times 1024", banks)
        assert ctx.f32_filter_stats() == (l0, f0)
        assert all(got[i][0].shape[0] > 0 for i in range(2, 7))
        # one +inf value and one NaN row: the exact route; those rows match nothing, the others are unchanged
        Qn = Q.copy()
        Qn[20, dim // 2] = np.inf
        Qn[33] = np.nan
        qn = ctx.bank(Qn); made.append(qn)
        l0, f0 = ctx.f32_filter_stats()
        got = _check_all(ctx, coll, qn, Qn, images, INF, False, "inf and NaN in the query", banks)
        assert ctx.f32_filter_stats() == (l0, f0)
        clean = _want(dim, INF, False)
        for i in range(len(images)):
            assert 20 not in got[i][0] and 33 not in got[i][0]
            keep = ~np.isin(clean[i][0], (20, 33))
            # (a row that lost the reverse election to 20 or 33 may now win it: the clean rows are a subset)
            assert set(clean[i][0][keep].tolist()) <= set(got[i][0].tolist())
    finally:
        ctx.set_option("f32_filter", old)
        for b in made + banks:
            b.close()
        coll.close()


def test_stack_scale_lifted_after_the_first_call(ctx):
    dim = 200
    images, Q, _ = _data(dim)
    coll = _collection(ctx, images)
    qb = ctx.bank(Q)
    old = ctx.get_option("f32_filter")
    try:
        ctx.set_option("f32_filter", 2)
        first = coll.wide_mutual_ratio_each(qb, 0.8, True)
        for i, w in enumerate(_want(dim, 0.8, True)):
            _same(first[i], w, "before the add, image %d" % i)
        vmax = max(float(np.abs(im).max()) for im in images if im.shape[0])
        extra = images[4].copy()
        extra[3, 5] = 32 * vmax                        # the stack's scale is lifted: every image's fp16 planes are rewritten
        assert coll.add_wide(extra) == 8
        grown = images + [extra]
        l0, f0 = ctx.f32_filter_stats()
        got = _check_all(ctx, coll, qb, Q, grown, 0.8, True, "after the add")
        l1, f1 = ctx.f32_filter_stats()
        assert l1 > l0 and f1 == f0                    # the exponents now differ by 5: still the filter
        assert got[8][0].shape[0] > 0
    finally:
        ctx.set_option("f32_filter", old)
        qb.close()
        coll.close()


def test_many_slots(ctx):
    """600 images of 1 .. 40 rows: 1 200 slots in one chunk -- the search over the prefix arrays has depth -- through the
    filter and through the exact kernel."""
    sizes = [1 + (i * 7) % 40 for i in range(600)]
    rng = np.random.default_rng(9300)
    base = wide_pairs_ref.images([40], 129, 9301)[0]
    images = [wide_pairs_ref.unit(base[rng.permutation(40)[:n]].astype(np.float64) + 0.02 / np.sqrt(129) * rng.standard_normal((n, 129)))
              for n in sizes]
    Q = wide_pairs_ref.unit(base.astype(np.float64) + 0.02 / np.sqrt(129) * rng.standard_normal((40, 129)))
    coll = _collection(ctx, images)
    qb = ctx.bank(Q)
    old = ctx.get_option("f32_filter")
    try:
        want = ref.mutual_ratio_each(Q, images, 0.8, True)
        assert sum(w[0].shape[0] for w in want) >= 600
        for mode in (2, 0):
            ctx.set_option("f32_filter", mode)
            l0, f0 = ctx.f32_filter_stats()
            counts = coll.wide_mutual_ratio_each_counts(qb, 0.8, True)              # (one C call)
            l1, f1 = ctx.f32_filter_stats()
            assert (l1 - l0, f1 - f0) == ((1, 0) if mode == 2 else (0, 0))           # ONE launch for the one chunk
            got = coll.wide_mutual_ratio_each(qb, 0.8, True)
            assert np.diff(counts).tolist() == [g[0].shape[0] for g in got]
            for i in range(600):
                _same(got[i], want[i], "filter %d image %d" % (mode, i))
            k_idx, k_dist = coll.wide_knn2_each(qb)
            w_idx, w_dist = ref.knn2_each(Q, images)
            assert np.array_equal(k_idx, w_idx) and np.array_equal(_bits(k_dist), _bits(w_dist))
    finally:
        ctx.set_option("f32_filter", old)
        qb.close()
        coll.close()


def test_chunks_do_not_change_the_result(ctx):
    dim = 161
    images, Q, _ = _data(dim)
    coll = _collection(ctx, images)
    qb = ctx.bank(Q)
    old = ctx.get_option("f32_filter")
    before = ctx.get_option("coll_ws_bytes")
    try:
        ctx.set_option("f32_filter", 2)
        want, off = coll.wide_mutual_ratio_each(qb, INF, True), coll.wide_mutual_ratio_each_counts(qb, INF, True)
        k_want = coll.wide_knn2_each(qb)
        assert off[-1] > 0
        for budget in (1, 6 << 20):                    # one image per chunk; a middle value: several small images per chunk
            ctx.set_option("coll_ws_bytes", budget)
            l0 = ctx.f32_filter_stats()[0]
            assert np.array_equal(coll.wide_mutual_ratio_each_counts(qb, INF, True), off)      # (one C call)
            chunks = ctx.f32_filter_stats()[0] - l0
            if budget == 1:
                assert chunks == sum(1 for n in SIZES if n)                                    # a chunk per non-empty image
            else:
                assert 1 < chunks < 6
            got = coll.wide_mutual_ratio_each(qb, INF, True)
            for i in range(len(want)):
                _same(got[i], want[i], "budget %d image %d" % (budget, i))
            k_got = coll.wide_knn2_each(qb)
            assert np.array_equal(k_got[0], k_want[0]) and np.array_equal(_bits(k_got[1]), _bits(k_want[1]))
    finally:
        ctx.set_option("coll_ws_bytes", before)
        ctx.set_option("f32_filter", old)
        qb.close()
        coll.close()


def test_the_list_overflow_redoes_the_chunk(ctx):
    """One cluster of exact copies: 2100 identical rows are all inside every row's margin, 600 query rows next to them make
    1.26M records in the forward slot alone against the chunk's 2^20; the exact kernel redoes that chunk and the fallback is
    counted once.  The images of the other chunks are untouched by it."""
    rng = np.random.default_rng(11)
    T = np.repeat(rng.standard_normal((1, 192)).astype(np.float32), 2100, axis=0)
    Q = (T[:600] + 1e-3 * rng.standard_normal((600, 192))).astype(np.float32)
    side = [(T[:50] + 0.5 * rng.standard_normal((50, 192))).astype(np.float32) for _ in range(2)]
    images = [side[0], T, side[1]]
    coll = _collection(ctx, images)
    qb = ctx.bank(Q)
    old = ctx.get_option("f32_filter")
    before = ctx.get_option("coll_ws_bytes")
    try:
        ctx.set_option("f32_filter", 2)
        want = ref.mutual_ratio_each(Q, images, INF, True)
        assert want[1][0].shape[0] > 0
        for budget, chunks in ((before, 1), (1, 3)):
            ctx.set_option("coll_ws_bytes", budget)
            l0, f0 = ctx.f32_filter_stats()
            counts = coll.wide_mutual_ratio_each_counts(qb, INF, True)
            l1, f1 = ctx.f32_filter_stats()
            assert (l1 - l0, f1 - f0) == (chunks, 1), (budget, l1 - l0, f1 - f0)     # one fallback: the overflowed chunk's
            got = coll.wide_mutual_ratio_each(qb, INF, True)
            assert np.diff(counts).tolist() == [g[0].shape[0] for g in got]
            for i in range(3):
                _same(got[i], want[i], "budget %s image %d" % (budget, i))
    finally:
        ctx.set_option("coll_ws_bytes", before)
        ctx.set_option("f32_filter", old)
        qb.close()
        coll.close()


def test_cap_rules(ctx):
    dim = 129
    images, Q, _ = _data(dim)
    want = _want(dim, 0.8, False)
    coll = _collection(ctx, images)
    qb = ctx.bank(Q)
    try:
        offsets, total_rows, cols = ref.pack(want, 1 << 40)
        mid = int(offsets[5]) + 1                      # ends inside image 5: images 0 .. 4 are whole
        assert offsets[5] > 0 and offsets[6] > mid
        got = coll.wide_mutual_ratio_each(qb, 0.8, False, cap=mid)
        for i in range(8):
            if i < 5:
                _same(got[i], want[i], "cap %d image %d" % (mid, i))
            else:
                assert got[i][0].shape[0] == 0
        # the raw call: offsets hold the full counts whatever cap is; cap = 0 takes NULL arrays
        lib, h = ctx.lib, ctx.handle
        P = _ffi._ptr
        for cap in (mid, 0, total_rows):
            off = np.full(9, -7, np.int64)
            qi, ti = np.full(max(cap, 1), -7, np.int32), np.full(max(cap, 1), -7, np.int32)
            d, r = np.full(max(cap, 1), -7, np.float32), np.full(max(cap, 1), -7, np.float64)
            n = ctypes.c_int64(-7)
            rc = lib.fm_collection_wide_mutual_ratio_each(h, coll.handle, qb.handle, 0.8, 0, cap, P(off), P(qi) if cap else None,
                                                          P(ti) if cap else None, P(d) if cap else None, P(r) if cap else None, ctypes.byref(n))
            assert rc == 0 and off.tolist() == offsets.tolist() and n.value == total_rows
            whole = ref.pack(want, cap)[1]
            assert np.array_equal(qi[:whole], cols[0][:whole]) and np.array_equal(ti[:whole], cols[1][:whole])
            assert np.array_equal(_bits(d[:whole]), _bits(cols[2][:whole])) and (qi[whole:] == -7).all()
    finally:
        qb.close()
        coll.close()


def test_device_form_and_torchmatch(ctx):
    import torch
    from fastmatch_amd import torchmatch
    dim = 256
    images, Q, _ = _data(dim)
    coll = _collection(ctx, images)
    qb = ctx.bank(Q)
    side = torch.cuda.Stream()                         # a consumer stream that is not the context's
    try:
        for tau, sym in ((0.8, True), (INF, False)):
            want = coll.wide_mutual_ratio_each(qb, tau, sym)
            offsets = coll.wide_mutual_ratio_each_counts(qb, tau, sym)
            total, n = int(offsets[-1]), len(want)
            mid = int(offsets[n // 2 + 1]) - 1
            for cap in (total + 3, max(mid, 0), 0):
                with torch.cuda.stream(side):
                    rows = torch.full((cap, 3), -7, dtype=torch.int32, device="cuda")
                    d_off = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
                    got_total = coll.wide_mutual_ratio_each_dev(qb, tau, sym, d_off.data_ptr(), rows.data_ptr() if cap else 0, cap,
                                                                want_total=True, consumer_stream=side.cuda_stream)
                    h_off, got = d_off.cpu().numpy(), rows.cpu().numpy()
                assert got_total == total and h_off.tolist() == offsets.tolist()
                whole = ref.pack(want, cap)[1]
                at = 0
                for i in range(n):
                    k = want[i][0].shape[0]
                    if at + k > whole:
                        break
                    assert np.array_equal(got[at:at + k, 0], want[i][0]) and np.array_equal(got[at:at + k, 1], want[i][1])
                    assert np.array_equal(got[at:at + k, 2].view(np.uint32), _bits(want[i][2]))
                    at += k
                assert at == whole and (got[whole:] == -7).all()          # the longest prefix of WHOLE images
        # the _dev call is not accounted in fm_stats
        ctx.sync()
        s0 = ctx.stats()
        d_off = torch.zeros(9, dtype=torch.int64, device="cuda")
        coll.wide_mutual_ratio_each_dev(qb, 0.8, False, d_off.data_ptr(), 0, 0, consumer_stream=torch.cuda.current_stream().cuda_stream)
        ctx.sync()
        assert ctx.stats()["pairs"] == s0["pairs"]
        # torchmatch: images and query from tensors of the three dtypes, against the reference on the widened values
        for dt in (torch.float32, torch.float16, torch.bfloat16):
            src = [torch.from_numpy(im).cuda().to(dt) for im in images]
            tq = torch.from_numpy(Q).cuda().to(dt)
            wide_images = [t.float().cpu().numpy() for t in src]
            wq = tq.float().cpu().numpy()
            packed = ref.pack(ref.mutual_ratio_each(wq, wide_images, 0.8, True), 1 << 40)
            with torchmatch.Collection(context=ctx) as tc:
                for i, t in enumerate(src):
                    assert tc.add_wide(t) == i
                for cap in (None, packed[1] + 4):
                    offsets, rows = tc.wide_mutual_ratio_each(tq, 0.8, symmetric=True, cap=cap)
                    assert offsets.cpu().numpy().tolist() == packed[0].tolist()
                    got = rows.cpu().numpy()[:packed[1]]
                    assert np.array_equal(got[:, 0], packed[2][0]) and np.array_equal(got[:, 1], packed[2][1])
                    assert np.array_equal(got[:, 2].view(np.uint32), _bits(packed[2][2]))
                with pytest.raises(ValueError, match="wide"):
                    tc.knn(tq, 2)
        # matchutil: BFMatcher.add_wide, the three wide-query methods
        m = matchutil.BFMatcher()
        m.add_wide(images)
        want = coll.wide_mutual_ratio_each(qb, 0.8, True)
        lists = m.mutualRatioMatchWideEach_arrays(Q, 0.8, True)
        for i in range(len(images)):
            _same(lists[i], want[i], "BFMatcher image %d" % i)
        dm = m.mutualRatioMatchWideEach(Q, 0.8, True)
        assert [len(v) for v in dm] == [w[0].shape[0] for w in want] and all(x.imgIdx == 5 for x in dm[5])
        k_idx, k_dist = m.knnMatchWideEach_arrays(Q)
        w_idx, w_dist = coll.wide_knn2_each(qb)
        assert np.array_equal(k_idx, w_idx) and np.array_equal(_bits(k_dist), _bits(w_dist))
    finally:
        qb.close()
        coll.close()


def test_stats_account_the_sweeps(ctx):
    images, Q, _ = _data(129)
    coll = _collection(ctx, images)
    qb = ctx.bank(Q)
    try:
        ctx.sync()
        before = ctx.stats()
        coll.wide_mutual_ratio_each_counts(qb, 0.8)                                # (one C call)
        mid = ctx.stats()
        assert mid["pairs"] - before["pairs"] == 2 * 300 * sum(SIZES)
        coll.wide_knn2_each(qb)
        assert ctx.stats()["pairs"] - mid["pairs"] == 300 * sum(SIZES)
    finally:
        qb.close()
        coll.close()


def test_errors_and_empty_cases(ctx):
    rng = np.random.default_rng(9600)
    w = rng.standard_normal((50, 200)).astype(np.float32)
    narrow = rng.standard_normal((50, 128)).astype(np.float32)
    lib, h = ctx.lib, ctx.handle
    P = _ffi._ptr
    NOS = _ffi._stream_arg(None)
    off = np.zeros(16, np.int64)
    z = np.zeros(4096, np.int64)
    A = [P(z)] * 6

    def err():
        return lib.fm_last_error(h).decode()

    knn2, mut, mut_dev = lib.fm_collection_wide_knn2_each, lib.fm_collection_wide_mutual_ratio_each, lib.fm_collection_wide_mutual_ratio_each_dev
    coll, other, empty = ctx.collection(), ctx.collection(), ctx.collection()
    made = []
    try:
        import torch
        wq = ctx.bank(w); made.append(wq)
        w256 = ctx.bank(rng.standard_normal((5, 256)).astype(np.float32)); made.append(w256)
        nq_ = ctx.bank(narrow, float_route=True); made.append(nq_)
        q0 = ctx.bank(np.zeros((0, 200), np.float32)); made.append(q0)
        assert q0.kind == _ffi.FM_BANK_F32W
        coll.add_wide(w)
        coll.add_wide(np.zeros((0, 200), np.float32))
        coll.add_wide(w[:7].copy())
        other.add(narrow)
        state = (coll.info(), coll.image_rows().tolist())
        d_off = torch.zeros(4, dtype=torch.int64, device="cuda")
        d_rows = torch.zeros((10, 3), dtype=torch.int32, device="cuda")

        def each(c, b, cap=10, offsets=P(off), arrays=None):
            a = A[:4] if arrays is None else arrays
            return mut(h, c, b, 0.8, 0, cap, offsets, *a, None)

        # 1. handles
        assert each(None, wq.handle) == EINVAL and mut(None, coll.handle, wq.handle, 0.8, 0, 10, P(off), *A[:4], None) == EINVAL
        assert each(coll.handle, None) == EINVAL and "NULL" in err()
        assert knn2(h, None, wq.handle, *A[:2]) == EINVAL and knn2(h, coll.handle, None, *A[:2]) == EINVAL
        assert mut_dev(h, None, wq.handle, 0.8, 0, 10, d_off.data_ptr(), d_rows.data_ptr(), None, NOS) == EINVAL
        # 2. a collection of another kind: before the query is looked at
        for b in (wq, nq_):
            assert each(other.handle, b.handle) == EINVAL and "fm_collection_mutual_ratio_each" in err()
            assert mut_dev(h, other.handle, b.handle, 0.8, 0, 10, d_off.data_ptr(), d_rows.data_ptr(), None, NOS) == EINVAL
            assert "fm_collection_mutual_ratio_each" in err()
            assert knn2(h, other.handle, b.handle, *A[:2]) == EINVAL and "fm_collection_knn2_each" in err()
        # 3. the query's kind and width, before the output pointers
        assert each(coll.handle, nq_.handle, cap=-1, offsets=None) == EINVAL and "wide" in err()
        assert each(coll.handle, w256.handle, cap=-1, offsets=None) == EINVAL and "width" in err()
        assert knn2(h, coll.handle, w256.handle, None, None) == EINVAL and "width" in err()
        assert knn2(h, empty.handle, nq_.handle, None, None) == EINVAL and "wide" in err()
        q0n = ctx.bank(np.zeros((0, 128), np.float32)); made.append(q0n)
        assert each(coll.handle, q0n.handle) == EINVAL             # even an empty query must be wide
        # 4. the mutual calls' output pointers
        assert each(coll.handle, wq.handle, cap=-1) == EINVAL and "cap" in err()
        assert each(coll.handle, wq.handle, offsets=None) == EINVAL and "offsets" in err()
        for k in range(4):
            arrays = list(A[:4])
            arrays[k] = None
            assert each(coll.handle, wq.handle, arrays=arrays) == EINVAL and "NULL" in err()
        assert mut_dev(h, coll.handle, wq.handle, 0.8, 0, 10, None, d_rows.data_ptr(), None, NOS) == EINVAL
        assert mut_dev(h, coll.handle, wq.handle, 0.8, 0, 10, d_off.data_ptr(), None, None, NOS) == EINVAL
        assert mut_dev(h, coll.handle, wq.handle, 0.8, 0, 10, P(off), d_rows.data_ptr(), None, NOS) == EINVAL       # host memory
        assert mut_dev(h, coll.handle, wq.handle, 0.8, 0, 10, d_off.data_ptr(), P(z), None, NOS) == EINVAL
        # 5. knn2's output pointers
        assert knn2(h, coll.handle, wq.handle, None, A[0]) == EINVAL and knn2(h, coll.handle, wq.handle, A[0], None) == EINVAL
        assert (coll.info(), coll.image_rows().tolist()) == state
        # the sixteen existing calls still refuse this collection, whatever the query
        coll.train()
        mk = other.mask(4); made.append(mk)
        calls = [
            lambda b: lib.fm_collection_knn(h, coll.handle, b, 1, *A[:3]),
            lambda b: lib.fm_collection_knn_dev(h, coll.handle, b, 1, None, None, None, NOS),
            lambda b: lib.fm_collection_knn2_ratio(h, coll.handle, b, 0.8, 10, *A[:5], None),
            lambda b: lib.fm_collection_knn2_ratio_dev(h, coll.handle, b, 0.8, 10, None, None, None, NOS),
            lambda b: lib.fm_collection_knn2_each(h, coll.handle, b, *A[:2]),
            lambda b: lib.fm_collection_votes(h, coll.handle, b, 0.8, 0, A[0]),
            lambda b: lib.fm_collection_knn_masked(h, coll.handle, b, mk.handle, 1, *A[:3]),
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
        assert len(calls) == 16
        for n, call in enumerate(calls):
            for b in (nq_, wq):
                rc = call(b.handle)
                assert rc == EUNSUPPORTED and "wide" in err(), (n, rc, err())
        assert (coll.info(), coll.image_rows().tolist()) == state
        # valid empty cases.  A collection on which no add has succeeded: offsets[0] = 0
        off[:] = -7
        n = ctypes.c_int64(-7)
        assert mut(h, empty.handle, wq.handle, 0.8, 0, 0, P(off), None, None, None, None, ctypes.byref(n)) == 0
        assert off[0] == 0 and n.value == 0
        assert knn2(h, empty.handle, wq.handle, None, None) == 0
        assert empty.wide_mutual_ratio_each(wq, 0.8) == [] and empty.wide_knn2_each(wq)[0].shape == (0, 50, 2)
        # nq = 0: all-zero offsets, NULL arrays with n_images * nq = 0
        assert coll.wide_mutual_ratio_each_counts(q0, 0.8).tolist() == [0, 0, 0, 0]
        assert knn2(h, coll.handle, q0.handle, None, None) == 0 and coll.wide_knn2_each(q0)[0].shape == (3, 0, 2)
        # empty images only
        empty.add_wide(np.zeros((0, 200), np.float32))
        empty.add_wide(np.zeros((0, 200), np.float32))
        assert empty.wide_mutual_ratio_each_counts(wq, INF).tolist() == [0, 0, 0]
        k_idx, k_dist = empty.wide_knn2_each(wq)
        assert (k_idx == -1).all() and np.isinf(k_dist).all() and k_idx.shape == (2, 50, 2)
        # and the call that is served: every row of w finds itself in image 0
        got = coll.wide_mutual_ratio_each(wq, INF)
        assert got[0][0].tolist() == got[0][1].tolist() == list(range(50)) and got[1][0].shape[0] == 0
        assert got[2][0].tolist() == list(range(7))
        want = ref.mutual_ratio_each(w, [w, w[:0], w[:7]], INF)
        for i in range(3):
            _same(got[i], want[i], "image %d" % i)
    finally:
        for b in made:
            b.close()
        coll.close()
        other.close()
        empty.close()
