"""GPU: Fast-Match's self-distance test on binary descriptors -- fm_hamming_self_dist(_batch), fm_hamming_set_selfdist,
fm_hamming_match_ratio, fm_hamming_match_accepted(_dev), fm_collection_hamming_match_accepted_each(_dev) and the Python layers
on top -- against the NumPy reference (tests/hamming_fast_ref.py).  Every comparison is exact: integers, float32 and float64
bit patterns (NaNs by position); there is no tolerance anywhere.

Shapes follow the self sweep's geometry: a stage is 128 reduced rows, a workgroup owns 256 output rows (a chunk), whose
diagonal lies in the stages 2 chunk and 2 chunk + 1; 1300 rows are 11 stages in 3 splits (asserted from the restated rule)."""
import ctypes

import numpy as np
import pytest

import fastmatch_amd
import hamming_fast_ref as HF
import hamming_ref as H
from fastmatch_amd import _ffi, matchutil, torchmatch

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -4
INF = float("inf")
SIZES = [1, 2, 3, 127, 128, 129, 255, 256, 257, 1300]
WIDTHS = [1, 16, 17, 32, 33, 40, 48, 61, 64]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _knn2_second(ctx, b):
    """The existing way to the same values: the second column of fm_knn2(b, b), as float64."""
    return ctx.knn2(b, b)[1][:, 1].astype(np.float64)


def _splits(n):
    """plan_hamming's split count for an n x n sweep, restated."""
    n_pad = (n + 127) // 128 * 128
    nchunks, nstages = (n_pad + 255) // 256, n_pad // 128
    ns = max(1, min((2048 + nchunks - 1) // nchunks, (nstages + 3) // 4))
    per = (nstages + ns - 1) // ns
    return (nstages + per - 1) // per


def _check_self(ctx, B, expect=None):
    ref = HF.self_dist(B) if expect is None else expect
    b = ctx.bank_binary(B)
    try:
        got = ctx.hamming_self_dist(b)
        assert got.dtype == np.float64 and _same(got, ref), (B.shape, np.nonzero(_bits(got) != _bits(ref))[0][:8])
        assert _same(got, _knn2_second(ctx, b))
    finally:
        b.close()
    return ref


# ---- self distances ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", WIDTHS)
def test_self_dist_sizes(ctx, width):
    assert _splits(1300) == 3 and _splits(257) == 1
    rng = np.random.default_rng(100 + width)
    for n in SIZES:
        ref = _check_self(ctx, rng.integers(0, 256, (n, width), dtype=np.uint8))
        if n == 1:
            assert ref[0] == np.inf


@pytest.mark.parametrize("width", [17, 32, 64])
@pytest.mark.parametrize("n,at", [(2, 1), (130, 129), (130, 0), (300, 131), (385, 384)])
def test_isolated_row_beyond_half_the_width(ctx, width, n, at):
    """Padding rows are all-zero FP4 rows, W / 2 from everything.  A row whose nearest real neighbour is FARTHER than W / 2
    would take a padding row as its neighbour if padding were excluded by value.  Three rows that hold a complement pair cannot
    all be more than W / 2 apart (d(y, x) + d(y, ~x) = W), so the bank is: row `at` = x, every other row ~x with up to two
    bits flipped -- x's nearest neighbour is at W - 2 or farther; n = 2 is the pair (x, ~x), where every distance exceeds W / 2.
    n % 128 != 0: the tail stage holds padding."""
    rng = np.random.default_rng(7 * n + width)
    W = 8 * width
    x = rng.integers(0, 256, width, dtype=np.uint8)
    B = np.repeat((~x)[None, :], n, axis=0)
    for i in range(n):
        for bit in rng.integers(0, W, int(rng.integers(0, 3))):
            B[i, bit // 8] ^= np.uint8(1 << (bit % 8))
    B[at] = x
    ref = HF.self_dist(B)
    assert ref[at] >= W - 2 > W / 2 and n % 128 != 0
    _check_self(ctx, B, ref)


def test_duplicates_and_equal_banks(ctx):
    rng = np.random.default_rng(11)
    B = rng.integers(0, 256, (300, 32), dtype=np.uint8)
    B[200] = B[10]                    # a duplicate at a higher index, in another chunk
    B[299] = B[298]                   # neighbours in the tail stage
    B[3] = B[130]                     # ... and at a lower index, across a stage
    ref = _check_self(ctx, B)
    assert all(ref[i] == 0.0 for i in (10, 200, 298, 299, 3, 130)) and (ref[[0, 1, 2]] > 0).all()
    for n in (2, 130, 257):
        same = np.repeat(rng.integers(0, 256, (1, 61), dtype=np.uint8), n, axis=0)
        assert not _check_self(ctx, same).any()


@pytest.mark.parametrize("n,row", [(300, 5), (300, 298), (1300, 700), (257, 0)])
def test_neighbour_in_the_last_real_row(ctx, n, row):
    """Row `row`'s nearest neighbour is the LAST real row, in the tail stage, behind which the padding starts."""
    rng = np.random.default_rng(n + row)
    B = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    B[n - 1] = B[row]
    B[n - 1, 7] ^= 0x10
    ref = _check_self(ctx, B)
    assert ref[row] == 1.0 and ref[n - 1] == 1.0


def _eight_banks(ctx):
    rng = np.random.default_rng(23)
    shapes = [(300, 32), (1, 32), (130, 17), (257, 61), (1300, 61), (0, 32), (128, 17), (40, 61)]
    mats = [rng.integers(0, 256, s, dtype=np.uint8) for s in shapes]
    mats[2][100] = mats[2][4]
    return mats, [ctx.bank_binary(m) for m in mats]


def test_batched_self_dist(ctx):
    """Eight banks of mixed sizes, three widths in two K-step counts, one of them empty, in ONE call: the attached values and
    the returned ones against the one-by-one call."""
    mats, banks = _eight_banks(ctx)
    rng = np.random.default_rng(29)
    tmats = {w: rng.integers(0, 256, (500, w), dtype=np.uint8) for w in (17, 32, 61)}
    trains = {w: ctx.bank_binary(m) for w, m in tmats.items()}
    try:
        single = [ctx.hamming_self_dist(b) for b in banks]
        for m, s in zip(mats, single):
            assert _same(s, HF.self_dist(m))
        # the `out` form: synchronous, every array returned
        outs = ctx.hamming_self_dist_batch(banks)
        assert len(outs) == 8 and all(_same(o, s) for o, s in zip(outs, single))
        via_out = [ctx.hamming_match_ratio(b, trains[b.dim], 0.9) for b in banks]
        # the enqueue-only form on fresh banks: nothing comes back, the values are attached on the device
        fresh = [ctx.bank_binary(m) for m in mats]
        assert ctx.hamming_self_dist_batch(fresh, want_host=False) is None
        for m, b, s, v in zip(mats, fresh, single, via_out):
            tidx, dist, ratio, passed, npass = ctx.hamming_match_ratio(b, trains[b.dim], 0.9)
            assert _same(tidx, v[0]) and _same(dist, v[1]) and HF.same_f64(ratio, v[2]) and np.array_equal(passed, v[3]) and npass == v[4]
            # ... and they are the one-by-one values: the ratios are those of a division by the same words
            rt, rd, rr, rp = HF.match_ratio(m, tmats[b.dim], s, 0.9)
            assert _same(tidx, rt) and HF.same_f64(ratio, rr) and np.array_equal(passed, rp)
        # a bank listed twice
        hs = (ctypes.c_void_p * 2)(banks[0].handle, banks[0].handle)
        assert ctx.lib.fm_hamming_self_dist_batch(ctx.handle, 2, hs, None) == EINVAL
        assert "listed twice" in ctx.lib.fm_last_error(ctx.handle).decode()
        for b in fresh:
            b.close()
    finally:
        for b in banks + list(trains.values()):
            b.close()


# ---- bank pairs ------------------------------------------------------------------------------------------------------------
def _planted(nq, nt, width, seed):
    """A pair with planted near-duplicates: some query rows have a train row 0 .. 3 bits away (accepted at small tau), some
    have a duplicate inside the query bank (selfdist 0: never accepted), the rest are random (ratio near 1)."""
    rng = np.random.default_rng(seed)
    Q = rng.integers(0, 256, (nq, width), dtype=np.uint8)
    T = rng.integers(0, 256, (nt, width), dtype=np.uint8)
    for k in range(0, min(nq, nt), 3):
        T[(k * 7) % nt] = Q[k]
        for bit in rng.integers(0, 8 * width, int(rng.integers(0, 4))):
            T[(k * 7) % nt, bit // 8] ^= np.uint8(1 << (bit % 8))
    if nq > 40 and nt > 10:
        Q[17] = Q[4]                  # selfdist 0 for both (every train row elects the lower one, row 4)
        T[5] = Q[4]
        T[5, 0] ^= 1                  # ... at d = 1 from train row 5: 1 / 0 = +inf
        Q[30] = Q[8]
        T[9] = Q[8]                   # ... and row 8 at d = 0: 0 / 0 = NaN
    return Q, T


PAIRS = [(300, 700, 32, 1), (129, 1, 32, 2), (1, 129, 61, 3), (257, 300, 17, 4), (40, 1300, 64, 5)]


@pytest.fixture(scope="module")
def pairs(ctx):
    out = []
    for nq, nt, w, seed in PAIRS:
        Q, T = _planted(nq, nt, w, seed)
        qb, tb = ctx.bank_binary(Q), ctx.bank_binary(T)
        sd = ctx.hamming_self_dist_batch([qb])[0]
        assert _same(sd, HF.self_dist(Q))
        out.append((Q, T, sd, qb, tb))
    yield out
    for _, _, _, qb, tb in out:
        qb.close()
        tb.close()


@pytest.mark.parametrize("tau", [0.6, 0.9, INF])
def test_match_ratio_and_accepted(ctx, pairs, tau):
    some_pass = some_fail = False
    for Q, T, sd, qb, tb in pairs:
        rt, rd, rr, rp = HF.match_ratio(Q, T, sd, tau)
        tidx, dist, ratio, passed, npass = ctx.hamming_match_ratio(qb, tb, tau)
        assert _same(tidx, rt) and _same(dist, rd) and HF.same_f64(ratio, rr) and np.array_equal(passed, rp) and npass == rp.sum()
        xt, xd = ctx.xcheck1(qb, tb)                          # the cross-check is fm_xcheck1's
        assert _same(tidx, xt) and _same(dist, xd)
        aq, at, ad, ar = HF.match_accepted(Q, T, sd, tau)
        q, t, d, r = ctx.hamming_match_accepted(qb, tb, tau)
        assert _same(q, aq) and _same(t, at) and _same(d, ad) and _same(r, ar)
        some_pass |= bool(rp.any())
        some_fail |= bool(((rt >= 0) & ~rp).any())
        if len(Q) == 1:                                       # a bank of one query row: selfdist +inf, ratio 0
            assert sd[0] == np.inf and (tau <= 0 or (rp[0] and rr[0] == 0.0))
    assert some_pass and some_fail
    Q, T, sd, qb, tb = pairs[0]
    rt, rd, rr, rp = HF.match_ratio(Q, T, sd, tau)
    assert sd[4] == 0 and rd[4] == 1 and rr[4] == np.inf and not rp[4]            # d / 0
    assert sd[8] == 0 and rd[8] == 0 and np.isnan(rr[8]) and not rp[8]            # 0 / 0


def test_accepted_cap_and_device_rows(ctx, pairs):
    import torch
    Q, T, sd, qb, tb = pairs[0]
    aq, at, ad, ar = HF.match_accepted(Q, T, sd, 0.9)
    m = len(aq)
    assert m > 8
    for cap in (m - 5, 0, m, m + 9):
        out = tuple(np.full(max(cap, 1), -9, dt) for dt in (np.int32, np.int32, np.float32, np.float64))
        n = ctypes.c_int64(-1)
        rc = ctx.lib.fm_hamming_match_accepted(ctx.handle, qb.handle, tb.handle, 0.9, cap, *[_ffi._ptr(a) for a in out], ctypes.byref(n))
        assert rc == 0 and n.value == m                       # the FULL count, whatever the capacity
        k = min(cap, m)
        assert _same(out[0][:k], aq[:k]) and _same(out[1][:k], at[:k]) and _same(out[2][:k], ad[:k]) and _same(out[3][:k], ar[:k])
        assert (out[0][k:] == -9).all()
        rows = torch.full((max(cap, 1), 3), -9, dtype=torch.int32, device="cuda")
        cnt = torch.full((1,), -9, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        assert ctx.hamming_match_accepted_dev(qb, tb, 0.9, rows.data_ptr(), cnt.data_ptr(), cap) == m
        r = rows.cpu().numpy()
        assert int(cnt.item()) == k                           # fm_match_accepted_dev's rule: the rows written
        assert _same(r[:k, 0], aq[:k]) and _same(r[:k, 1], at[:k]) and _same(r[:k, 2].view(np.float32), ad[:k])
        assert (r[k:] == -9).all()


def test_caller_self_distances_are_honoured(ctx, pairs):
    Q, T, sd, _, tb = pairs[0]
    qb = ctx.bank_binary(Q)
    try:
        mine = np.linspace(1.0, 300.0, len(Q))
        mine[3], mine[9] = 0.0, np.inf
        qb.set_hamming_selfdist(mine)
        rt, rd, rr, rp = HF.match_ratio(Q, T, mine, 0.9)
        tidx, dist, ratio, passed, npass = ctx.hamming_match_ratio(qb, tb, 0.9)
        assert _same(tidx, rt) and HF.same_f64(ratio, rr) and np.array_equal(passed, rp) and npass == rp.sum()
        ctx.hamming_self_dist_batch([qb], want_host=False)    # ... and computed ones replace them
        assert HF.same_f64(ctx.hamming_match_ratio(qb, tb, 0.9)[2], HF.match_ratio(Q, T, sd, 0.9)[2])
    finally:
        qb.close()


def test_empty_banks(ctx):
    e = ctx.bank_binary(np.zeros((0, 32), np.uint8))
    t = ctx.bank_binary(np.random.default_rng(1).integers(0, 256, (50, 32), dtype=np.uint8))
    try:
        assert ctx.hamming_self_dist(e).shape == (0,)
        assert ctx.hamming_self_dist_batch([e])[0].shape == (0,)
        assert all(len(a) == 0 for a in ctx.hamming_match_accepted(e, t, 0.9))      # no rows, and no self distances needed
        ctx.hamming_self_dist_batch([t], want_host=False)
        tidx, dist, ratio, passed, npass = ctx.hamming_match_ratio(t, e, 0.9)       # an empty train bank: nothing matches
        assert (tidx == -1).all() and np.isinf(dist).all() and npass == 0
    finally:
        e.close()
        t.close()


def test_stats_count_pairs(ctx):
    rng = np.random.default_rng(5)
    q, t = ctx.bank_binary(rng.integers(0, 256, (300, 32), dtype=np.uint8)), ctx.bank_binary(rng.integers(0, 256, (170, 32), dtype=np.uint8))
    try:
        ctx.sync()
        ctx.reset_stats()
        ctx.hamming_self_dist(q)
        assert ctx.stats()["pairs"] == 300 * 300
        q.set_hamming_selfdist(ctx.hamming_self_dist(q))
        ctx.reset_stats()
        ctx.hamming_match_accepted(q, t, 0.9)
        assert ctx.stats()["pairs"] == 300 * 170
        assert ctx.lib.fm_abi_version() == _ffi.FM_ABI_VERSION == 12
    finally:
        q.close()
        t.close()


# ---- collections -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gallery(ctx):
    """Four images, one of them empty; the query shares planted rows with each."""
    rng = np.random.default_rng(41)
    Q = rng.integers(0, 256, (300, 32), dtype=np.uint8)
    Q[250] = Q[20]
    images = []
    for i, n in enumerate((400, 0, 129, 260)):
        img = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        for k in range(i, min(n, 300), 4):
            img[(k * 5) % n] = Q[k]
            img[(k * 5) % n, k % 32] ^= np.uint8(1 << (k % 8)) if k % 3 else np.uint8(0)
        images.append(img)
    qb = ctx.bank_binary(Q)
    sd = ctx.hamming_self_dist_batch([qb])[0]
    coll = ctx.collection()
    for img in images:
        coll.add_binary(img)
    yield Q, sd, qb, images, coll
    coll.close()
    qb.close()


@pytest.mark.parametrize("ws_bytes", [0, 4096])
def test_collection_each_equals_the_pair_call(ctx, gallery, ws_bytes):
    """Every image of the collection call equals the bank-pair call on that image; with a small coll_ws_bytes (17 bytes per
    (image, query row): 300 rows are 5100, so 4096 holds ONE image) the images run in several chunks."""
    Q, sd, qb, images, coll = gallery
    before = ctx.get_option("coll_ws_bytes")
    ctx.set_option("coll_ws_bytes", ws_bytes)
    try:
        for tau in (0.6, INF):
            got = coll.hamming_match_accepted_each(qb, tau)
            assert len(got) == 4 and len(got[1][0]) == 0
            total = 0
            for img, g in zip(images, got):
                tb = ctx.bank_binary(img)
                pair = ctx.hamming_match_accepted(qb, tb, tau)
                tb.close()
                ref = HF.match_accepted(Q, img, sd, tau)
                assert all(_same(a, b) for a, b in zip(g, pair)) and all(_same(a, b) for a, b in zip(g, ref))
                total += len(ref[0])
            assert total > 20
        # cap below the count: the full counts, the first rows
        capped = coll.hamming_match_accepted_each(qb, INF, cap=7)
        full = coll.hamming_match_accepted_each(qb, INF)
        assert all(_same(c[0], f[0][:7]) and _same(c[3], f[3][:7]) for c, f in zip(capped, full))
    finally:
        ctx.set_option("coll_ws_bytes", before)


def test_collection_each_dev_with_a_consumer_stream(ctx, gallery):
    import torch
    Q, sd, qb, images, coll = gallery
    ref = [HF.match_accepted(Q, img, sd, 0.9) for img in images]
    cap = 40
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        rows = torch.full((4, cap, 3), -9, dtype=torch.int32, device="cuda")
        cnt = torch.full((4,), -9, dtype=torch.int64, device="cuda")
        h = np.full(4, -9, np.int64)
        coll.hamming_match_accepted_each_dev(qb, 0.9, rows.data_ptr(), cnt.data_ptr(), cap, h_counts=h, consumer_stream=side.cuda_stream)
        r, c = rows.cpu().numpy(), cnt.cpu().numpy()          # (read on the consumer stream, which waits for the fills)
    assert np.array_equal(h, [len(x[0]) for x in ref]) and np.array_equal(c, np.minimum(h, cap))
    for i, (aq, at, ad, _) in enumerate(ref):
        k = int(c[i])
        assert _same(r[i, :k, 0], aq[:k]) and _same(r[i, :k, 1], at[:k]) and _same(r[i, :k, 2].view(np.float32), ad[:k])
        assert (r[i, k:] == -9).all()


def test_matchutil_and_torch_layers(ctx, gallery):
    import torch
    Q, sd, qb, images, coll = gallery
    ref = [HF.match_accepted(Q, img, sd, 0.8) for img in images]
    opts = {"context": ctx}
    # matchutil: arrays, DMatch lists, the matcher
    got = matchutil.hamming_fast_match_arrays(Q, images[0], 0.8, options=opts)
    assert all(_same(a, b) for a, b in zip(got, ref[0]))
    dm = matchutil.hamming_fast_match(Q, images[3], 0.8, options=opts)
    assert [(m.queryIdx, m.trainIdx, m.distance) for m in dm] == [(int(q), int(t), float(d)) for q, t, d, _ in zip(*ref[3])]
    bf = matchutil.BFMatcher(matchutil.NORM_HAMMING, options=opts)
    bf.add(images)
    each = bf.hammingFastMatchEach_arrays(Q, 0.8)
    assert len(each) == 4 and all(all(_same(a, b) for a, b in zip(g, r)) for g, r in zip(each, ref))
    lists = bf.hammingFastMatchEach(Q, 0.8)
    assert [len(l) for l in lists] == [len(r[0]) for r in ref] and all(m.imgIdx == 2 for m in lists[2])
    with pytest.raises(ValueError, match="hammingFastMatchEach"):
        bf.fastMatchEach(Q, 0.8)
    # torchmatch: tensors in, device rows out; the self distances are computed on the device
    tq, tt = torch.from_numpy(Q).cuda(), torch.from_numpy(images[0]).cuda()
    rows, count = torchmatch.hamming_fast_match(tq, tt, 0.8)
    r = rows.cpu().numpy()
    assert int(count.item()) == len(ref[0][0]) == len(r)
    assert _same(r[:, 0], ref[0][0]) and _same(r[:, 1], ref[0][1]) and _same(r[:, 2].view(np.float32), ref[0][2])
    rows2, _ = torchmatch.hamming_fast_match(qb, tt, 0.8)     # a resident bank that carries its own
    assert torch.equal(rows, rows2)
    with torchmatch.Collection(context=ctx) as tc:
        for img in images:
            tc.add(torch.from_numpy(img).cuda(), binary=True)
        erows, ecnt = tc.hamming_fast_match_each(qb, 0.8)
        torch.cuda.synchronize()
        er, ec = erows.cpu().numpy(), ecnt.cpu().numpy()
        assert np.array_equal(ec, [len(x[0]) for x in ref])
        for i, (aq, at, ad, _) in enumerate(ref):
            k = len(aq)
            assert _same(er[i, :k, 0], aq) and _same(er[i, :k, 1], at) and _same(er[i, :k, 2].view(np.float32), ad)
        with pytest.raises(ValueError, match="binary Bank"):
            tc.hamming_fast_match_each(tq, 0.8)


# ---- errors ----------------------------------------------------------------------------------------------------------------
def test_refusal_order(ctx, gallery):
    Q, sd, qb, images, coll = gallery
    lib, h = ctx.lib, ctx.handle
    rng = np.random.default_rng(3)
    l2 = ctx.bank(rng.integers(0, 256, (20, 128), dtype=np.uint8))
    narrow = ctx.bank_binary(rng.integers(0, 256, (20, 16), dtype=np.uint8))       # another width, and no self distances
    bare = ctx.bank_binary(Q[:20])                                                  # the right width, no self distances
    tb = ctx.bank_binary(images[0])
    I64 = ctypes.c_int64

    def err():
        return lib.fm_last_error(h).decode()

    def pair_calls(q, t, cap=4, null_out=False):
        """The three bank-pair calls with valid outputs (or NULL ones): [(name, rc, message)]."""
        n = max(q.n if q is not None else 1, 1)
        a = [np.zeros(n, dt) for dt in (np.int32, np.int32, np.float32, np.float64)]
        p = [None] * 4 if null_out else [_ffi._ptr(x) for x in a]
        qh, th = (q.handle if q is not None else None), (t.handle if t is not None else None)
        out = []
        out.append(("fm_hamming_match_ratio", lib.fm_hamming_match_ratio(h, qh, th, 0.9, p[1], p[2], p[3], None, None), err()))
        out.append(("fm_hamming_match_accepted", lib.fm_hamming_match_accepted(h, qh, th, 0.9, cap, p[0], p[1], p[2], p[3], ctypes.byref(I64())), err()))
        return out

    try:
        # 1. NULL handles
        for name, rc, msg in pair_calls(None, tb) + pair_calls(qb, None):
            assert rc == EINVAL and "NULL" in msg, (name, msg)
        assert lib.fm_hamming_self_dist(h, None, None) == EINVAL and lib.fm_hamming_set_selfdist(h, None, None) == EINVAL
        assert lib.fm_hamming_match_accepted_dev(h, None, tb.handle, 0.9, 4, None, None, None) == EINVAL
        # 2. not binary -- in front of the width (l2 is 128 wide, tb 32), the self distances (l2 has none), cap and the outputs
        for q, t in ((l2, tb), (qb, l2)):
            for name, rc, msg in pair_calls(q, t, cap=-1, null_out=True):
                assert rc == EINVAL and "binary" in msg and name.replace("_hamming", "") + " is the L2 call" in msg, (name, msg)
        assert lib.fm_hamming_match_accepted_dev(h, l2.handle, tb.handle, 0.9, -1, None, None, None) == EINVAL
        assert "fm_match_accepted_dev is the L2 call" in err()
        out = np.zeros(20)
        assert lib.fm_hamming_self_dist(h, l2.handle, _ffi._ptr(out)) == EINVAL and "fm_self_dist is the L2 call" in err()
        assert lib.fm_hamming_set_selfdist(h, l2.handle, _ffi._ptr(out)) == EINVAL and "fm_bank_set_selfdist is the L2 call" in err()
        hs = (ctypes.c_void_p * 2)(qb.handle, l2.handle)
        assert lib.fm_hamming_self_dist_batch(h, 2, hs, None) == EINVAL and "fm_self_dist_batch is the L2 call" in err()
        # 3. widths -- in front of the self distances (narrow has none)
        for name, rc, msg in pair_calls(narrow, tb, cap=-1, null_out=True):
            assert rc == EINVAL and "width" in msg, (name, msg)
        # 4. no self distances -- in front of cap and the outputs
        for name, rc, msg in pair_calls(bare, tb, cap=-1, null_out=True):
            assert rc == EINVAL and "no self distances" in msg, (name, msg)
        assert lib.fm_hamming_match_accepted_dev(h, bare.handle, tb.handle, 0.9, -1, None, None, None) == EINVAL and "no self distances" in err()
        # 5. cap, then the outputs
        name, rc, msg = pair_calls(qb, tb, cap=-1, null_out=True)[1]
        assert rc == EINVAL and "cap < 0" in msg
        for name, rc, msg in pair_calls(qb, tb, cap=4, null_out=True):
            assert rc == EINVAL and "NULL" in msg, (name, msg)
        assert lib.fm_hamming_match_accepted_dev(h, qb.handle, tb.handle, 0.9, -1, None, None, None) == EINVAL and "cap < 0" in err()
        assert lib.fm_hamming_match_accepted_dev(h, qb.handle, tb.handle, 0.9, 4, None, None, None) == EINVAL and "NULL" in err()
        host = np.zeros((4, 3), np.int32)
        assert lib.fm_hamming_match_accepted_dev(h, qb.handle, tb.handle, 0.9, 4, _ffi._ptr(host), _ffi._ptr(host), None) == EINVAL
        assert "device memory" in err()
        # the collection forms: handles / another context, kinds, width, self distances, cap
        n4 = np.zeros(4, np.int64)
        f = lib.fm_collection_hamming_match_accepted_each
        assert f(h, None, qb.handle, 0.9, 0, None, None, None, None, _ffi._ptr(n4)) == EINVAL
        assert f(h, coll.handle, None, 0.9, 0, None, None, None, None, _ffi._ptr(n4)) == EINVAL
        other = fastmatch_amd.Context(0)
        try:
            assert f(other.handle, coll.handle, qb.handle, 0.9, 0, None, None, None, None, _ffi._ptr(n4)) == EINVAL
            assert "another context" in other.lib.fm_last_error(other.handle).decode()
        finally:
            other.close()
        assert f(h, coll.handle, l2.handle, 0.9, -1, None, None, None, None, None) == EINVAL
        assert "fm_collection_match_accepted_each is the L2 call" in err()
        with ctx.collection() as c8:
            c8.add(rng.integers(0, 256, (30, 128), dtype=np.uint8))
            assert f(h, c8.handle, qb.handle, 0.9, -1, None, None, None, None, None) == EINVAL and "is the L2 call" in err()
            g = lib.fm_collection_hamming_match_accepted_each_dev
            assert g(h, c8.handle, qb.handle, 0.9, -1, None, None, None, None) == EINVAL
            assert "fm_collection_match_accepted_each_dev is the L2 call" in err()
        assert f(h, coll.handle, narrow.handle, 0.9, -1, None, None, None, None, None) == EINVAL and "width" in err()
        assert f(h, coll.handle, bare.handle, 0.9, -1, None, None, None, None, None) == EINVAL and "no self distances" in err()
        assert f(h, coll.handle, qb.handle, 0.9, -1, None, None, None, None, None) == EINVAL and "cap < 0" in err()
        assert f(h, coll.handle, qb.handle, 0.9, 4, None, None, None, None, None) == EINVAL and "NULL" in err()
        # an empty collection is valid, whatever it will hold
        with ctx.collection() as c0:
            assert c0.hamming_match_accepted_each(qb, 0.9) == []
    finally:
        for b in (l2, narrow, bare, tb):
            b.close()


def test_l2_named_calls_still_refuse_binary_banks(ctx, gallery):
    """Restates (and does not replace) what tests/test_hamming_gpu.py and tests/test_collection_accepted_gpu.py assert."""
    Q, sd, qb, images, coll = gallery
    tb = ctx.bank_binary(images[0])
    try:
        for call in (lambda: ctx.self_dist(qb), lambda: ctx.self_dist_batch([qb]), lambda: qb.set_selfdist(sd),
                     lambda: ctx.match_ratio(qb, tb, 0.9), lambda: ctx.match_accepted(qb, tb, 0.9),
                     lambda: ctx.match_accepted_dev(qb, tb, 0.9, 0, 0, 4), lambda: coll.match_accepted_each(qb, 0.9)):
            with pytest.raises(fastmatch_amd.FastMatchHipError) as e:
                call()
            assert e.value.code == EUNSUPPORTED and "hamming" in str(e.value)
        # ... and nothing was disturbed
        assert _same(ctx.hamming_self_dist(qb), sd)
    finally:
        tb.close()
