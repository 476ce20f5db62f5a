"""GPU: image pairs inside a train collection (fm_collection_pairs_mutual_ratio, its device form, Collection.pairs_mutual_ratio,
torchmatch.Collection.match_pairs, BFMatcher.matchPairs): pair (a, b) equals Context.mutual_ratio(bank(image a), bank(image
b)), bit for bit, on every kind, and the NumPy reference (tests/pairs_ref.py) on the kinds whose arithmetic the reference
restates exactly (uint8, integer-valued float32, binary: mutual_ratio_ref sums float32 rows in another order than the float32
route, as in the sibling collection tests)."""
import os
import sys

import numpy as np
import pytest

from fastmatch_amd import _ffi, matchutil, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f32_regimes                              # noqa: E402
import pairs_ref as ref                         # noqa: E402
from kat import far_banks, SQRT_TIE_MIN         # noqa: E402

pytestmark = pytest.mark.gpu

EINVAL = -1
INF = float("inf")
BOUNDARY_SIZES = [0, 1, 127, 128, 129, 1000, 5, 0]
LISTED = [(5, 5), (2, 3), (3, 2), (2, 3), (0, 7), (7, 0), (1, 1)]
KINDS = ("u8", "f32int", "f32", "f32nofilter", "bin1", "bin32", "bin64")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want, what):
    assert np.array_equal(got[0], want[0]), what + ": rows of a"
    assert np.array_equal(got[1], want[1]), what + ": rows of b"
    assert np.array_equal(_bits(got[2]), _bits(want[2])), what + ": distances"
    assert np.array_equal(np.asarray(got[3]).view(np.uint64), np.asarray(want[3]).view(np.uint64)), what + ": ratios"


def _plant(images, noisy):
    """Every third row of each image of two rows or more is a noisy view of a row of the largest image (the same rows in every
    image, so all of them share content), every fifteenth row of the largest a second view of a row of its own, and one row is
    present twice in the largest image and once more in another: mutual matches, shared first neighbours and failed reverse
    ratios exist between the images."""
    big = images[5]
    for j in range(1, big.shape[0], 15):
        big[j] = noisy(big[(j * 11 + 4) % big.shape[0]])
    big[7] = big[3]
    for i, im in enumerate(images):
        if i == 5 or im.shape[0] < 2:
            continue
        for j in range(0, im.shape[0], 3):
            im[j] = noisy(big[(j * 7) % big.shape[0]])
    images[4][1] = big[3]


def _data(kind, sizes=BOUNDARY_SIZES):
    """(images, binary, float_route) of a kind; deterministic."""
    rng = np.random.default_rng(5100 + KINDS.index(kind))
    if kind.startswith("bin"):
        w = int(kind[3:])
        images = [rng.integers(0, 256, (n, w), dtype=np.uint8) for n in sizes]

        def noisy(row):
            out = row.copy()
            out[rng.integers(0, w)] ^= np.uint8(1 << rng.integers(0, 8))
            return out
        _plant(images, noisy)
        return images, True, False
    if kind in ("u8", "f32int"):
        images = [synth.synth_sift(max(n, 1), rng)[:n].copy() for n in sizes]
        _plant(images, lambda row: np.clip(row.astype(np.int32) + rng.integers(-3, 4, row.shape), 0, 255).astype(np.uint8))
        if kind == "f32int":
            images = [im.astype(np.float32) for im in images]
        return images, False, False
    images = [f32_regimes._gauss(5200 + i, n).astype(np.float32) for i, n in enumerate(sizes)]
    _plant(images, lambda row: (row + rng.normal(0.0, 0.01, row.shape)).astype(np.float32))
    if kind == "f32nofilter":
        images[2] = f32_regimes.qt_apart(45)[0][:127].copy()     # leaves fp16's range under the collection's scale: no filter
    return images, False, True


def _bank(ctx, a, binary, float_route):
    return ctx.bank_binary(a) if binary else ctx.bank(a, float_route=float_route)


def _collection(ctx, images, binary):
    c = ctx.collection()
    for i, im in enumerate(images):
        assert (c.add_binary(im) if binary else c.add(im)) == i
    return c


def _loop(ctx, banks, pairs, tau, sym):
    """The pair calls the match graph replaces: Context.mutual_ratio on banks made from the same arrays."""
    return [ctx.mutual_ratio(banks[a], banks[b], tau, sym) for a, b in pairs]


def _exact_for_the_reference(kind, images):
    if kind in ("f32", "f32nofilter"):
        return None
    return [im.astype(np.uint8) for im in images] if kind == "f32int" else images


@pytest.mark.parametrize("kind", KINDS)
def test_every_pair_equals_the_pair_call(ctx, kind):
    images, binary, float_route = _data(kind)
    coll = _collection(ctx, images, binary)
    banks = [_bank(ctx, im, binary, float_route) for im in images]
    exact = _exact_for_the_reference(kind, images)
    try:
        ctx.set_option("f32_filter", 2 if kind in ("f32", "f32nofilter") else 1)
        assert coll.info()[3] == (_ffi.FM_BANK_BIN if binary else _ffi.FM_BANK_F32 if float_route else _ffi.FM_BANK_I8)
        accepted = 0
        for pairs in (None, LISTED):
            plist = ref.all_pairs(len(images)) if pairs is None else pairs
            assert len(plist) == (28 if pairs is None else 7)
            for tau in (0.8, INF):
                for sym in (False, True):
                    got = coll.pairs_mutual_ratio(pairs, tau, sym)
                    want = _loop(ctx, banks, plist, tau, sym)
                    assert len(got) == len(plist)
                    for p, ab in enumerate(plist):
                        _same(got[p], want[p], "%s tau=%s sym=%d pair %s against the pair call" % (kind, tau, sym, ab))
                    if exact is not None:
                        r = ref.pairs_mutual_ratio(exact, plist, tau, sym, binary)
                        for p, ab in enumerate(plist):
                            _same(got[p], r[p], "%s tau=%s sym=%d pair %s against the reference" % (kind, tau, sym, ab))
                    counts = coll.pairs_mutual_ratio_counts(pairs, tau, sym)
                    assert np.diff(counts).tolist() == [g[0].shape[0] for g in got] and counts[0] == 0
                    for p, (a, b) in enumerate(plist):
                        if min(images[a].shape[0], images[b].shape[0]) == 0:
                            assert got[p][0].shape[0] == 0                           # empty images accept nothing
                    if pairs is LISTED:
                        _same(got[1], got[3], "a pair listed twice")
                        assert got[0][0].tolist() == got[0][1].tolist()              # (5, 5): a row matches itself or an earlier twin
                    accepted += sum(g[0].shape[0] for g in got)
        if kind != "bin1":
            assert coll.pairs_mutual_ratio([(4, 5), (3, 4)], 0.8)[0][0].shape[0] >= 10    # the planted views are found
        assert accepted > 0
    finally:
        ctx.set_option("f32_filter", 1)
        for b in banks:
            b.close()
        coll.close()


@pytest.mark.parametrize("kind", ("u8", "bin32"))
def test_more_slots_than_any_argument_struct_holds(ctx, kind):
    """48 images of 1 .. 40 rows, exhaustive: 1 128 pairs, 2 256 sweeps -- beyond the 16 of a batched launch and beyond 1 024,
    so the search over the prefix array has depth."""
    sizes = [1 + (i * 7) % 40 for i in range(48)]
    rng = np.random.default_rng(5300 + len(kind))
    binary = kind == "bin32"
    base = rng.integers(0, 256, (40, 32), dtype=np.uint8) if binary else synth.synth_sift(40, rng)
    images = []
    for n in sizes:
        im = base[rng.permutation(40)[:n]].copy()                  # shared rows, slightly perturbed: matches between all images
        if binary:
            im[:, 0] ^= rng.integers(0, 2, n, dtype=np.uint8)
        else:
            im[:, :8] = np.clip(im[:, :8].astype(np.int32) + rng.integers(-2, 3, (n, 8)), 0, 255).astype(np.uint8)
        images.append(im)
    assert sorted(set(sizes)) == list(range(1, 41))
    coll = _collection(ctx, images, binary)
    banks = [_bank(ctx, im, binary, False) for im in images]
    try:
        plist = ref.all_pairs(48)
        assert len(plist) == 1128
        got = coll.pairs_mutual_ratio(None, 0.8, True)
        want = _loop(ctx, banks, plist, 0.8, True)
        r = ref.pairs_mutual_ratio(images, None, 0.8, True, binary)
        for p, ab in enumerate(plist):
            _same(got[p], want[p], "%s pair %s against the pair call" % (kind, ab))
            _same(got[p], r[p], "%s pair %s against the reference" % (kind, ab))
        assert sum(g[0].shape[0] for g in got) >= 1128
    finally:
        for b in banks:
            b.close()
        coll.close()


def test_few_large_pairs_take_split_sweeps_with_shared_bounds(ctx):
    """A call of few pairs keeps the planner's splits: images of 16 stages and more are swept in two splits per slot, with the
    shared bounds of the "coop" option in the chunk's workspace (the other tests' images are too small for a second split)."""
    rng = np.random.default_rng(5350)
    base = synth.synth_sift(2304, rng)
    images = [base.copy(), synth.synth_sift(2100, rng), synth.synth_sift(300, rng)]
    images[1][::2] = np.clip(base[:2100:2].astype(np.int32) + rng.integers(-3, 4, (1050, 128)), 0, 255).astype(np.uint8)
    images[2][:100] = base[2200:2300]
    pairs = [(0, 1), (1, 0), (0, 0), (2, 0), (0, 2)]
    coll = _collection(ctx, images, False)
    banks = [ctx.bank(im) for im in images]
    before = ctx.get_option("coop")
    try:
        want = ref.pairs_mutual_ratio(images, pairs, 0.8, True)
        assert want[0][0].shape[0] >= 900 and want[3][0].shape[0] >= 90
        for coop in (1, 0):
            ctx.set_option("coop", coop)
            for tau, sym in ((0.8, True), (INF, False)):
                got = coll.pairs_mutual_ratio(pairs, tau, sym)
                loop = _loop(ctx, banks, pairs, tau, sym)
                for p, ab in enumerate(pairs):
                    _same(got[p], loop[p], "coop=%d tau=%s pair %s against the pair call" % (coop, tau, ab))
                    if tau == 0.8:
                        _same(got[p], want[p], "coop=%d pair %s against the reference" % (coop, ab))
    finally:
        ctx.set_option("coop", before)
        for b in banks:
            b.close()
        coll.close()


@pytest.mark.parametrize("kind", ("u8", "f32", "bin32"))
def test_chunks_do_not_change_the_result(ctx, kind):
    images, binary, float_route = _data(kind)
    coll = _collection(ctx, images, binary)
    try:
        before = ctx.get_option("coll_ws_bytes")
        want_all, off_all = coll.pairs_mutual_ratio(None, INF, True), coll.pairs_mutual_ratio_counts(None, INF, True)
        want_l, off_l = coll.pairs_mutual_ratio(LISTED, 0.8, False), coll.pairs_mutual_ratio_counts(LISTED, 0.8, False)
        assert off_all[-1] > 0 and off_l[-1] > 0
        for budget in (1, 1 << 20):                        # one pair per chunk; a middle value: several small pairs per chunk
            ctx.set_option("coll_ws_bytes", budget)
            for pairs, want, off in ((None, want_all, off_all), (LISTED, want_l, off_l)):
                tau, sym = (INF, True) if pairs is None else (0.8, False)
                got = coll.pairs_mutual_ratio(pairs, tau, sym)
                assert np.array_equal(coll.pairs_mutual_ratio_counts(pairs, tau, sym), off)
                for p in range(len(want)):
                    _same(got[p], want[p], "%s budget %d pair %d" % (kind, budget, p))
        ctx.set_option("coll_ws_bytes", before)
        assert ctx.get_option("coll_ws_bytes") == before
    finally:
        ctx.set_option("coll_ws_bytes", 0)
        coll.close()


def test_float32_root_ties_in_two_images_of_four(ctx):
    rng = np.random.default_rng(5400)
    Q, far = far_banks(300, 500, rng)
    near0 = np.zeros((400, 128), np.uint8)
    near0[:, 101:111] = rng.integers(0, 3, (400, 10), dtype=np.uint8)
    near1 = near0[::-1][:129].copy()
    images = [near0, far, Q, near1]
    assert int((far.astype(np.int64) ** 2).sum(1).max()) >= SQRT_TIE_MIN
    coll = _collection(ctx, images, False)
    banks = [ctx.bank(im) for im in images]
    try:
        for pairs in (None, [(2, 1), (1, 2), (1, 1)]):
            plist = ref.all_pairs(4) if pairs is None else pairs
            for sym in (False, True):
                got = coll.pairs_mutual_ratio(pairs, INF, sym)
                want = ref.pairs_mutual_ratio(images, plist, INF, sym)
                loop = _loop(ctx, banks, plist, INF, sym)
                for p, ab in enumerate(plist):
                    _same(got[p], want[p], "pair %s sym=%d against the reference" % (ab, sym))
                    _same(got[p], loop[p], "pair %s sym=%d against the pair call" % (ab, sym))
        assert coll.pairs_mutual_ratio([(2, 1)], INF)[0][0].shape[0] > 0
    finally:
        for b in banks:
            b.close()
        coll.close()


def _raw(ctx, coll, pairs, tau, sym, cap, fill=-7):
    """The C call into sentinel-filled arrays: (rc, offsets, qidx, tidx, dist, ratio, n_total)."""
    import ctypes
    arr = None if pairs is None else _ffi.pairs_array(pairs)
    ni = coll.info()[0]
    n = ni * (ni - 1) // 2 if pairs is None else arr.shape[0]
    kept = max(cap, 0)
    offsets = np.full(n + 1, fill, np.int64)
    q, t = np.full(kept, fill, np.int32), np.full(kept, fill, np.int32)
    d, r = np.full(kept, fill, np.float32), np.full(kept, fill, np.float64)
    total = ctypes.c_int64(fill)
    rc = ctx.lib.fm_collection_pairs_mutual_ratio(ctx.handle, coll.handle, _ffi._ptr(arr), n, tau, int(sym), cap, _ffi._ptr(offsets),
                                                  _ffi._ptr(q) if kept else None, _ffi._ptr(t) if kept else None,
                                                  _ffi._ptr(d) if kept else None, _ffi._ptr(r) if kept else None, ctypes.byref(total))
    return rc, offsets, q, t, d, r, total.value


@pytest.mark.parametrize("kind", ("u8", "bin32"))
def test_the_packed_output(ctx, kind):
    images, binary, float_route = _data(kind)
    coll = _collection(ctx, images, binary)
    try:
        plist = ref.all_pairs(len(images))
        per = ref.pairs_mutual_ratio(images, plist, 0.8, True, binary)
        offsets, total, cols = ref.pack(per, 1 << 40)
        assert total > 0
        counts = np.diff(offsets)
        mid = [p for p in range(5, len(plist) - 1) if counts[p] > 0 and offsets[p] > 0 and offsets[p + 1] < total][0]
        for cap in (0, total, total + 5, int(offsets[mid + 1]) - 1, int(offsets[mid])):
            want_off, rows, want = ref.pack(per, cap)
            rc, off, q, t, d, r, n_total = _raw(ctx, coll, None, 0.8, True, cap)
            assert rc == 0 and n_total == total and off.tolist() == offsets.tolist() == want_off.tolist()
            _same((q[:rows], t[:rows], d[:rows], r[:rows]), want, "%s cap=%d" % (kind, cap))
            # the later rows are untouched: the longest prefix of WHOLE pairs
            assert (q[rows:] == -7).all() and (t[rows:] == -7).all() and (d[rows:] == -7).all() and (r[rows:] == -7).all()
        assert ref.pack(per, int(offsets[mid + 1]) - 1)[1] == offsets[mid]          # one short of the end of pair `mid`: it is left out
        assert _raw(ctx, coll, None, 0.8, True, -1)[0] == EINVAL
        assert np.array_equal(coll.pairs_mutual_ratio_counts(None, 0.8, True), offsets)
        # Collection.pairs_mutual_ratio with a cap: the pairs behind the prefix come back empty
        got = coll.pairs_mutual_ratio(None, 0.8, True, cap=int(offsets[mid + 1]) - 1)
        for p in range(len(plist)):
            if p < mid:
                _same(got[p], per[p], "capped, pair %d" % p)
            else:
                assert got[p][0].shape[0] == 0
    finally:
        coll.close()


@pytest.mark.parametrize("kind", ("u8", "f32"))
def test_options_do_not_change_the_result(ctx, kind):
    images, binary, float_route = _data(kind)
    coll = _collection(ctx, images, binary)
    defaults = {name: ctx.get_option(name) for name in ("batch_group", "coop", "glds", "f32_filter")}
    try:
        want = coll.pairs_mutual_ratio(LISTED + [(5, 4), (2, 5)], INF, True)
        assert sum(w[0].shape[0] for w in want) > 0
        for name, values in (("batch_group", (1, 16)), ("coop", (0,)), ("glds", (0,)), ("f32_filter", (0, 2))):
            for v in values:
                ctx.set_option(name, v)
                got = coll.pairs_mutual_ratio(LISTED + [(5, 4), (2, 5)], INF, True)
                for p in range(len(want)):
                    _same(got[p], want[p], "%s %s=%d pair %d" % (kind, name, v, p))
            ctx.set_option(name, defaults[name])
    finally:
        for name, v in defaults.items():
            ctx.set_option(name, v)
        coll.close()


def test_refusals_in_order(ctx):
    import ctypes
    rng = np.random.default_rng(5600)
    coll = _collection(ctx, [synth.synth_sift(200, rng), synth.synth_sift(100, rng), synth.synth_sift(50, rng)], False)
    other = _ffi.Context(0)
    foreign = other.collection()
    lib, h = ctx.lib, ctx.handle
    f = lib.fm_collection_pairs_mutual_ratio
    off = np.zeros(8, np.int64)
    a = [_ffi._ptr(np.zeros(500, t)) for t in (np.int32, np.int32, np.float32, np.float64)]
    ok, bad = _ffi.pairs_array([(0, 1), (2, 0)]), _ffi.pairs_array([(0, 1), (3, 0)])
    neg = _ffi.pairs_array([(0, -1)])
    P = _ffi._ptr

    def err():
        return lib.fm_last_error(h).decode()
    try:
        # 1. the handles (everything behind them wrong as well)
        assert f(None, coll.handle, P(bad), -1, 0.8, 0, -1, None, None, None, None, None, None) == EINVAL
        assert f(h, None, P(bad), -1, 0.8, 0, -1, None, None, None, None, None, None) == EINVAL
        assert f(h, foreign.handle, P(bad), -1, 0.8, 0, -1, None, None, None, None, None, None) == EINVAL
        assert "another context" in err()
        # 2. the number of pairs
        assert f(h, coll.handle, P(bad), -1, 0.8, 0, -1, None, None, None, None, None, None) == EINVAL and "n_pairs" in err()
        for n in (0, 2, 4):
            assert f(h, coll.handle, None, n, 0.8, 0, -1, None, None, None, None, None, None) == EINVAL and "n_images" in err()
        # 3. the image indices; nothing is enqueued
        ctx.sync()
        before = ctx.stats()
        assert f(h, coll.handle, P(bad), 2, 0.8, 0, -1, None, None, None, None, None, None) == EINVAL and "outside" in err()
        assert f(h, coll.handle, P(neg), 1, 0.8, 0, 500, P(off), *a, None) == EINVAL and "outside" in err()
        assert ctx.stats() == before
        # 4. the outputs
        assert f(h, coll.handle, P(ok), 2, 0.8, 0, -1, None, None, None, None, None, None) == EINVAL and "cap" in err()
        assert f(h, coll.handle, P(ok), 2, 0.8, 0, 500, None, *a, None) == EINVAL and "offsets" in err()
        assert f(h, coll.handle, P(ok), 2, 0.8, 0, 500, P(off), a[0], None, a[2], a[3], None) == EINVAL
        assert f(h, coll.handle, P(ok), 2, 0.8, 0, 500, P(off), a[0], a[1], a[2], None, None) == EINVAL
        assert ctx.stats() == before
        # valid: no pairs, counts only without row arrays, every pair by NULL, an empty collection
        off[:] = -7
        assert f(h, coll.handle, P(ok), 0, 0.8, 0, 0, P(off), None, None, None, None, None) == 0 and off[0] == 0 and off[1] == -7
        total = ctypes.c_int64(-7)
        assert f(h, coll.handle, P(ok), 2, INF, 0, 0, P(off), None, None, None, None, ctypes.byref(total)) == 0
        assert off[0] == 0 and off[2] == total.value > 0 and off[3] == -7
        assert f(h, coll.handle, None, 3, INF, 0, 0, P(off), None, None, None, None, None) == 0 and off[3] > 0
        after = ctx.stats()
        assert after["pairs"] - before["pairs"] == 2 * (200 * 100 + 50 * 200) + 2 * (200 * 100 + 200 * 50 + 100 * 50)
        empty = ctx.collection()
        assert f(h, empty.handle, None, 0, 0.8, 0, 0, P(off), None, None, None, None, ctypes.byref(total)) == 0 and total.value == 0
        assert f(h, empty.handle, None, 1, 0.8, 0, 0, P(off), None, None, None, None, None) == EINVAL
        assert f(h, empty.handle, P(ok), 2, 0.8, 0, 0, P(off), None, None, None, None, None) == EINVAL and "outside" in err()
        assert empty.pairs_mutual_ratio() == [] and empty.pairs_mutual_ratio([]) == []
        empty.close()
        # the device form: the same order, then its pointers (host memory is refused)
        g = lib.fm_collection_pairs_mutual_ratio_dev
        NOS = _ffi._stream_arg(None)
        assert g(h, coll.handle, P(bad), -1, 0.8, 0, -1, None, None, None, NOS) == EINVAL and "n_pairs" in err()
        assert g(h, coll.handle, P(bad), 2, 0.8, 0, -1, None, None, None, NOS) == EINVAL and "outside" in err()
        assert g(h, coll.handle, P(ok), 2, 0.8, 0, -1, None, None, None, NOS) == EINVAL and "cap" in err()
        assert g(h, coll.handle, P(ok), 2, 0.8, 0, 10, None, None, None, NOS) == EINVAL and "d_offsets" in err()
        assert g(h, coll.handle, P(ok), 2, 0.8, 0, 10, P(off), a[0], None, NOS) == EINVAL                  # host memory
    finally:
        foreign.close()
        other.close()
        coll.close()


@pytest.mark.parametrize("kind", ("u8", "f32", "bin32"))
def test_device_form_equals_the_host_form(ctx, kind):
    import torch
    from fastmatch_amd import torchmatch
    images, binary, float_route = _data(kind)
    coll = _collection(ctx, images, binary)
    try:
        for pairs, tau, sym in ((None, 0.8, True), (LISTED, INF, False), ([(2, 3)], 0.0, False)):
            want = coll.pairs_mutual_ratio(pairs, tau, sym)
            offsets = coll.pairs_mutual_ratio_counts(pairs, tau, sym)
            total, n = int(offsets[-1]), len(want)
            mid = int(offsets[n // 2 + 1]) - 1 if n > 2 else 0
            for cap in (total + 3, max(mid, 0), 0):
                side = torch.cuda.Stream()
                with torch.cuda.stream(side):
                    # (work on the side stream in front of the call: the fills below must not be overtaken)
                    busy = torch.ones(1 << 22, device="cuda").cumsum(0)
                    rows = torch.full((cap, 3), -7, dtype=torch.int32, device="cuda")
                    d_off = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
                    got_total = coll.pairs_mutual_ratio_dev(pairs, tau, sym, d_off.data_ptr(), rows.data_ptr() if cap else 0, cap,
                                                            want_total=True, consumer_stream=side.cuda_stream)
                    h_off, got = d_off.cpu().numpy(), rows.cpu().numpy()
                side.synchronize()
                assert float(busy[-1]) == float(1 << 22)
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
                assert at == whole and (got[whole:] == -7).all()
        # torchmatch: a collection fed from tensors on a non-default current stream; cap None (counts, then one fill) and a cap
        side = torch.cuda.Stream()
        with torch.cuda.stream(side), torchmatch.Collection(context=ctx) as tc:
            for im in images:
                tc.add(torch.from_numpy(im).cuda(), binary=binary)
            want = coll.pairs_mutual_ratio(LISTED, 0.8, True)
            packed = ref.pack(want, 1 << 40)
            for pairs in (LISTED, torch.tensor(LISTED, dtype=torch.int32)):
                for cap in (None, packed[1] + 4):
                    offsets, rows = tc.match_pairs(pairs, 0.8, symmetric=True, cap=cap)
                    assert offsets.dtype == torch.int64 and rows.dtype == torch.int32
                    assert rows.shape == (packed[1] if cap is None else cap, 3)
                    assert offsets.cpu().numpy().tolist() == packed[0].tolist()
                    got = rows.cpu().numpy()[:packed[1]]
                    assert np.array_equal(got[:, 0], packed[2][0]) and np.array_equal(got[:, 1], packed[2][1])
                    assert np.array_equal(got[:, 2].view(np.uint32), _bits(packed[2][2]))
            offsets, rows = tc.match_pairs(tau=0.8)
            assert offsets.shape == (29,) and offsets.cpu().numpy().tolist() == coll.pairs_mutual_ratio_counts(None, 0.8).tolist()
        side.synchronize()
    finally:
        coll.close()


@pytest.mark.parametrize("norm", ("l2", "hamming"))
def test_bfmatcher_match_pairs(ctx, norm):
    rng = np.random.default_rng(5700)
    if norm == "l2":
        base = synth.synth_sift(300, rng)
        images = [np.clip(base[rng.permutation(300)[:n]].astype(np.int32) + rng.integers(-3, 4, (n, 128)), 0, 255).astype(np.uint8)
                  for n in (200, 150, 0, 257)]
        m = matchutil.BFMatcher(matchutil.NORM_L2)
    else:                                                  # ORB-like: 32-byte rows, a few flipped bits per view
        base = rng.integers(0, 256, (300, 32), dtype=np.uint8)
        images = []
        for n in (200, 150, 0, 257):
            im = base[rng.permutation(300)[:n]].copy()
            im[np.arange(n), rng.integers(0, 32, n)] ^= np.uint8(4)
            images.append(im)
        m = matchutil.BFMatcher(matchutil.NORM_HAMMING)
    m.add(images)
    opts = {"normType": m.normType}
    for pairs in (None, [(3, 0), (0, 3), (1, 1), (2, 0), (3, 0)]):
        plist = ref.all_pairs(4) if pairs is None else pairs
        for sym in (False, True):
            got = m.matchPairs(pairs, ratio=0.8, symmetric=sym)
            arr, lists = m.matchPairs_arrays(pairs, 0.8, sym)
            assert arr.tolist() == [list(ab) for ab in plist] and set(got) == set(plist)
            for p, (a, b) in enumerate(plist):
                want = matchutil.mutual_ratio_match_arrays(images[a], images[b], 0.8, symmetric=sym, options=opts)
                _same(lists[p], want, "%s pair (%d, %d) sym=%d" % (norm, a, b, sym))
                assert [(d.queryIdx, d.trainIdx, d.imgIdx) for d in got[(a, b)]] == \
                       [(int(q), int(t), b) for q, t in zip(want[0], want[1])]
                assert [np.float32(d.distance) for d in got[(a, b)]] == want[2].tolist()
    assert sum(len(v) for v in m.matchPairs().values()) >= 100
