"""GPU: train collections fed from device memory (fm_collection_add_dev) and stacked results left there (fm_collection_knn_dev,
fm_collection_knn2_ratio_dev), with ``torchmatch.Collection`` on top.

The yardstick is the HOST-ADDED collection of the same values -- the paths test_collection_gpu.py and
test_collection_accepted_gpu.py check against the CPU oracle -- and every comparison is np.array_equal on the raw bits: a
device-added collection must be indistinguishable from its host twin through every fm_collection_* call.  One case per kind is
also checked directly against the oracle / tests/hamming_ref.py on the stacked rows."""
import ctypes

import numpy as np
import pytest

import fastmatch_amd
import oracle
from fastmatch_amd import _ffi, synth

import hamming_ref as H

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 127, 128, 129, 1000, 0, 4099]      # empty first / middle / last-but-one, a stage boundary and one past it, growth past 4096 rows
NQ = 300
EINVAL, EUNSUP = -1, -4
# (name, element type of the source, values, width)
CASES = [("u8", "u8", "int", 128), ("u8_61", "u8", "int", 61), ("f32_int", "f32", "int", 128), ("f32", "f32", "normal", 128),
         ("f32_61", "f32", "normal", 61), ("f16", "f16", "normal", 128), ("bf16", "bf16", "normal", 128),
         ("bin32", "bin", "bits", 32), ("bin7", "bin", "bits", 7)]


def _torch():
    import torch
    return torch


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same(a, b, what):
    assert len(a) == len(b), what
    for i, (x, y) in enumerate(zip(a, b)):
        x, y = np.asarray(x), np.asarray(y)
        assert x.shape == y.shape and x.dtype == y.dtype, "%s [%d]: %s %s / %s %s" % (what, i, x.shape, x.dtype, y.shape, y.dtype)
        assert np.array_equal(_bits(x), _bits(y)), "%s [%d]" % (what, i)


def _values(rng, elem, values, n, width):
    """The rows as a torch CPU tensor of the source's element type."""
    torch = _torch()
    if elem == "bin":
        return torch.from_numpy(rng.integers(0, 256, (n, width), dtype=np.uint8))
    if values == "int":
        a = synth.synth_sift(max(n, 1), rng)[:n, :width].copy()
        return torch.from_numpy(a if elem == "u8" else a.astype(np.float32))
    v = torch.from_numpy(rng.standard_normal((n, width)).astype(np.float32))
    return v.to({"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[elem])


def _host(t):
    """What the host add takes for the tensor's values: uint8 as it is, everything else as float32 (exact)."""
    torch = _torch()
    return t.numpy() if t.dtype == torch.uint8 else t.float().numpy()


def _dt_of(t, binary):
    torch = _torch()
    if binary:
        return _ffi.FM_DT_BIN
    return {torch.uint8: _ffi.FM_DT_U8, torch.float32: _ffi.FM_DT_F32, torch.float16: _ffi.FM_DT_F16, torch.bfloat16: _ffi.FM_DT_BF16}[t.dtype]


def _add_dev(coll, t, binary=False, stream=None):
    """fm_collection_add_dev of a CUDA tensor (rows stride(0) apart), behind the current torch stream."""
    torch = _torch()
    n, dim = t.shape
    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    return coll.add_from_device(t.data_ptr() if n else 0, _dt_of(t, binary), n, dim, t.stride(0) * t.element_size() if n > 1 else 0, stream=s)


def _add_host(coll, t, binary=False):
    return coll.add_binary(_host(t)) if binary else coll.add(_host(t))


def _case_data(name):
    """Images and query of a case as torch CPU tensors, made once per case; query rows planted in two images."""
    _, elem, values, width = next(c for c in CASES if c[0] == name)
    rng = np.random.default_rng(1000 + [c[0] for c in CASES].index(name))
    images = [_values(rng, elem, values, n, width) for n in SIZES]
    Q = _values(rng, elem, values, NQ, width)
    # rows 0 .. 9 of the 1000-row image are also rows 0 .. 9 of the 4099-row image: the query rows that copy them find both
    # at distance 0, and the earlier image has to win; some more copies from the 129-row image, a few one step away
    images[7][:10] = images[5][:10]
    Q[:10] = images[5][:10]
    Q[10:20] = images[4][100:110]
    Q[20:25] = images[7][4000:4005]
    if elem == "u8" or elem == "bin":
        Q[15:20, 0] ^= 1
    return images, Q, elem == "bin"


def _qbank(ctx, Q, coll, binary):
    if binary:
        return ctx.bank_binary(_host(Q))
    return ctx.bank(_host(Q), float_route=coll.info()[3] == _ffi.FM_BANK_F32)


def _outputs(ctx, coll, q, binary):
    """Everything the collection's entry points return for q."""
    out = [np.asarray(coll.info()), coll.image_rows()]
    for k in (1, 2, 5):
        out += list(coll.knn(q, k))
    out += list(coll.knn2_each(q))
    out += [coll.votes(q, 0.8, 0), coll.votes(q, 0.8, 1)]
    out += list(coll.knn2_ratio(q, 0.8))
    if not binary:
        if not q.has_selfdist:
            q.set_selfdist(ctx.self_dist(q))
        for rows in coll.match_accepted_each(q, 0.9):
            out += list(rows)
    return out


def _compare(ctx, dev, host, Q, binary, what):
    assert dev.info() == host.info(), what
    q = _qbank(ctx, Q, host, binary)
    try:
        _same(_outputs(ctx, dev, q, binary), _outputs(ctx, host, q, binary), what)
    finally:
        q.close()


# ---- parity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_device_added_collection_equals_the_host_added_one(ctx, name):
    images, Q, binary = _case_data(name)
    with ctx.collection() as dev, ctx.collection() as host:
        for i, im in enumerate(images):
            assert _add_dev(dev, im.cuda(), binary) == i == _add_host(host, im, binary)
        want_kind = _ffi.FM_BANK_BIN if binary else _ffi.FM_BANK_I8 if name in ("u8", "u8_61", "f32_int") else _ffi.FM_BANK_F32
        assert dev.info() == (len(SIZES), sum(SIZES), images[0].shape[1], want_kind)
        _compare(ctx, dev, host, Q, binary, name)
        if want_kind != _ffi.FM_BANK_F32:                        # exact integer distances: the planted ties went to the earlier image
            q = _qbank(ctx, Q, dev, binary)
            img, idx, dist = dev.knn(q, 2)
            assert (img[:10, 0] == 5).all() and (idx[:10, 0] == np.arange(10)).all() and (dist[:10, 0] == 0).all()
            assert (img[:10, 1] == 7).all() and (idx[:10, 1] == np.arange(10)).all() and (dist[:10, 1] == 0).all()
            q.close()


def _stacked_ref(kind, Q, images, k):
    dim = Q.shape[1]
    T = np.concatenate([im.reshape(-1, dim) for im in images])
    idx, dist = H.knn(Q, T, k) if kind == "bin" else oracle.bf_knn(Q, T, k, order=1 if kind == "f32" else 0)
    fr = np.concatenate([[0], np.cumsum([im.shape[0] for im in images])]).astype(np.int64)
    img = np.where(idx >= 0, np.searchsorted(fr, idx, side="right") - 1, -1).astype(np.int32)
    loc = np.where(idx >= 0, idx - fr[np.maximum(img, 0)], -1).astype(np.int32)
    return img, loc, dist


@pytest.mark.parametrize("kind", ["u8", "f32", "bin"])
def test_device_added_collection_against_the_oracle(ctx, kind):
    torch = _torch()
    rng = np.random.default_rng({"u8": 71, "f32": 72, "bin": 73}[kind])

    def rows(n):
        if kind == "bin":
            return rng.integers(0, 256, (n, 32), dtype=np.uint8)
        a = synth.synth_sift(max(n, 1), rng)[:n].copy()
        return a if kind == "u8" else (a + rng.uniform(-0.5, 0.5, a.shape)).astype(np.float32)

    images = [rows(n) for n in (0, 129, 1000, 0, 600)]
    Q = rows(NQ)
    Q[:8] = images[2][:8]
    with ctx.collection() as dev:
        for im in images:
            _add_dev(dev, torch.from_numpy(im).cuda(), kind == "bin")
        q = ctx.bank_binary(Q) if kind == "bin" else ctx.bank(Q)
        for k in (1, 2, 5):
            _same(dev.knn(q, k), _stacked_ref(kind, Q, images, k), "%s k=%d against the oracle" % (kind, k))
        q.close()


# ---- pitched sources ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,off,extra", [("u8", 16, 32), ("f32", 3, 12), ("bin32", 1, 8)])
def test_pitched_sources_are_read_in_place(ctx, name, off, extra):
    """[:, 16:144] of a uint8 tensor of width 160 (16-byte aligned rows: the vector path), [:, 3:131] of a float32 tensor of
    width 140 (element loads), [:, 1:33] of a uint8 tensor of width 40 as binary rows."""
    torch = _torch()
    images, Q, binary = _case_data(name)
    with ctx.collection() as dev, ctx.collection() as host:
        for im in images:
            n, w = im.shape
            wide = torch.full((n, w + extra), 77, dtype=im.dtype, device="cuda")
            assert wide.shape[1] == {"u8": 160, "f32": 140, "bin32": 40}[name]
            wide[:, off:off + w] = im.cuda()
            view = wide[:, off:off + w]
            assert n < 2 or (not view.is_contiguous() and view.stride(0) == w + extra)
            if name == "u8" and n:
                assert view.data_ptr() % 16 == 0 and (view.stride(0) * view.element_size()) % 16 == 0
            _add_dev(dev, view, binary)
            _add_host(host, im, binary)
        _compare(ctx, dev, host, Q, binary, "pitched " + name)


# ---- rebuild --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", ["device", "host"])
def test_rebuild_on_the_float32_route_with_alternating_adds(ctx, first):
    torch = _torch()
    rng = np.random.default_rng(81)
    ints = [torch.from_numpy(synth.synth_sift(n, rng).astype(np.float32)) for n in (200, 129, 1000)]
    frac = torch.from_numpy(rng.standard_normal((300, 128)).astype(np.float32) * 40).to(torch.float16)
    last = torch.from_numpy((synth.synth_sift(500, rng) + rng.uniform(-0.5, 0.5, (500, 128))).astype(np.float32))
    Q = torch.from_numpy((synth.synth_sift(NQ, rng) + rng.uniform(-0.5, 0.5, (NQ, 128))).astype(np.float32))
    Q[:10] = ints[2][:10]
    a, b = (_add_dev, _add_host) if first == "device" else (_add_host, _add_dev)

    def put(fn, coll, t):
        return fn(coll, t.cuda() if fn is _add_dev else t)

    with ctx.collection() as mixed, ctx.collection() as host:
        for im in ints:
            put(a, mixed, im); _add_host(host, im)
        assert mixed.info()[3] == _ffi.FM_BANK_I8 == host.info()[3]
        put(a, mixed, frac); _add_host(host, frac)                       # the first non-integer image: the rebuild
        assert mixed.info()[3] == _ffi.FM_BANK_F32 == host.info()[3]
        put(b, mixed, last); _add_host(host, last)                       # and one more image by the other add
        _compare(ctx, mixed, host, Q, False, "rebuild, %s adds first" % first)


# ---- the value limit ------------------------------------------------------------------------------------------------------
def test_value_limit_and_non_finite_values(ctx):
    torch = _torch()
    rng = np.random.default_rng(91)
    base = rng.standard_normal((400, 128)).astype(np.float32)
    Q = torch.from_numpy(rng.standard_normal((NQ, 128)).astype(np.float32))
    at = base[:200].copy(); at[7, 5] = np.float32(2.0 ** 57)
    above = base[:200].copy(); above[7, 5] = np.float32(2.0 ** 58)
    wild = base[:300].copy(); wild[3, 3] = np.inf; wild[9, 100] = np.nan; wild[11, 0] = -np.inf
    with ctx.collection() as dev, ctx.collection() as host:
        for im in (base, at):
            _add_dev(dev, torch.from_numpy(im).cuda()); host.add(im)     # exactly 2^57 is inside the limit
        q = ctx.bank(_host(Q), float_route=True)
        before = [np.asarray(dev.info()), dev.image_rows()] + list(dev.knn(q, 2))
        with pytest.raises(_ffi.FastMatchHipError) as e:
            _add_dev(dev, torch.from_numpy(above).cuda())
        assert e.value.code == EUNSUP
        with pytest.raises(_ffi.FastMatchHipError) as e:                 # (the host add refuses the same image)
            host.add(above)
        assert e.value.code == EUNSUP
        _same([np.asarray(dev.info()), dev.image_rows()] + list(dev.knn(q, 2)), before, "after the refused image")
        q.close()
        _add_dev(dev, torch.from_numpy(wild).cuda()); host.add(wild)     # inf and NaN are outside the limit's reach: filter off
        _compare(ctx, dev, host, Q, False, "2^57, inf and nan")
    # the refusal as the FIRST image of a collection leaves it empty and usable
    with ctx.collection() as dev, ctx.collection() as host:
        with pytest.raises(_ffi.FastMatchHipError) as e:
            _add_dev(dev, torch.from_numpy(above).cuda())
        assert e.value.code == EUNSUP and dev.info() == (0, 0, 0, 0)
        _add_dev(dev, torch.from_numpy(base).cuda()); host.add(base)
        _compare(ctx, dev, host, Q, False, "after a refused first image")


# ---- refusals -------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_collection_unchanged_and_usable(ctx):
    torch = _torch()
    lib, h, P = ctx.lib, ctx.handle, ctypes.c_void_p
    NOS = _ffi._stream_arg(None)
    rng = np.random.default_rng(101)
    U = synth.synth_sift(500, rng)
    F = rng.standard_normal((300, 128)).astype(np.float32)
    d = torch.zeros((64, 512), dtype=torch.uint8, device="cuda")
    hostmem = np.zeros((64, 128), np.uint8)
    out_i = torch.zeros((NQ, 8), dtype=torch.int32, device="cuda")
    out_j = torch.zeros((NQ, 8), dtype=torch.int32, device="cuda")
    out_f = torch.zeros((NQ, 8), dtype=torch.float32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    hout = np.zeros(NQ * 8, np.int32)
    torch.cuda.synchronize()
    with ctx.collection() as cu, ctx.collection() as cf, ctx.collection() as cb:
        _add_dev(cu, torch.from_numpy(U).cuda())
        _add_dev(cf, torch.from_numpy(F).cuda())
        _add_dev(cb, torch.from_numpy(U[:, :32].copy()).cuda(), True)
        qu, qf, qb = ctx.bank(U[:NQ]), ctx.bank(F[:NQ], float_route=True), ctx.bank_binary(U[:NQ, :32].copy())

        def state():
            return [np.asarray(c.info()) for c in (cu, cf, cb)] + [cu.image_rows()] + list(cu.knn(qu, 2)) + list(cf.knn(qf, 2)) + list(cb.knn(qb, 2))

        def add(c, ptr, dtype, n, dim, pitch):
            i = ctypes.c_int32(-7)
            rc = lib.fm_collection_add_dev(h, c.handle, P(ptr) if ptr else None, dtype, n, dim, pitch, NOS, ctypes.byref(i))
            assert rc == 0 or i.value == -7
            return rc

        ref = state()
        dp = d.data_ptr()
        pi, pj, pf, pc = P(out_i.data_ptr()), P(out_j.data_ptr()), P(out_f.data_ptr()), P(cnt.data_ptr())
        cases = [
            ("host pointer", lambda: add(cu, hostmem.ctypes.data, _ffi.FM_DT_U8, 64, 128, 0), EINVAL),
            ("NULL rows", lambda: add(cu, 0, _ffi.FM_DT_U8, 64, 128, 0), EINVAL),
            ("pitch below the row", lambda: add(cu, dp, _ffi.FM_DT_U8, 64, 128, 64), EINVAL),
            ("odd pitch for float16", lambda: add(cf, dp, _ffi.FM_DT_F16, 16, 128, 257), EINVAL),
            ("dtype 9", lambda: add(cu, dp, 9, 64, 128, 0), EINVAL),
            ("dtype 0", lambda: add(cu, dp, 0, 64, 128, 0), EINVAL),
            ("dim 129", lambda: add(cu, dp, _ffi.FM_DT_U8, 64, 129, 0), EUNSUP),
            ("65 binary bytes", lambda: add(cb, dp, _ffi.FM_DT_BIN, 64, 65, 0), EUNSUP),
            ("another width", lambda: add(cu, dp, _ffi.FM_DT_U8, 64, 64, 0), EINVAL),
            ("uint8 after float32", lambda: add(cf, dp, _ffi.FM_DT_U8, 64, 128, 0), EINVAL),
            ("binary after uint8", lambda: add(cu, dp, _ffi.FM_DT_BIN, 64, 128, 512), EUNSUP),      # (128 bytes: the width is refused first)
            ("binary after uint8, 32 bytes", lambda: add(cu, dp, _ffi.FM_DT_BIN, 64, 32, 0), EINVAL),
            ("uint8 after binary", lambda: add(cb, dp, _ffi.FM_DT_U8, 64, 32, 0), EINVAL),
            ("knn NULL img", lambda: lib.fm_collection_knn_dev(h, cu.handle, qu.handle, 2, None, pj, pf, NOS), EINVAL),
            ("knn NULL dist", lambda: lib.fm_collection_knn_dev(h, cu.handle, qu.handle, 2, pi, pj, None, NOS), EINVAL),
            ("knn host output", lambda: lib.fm_collection_knn_dev(h, cu.handle, qu.handle, 2, pi, P(hout.ctypes.data), pf, NOS), EINVAL),
            ("ratio NULL count", lambda: lib.fm_collection_knn2_ratio_dev(h, cu.handle, qu.handle, 0.8, NQ, pi, None, None, NOS), EINVAL),
            ("ratio NULL rows", lambda: lib.fm_collection_knn2_ratio_dev(h, cu.handle, qu.handle, 0.8, NQ, None, pc, None, NOS), EINVAL),
            ("ratio host rows", lambda: lib.fm_collection_knn2_ratio_dev(h, cu.handle, qu.handle, 0.8, NQ, P(hout.ctypes.data), pc, None, NOS), EINVAL),
            ("ratio host count", lambda: lib.fm_collection_knn2_ratio_dev(h, cu.handle, qu.handle, 0.8, NQ, pi, P(hout.ctypes.data), None, NOS), EINVAL),
            ("k = 0", lambda: lib.fm_collection_knn_dev(h, cu.handle, qu.handle, 0, pi, pj, pf, NOS), EINVAL),
            ("k = 9", lambda: lib.fm_collection_knn_dev(h, cu.handle, qu.handle, 9, pi, pj, pf, NOS), EUNSUP),
            ("query of another kind", lambda: lib.fm_collection_knn_dev(h, cu.handle, qb.handle, 2, pi, pj, pf, NOS), EINVAL),
        ]
        for name, call, want in cases:
            rc = call()
            assert rc == want, "%s: returned %d, expected %d" % (name, rc, want)
            msg = lib.fm_last_error(h)
            assert msg and len(msg.decode()) > 10, name
            _same(state(), ref, "collections after: " + name)
        # n = 0 is valid whatever the pointer, and takes an index
        assert cu.add_from_device(0, _ffi.FM_DT_U8, 0, 128) == 1
        assert cu.add_from_device(hostmem.ctypes.data, _ffi.FM_DT_U8, 0, 128) == 2
        assert cu.info()[:2] == (3, 500)
        for b in (qu, qf, qb):
            b.close()


# ---- device results -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["u8", "f32", "bin32"])
def test_device_results_equal_the_host_results(ctx, name):
    torch = _torch()
    images, Q, binary = _case_data(name)
    stream = torch.cuda.current_stream().cuda_stream
    with ctx.collection() as coll, ctx.collection() as empty:
        for im in images:
            _add_dev(coll, im.cuda(), binary)
        q = _qbank(ctx, Q, coll, binary)
        q0 = _qbank(ctx, Q[:0], coll, binary)
        q0_ok = q0.kind == coll.info()[3]           # (an empty float32 bank has the integer kind: a float32 collection refuses it)
        for c, what in ((coll, name), (empty, name + ", empty collection")):
            for k in (1, 2, 5):
                img = torch.full((NQ, k), -7, dtype=torch.int32, device="cuda")
                idx = torch.full((NQ, k), -7, dtype=torch.int32, device="cuda")
                dist = torch.full((NQ, k), -7.0, dtype=torch.float32, device="cuda")
                c.knn_dev(q, k, img.data_ptr(), idx.data_ptr(), dist.data_ptr(), consumer_stream=stream)
                got = (img.cpu().numpy(), idx.cpu().numpy(), dist.cpu().numpy())
                _same(got, c.knn(q, k), what + " knn k=%d" % k)
                if c is empty:
                    _same(got, (np.full((NQ, k), -1, np.int32), np.full((NQ, k), -1, np.int32), np.full((NQ, k), np.inf, np.float32)), what)
                if q0_ok or c is empty:
                    c.knn_dev(q0, k, 0, 0, 0, consumer_stream=stream)      # nq = 0: nothing is written, nothing is looked at
            hq, hm, ht, hd, _ = c.knn2_ratio(q, 0.8)
            m = hq.shape[0]
            assert (m > 10) == (c is coll), what
            for cap in (0, 3, NQ):
                rows = torch.full((max(cap, 1), 4), -7, dtype=torch.int32, device="cuda")
                count = torch.full((1,), -7, dtype=torch.int64, device="cuda")
                total = c.knn2_ratio_dev(q, 0.8, rows.data_ptr() if cap else 0, count.data_ptr(), cap, want_count=True, consumer_stream=stream)
                assert total == m, what
                n = int(count.item())
                assert n == min(m, cap), what
                r = rows.cpu().numpy()
                _same((r[:n, 0], r[:n, 1], r[:n, 2], r[:n, 3].copy().view(np.float32)), (hq[:n], hm[:n], ht[:n], hd[:n]), what + " ratio cap=%d" % cap)
                assert (r[n:] == -7).all(), what + ": rows past the count were written"
                count.fill_(-7)
                assert c.knn2_ratio_dev(q, 0.8, rows.data_ptr() if cap else 0, count.data_ptr(), cap, consumer_stream=stream) is None
                assert int(count.item()) == n
            if not (q0_ok or c is empty):
                continue
            count = torch.full((1,), -7, dtype=torch.int64, device="cuda")
            rows = torch.full((4, 4), -7, dtype=torch.int32, device="cuda")
            assert c.knn2_ratio_dev(q0, 0.8, rows.data_ptr(), count.data_ptr(), 4, want_count=True, consumer_stream=stream) == 0
            assert int(count.item()) == 0 and (rows.cpu().numpy() == -7).all()
        q.close(); q0.close()


# ---- streams --------------------------------------------------------------------------------------------------------------
def test_add_and_results_behind_a_side_stream_without_synchronize(ctx):
    from fastmatch_amd import torchmatch
    torch = _torch()
    g = torch.Generator(device="cuda").manual_seed(3)
    A = torch.randn(4096, 4096, device="cuda", generator=g)
    Qn = synth.synth_sift(NQ, np.random.default_rng(111))
    qb = ctx.bank(Qn)
    torch.cuda.synchronize()
    s1 = torch.cuda.Stream()
    with torchmatch.Collection(context=ctx) as coll:
        with torch.cuda.stream(s1):
            B = A
            for _ in range(12):                                    # tens of milliseconds of work in front of the descriptors
                B = torch.tanh(B @ A * 0.01)
            desc = ((B[:2000, :128] * 1.0e5).abs() % 256).floor().to(torch.uint8)     # exists only once the matmuls are done
            keep = desc.clone()
            assert coll.add(desc) == 0                             # producer = s1, no host synchronisation before it
            desc.zero_()                                           # the source is the caller's again
            img, idx, dist = coll.knn(qb, 2)                       # consumer = s1
            got = (img.clone(), idx.clone(), dist.clone())         # consumed on s1 with no host synchronisation
        s1.synchronize()
        K = keep.cpu().numpy()
        assert K.max() > 0 and len(np.unique(K)) > 50              # the descriptors were real
        assert int(desc.max().item()) == 0
        with ctx.collection() as host:
            host.add(K)
            _same([t.cpu().numpy() for t in got], host.knn(qb, 2), "knn behind the producer")
            _same(coll._coll.knn(qb, 2), host.knn(qb, 2), "collection after its source was zeroed")
    qb.close()


# ---- torchmatch.Collection ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["u8", "f16", "bin32"])
def test_torchmatch_collection_end_to_end(ctx, name):
    from fastmatch_amd import torchmatch
    torch = _torch()
    images, Q, binary = _case_data(name)
    with torchmatch.Collection(context=ctx) as tc, ctx.collection() as host:
        assert tc.info() == (0, 0, 0, 0)
        for i, im in enumerate(images):
            assert tc.add(im.cuda(), binary=binary) == i
            _add_host(host, im, binary)
        assert tc.info() == host.info()
        hb = _qbank(ctx, Q, host, binary)
        for q in (Q.cuda(), torchmatch.bank(Q.cuda(), binary=binary, float_route=name == "f16", context=ctx)):
            for k in (1, 2, 5):
                out = tc.knn(q, k)
                assert all(t.is_cuda and tuple(t.shape) == (NQ, k) for t in out)
                assert out[0].dtype == torch.int32 and out[1].dtype == torch.int32 and out[2].dtype == torch.float32
                _same([t.cpu().numpy() for t in out], host.knn(hb, k), "%s torchmatch knn k=%d" % (name, k))
            out = tc.ratio_match(q, 0.8)
            _same([t.cpu().numpy() for t in out], host.knn2_ratio(hb, 0.8)[:4], name + " torchmatch ratio_match")
            if isinstance(q, _ffi.Bank):
                if binary:
                    with pytest.raises(_ffi.FastMatchHipError) as e:
                        tc.fast_match_each(q, 0.9)
                    assert e.value.code == EUNSUP
                else:
                    with pytest.raises(_ffi.FastMatchHipError) as e:        # no self distances yet: the library's refusal
                        tc.fast_match_each(q, 0.9)
                    assert e.value.code == EINVAL
                    ctx.self_dist_batch([q], want_host=False)               # attached on the device
                    hb.set_selfdist(ctx.self_dist(hb))
                    rows, counts = tc.fast_match_each(q, 0.9)
                    assert tuple(rows.shape) == (len(SIZES), NQ, 3) and tuple(counts.shape) == (len(SIZES),)
                    r, cnt = rows.cpu().numpy(), counts.cpu().numpy()
                    want = host.match_accepted_each(hb, 0.9)
                    assert sum(len(w[0]) for w in want) > 10
                    for i, w in enumerate(want):
                        n = int(cnt[i])
                        assert n == len(w[0])
                        _same((r[i, :n, 0], r[i, :n, 1], r[i, :n, 2].copy().view(np.float32)), w[:3], "%s fast_match_each image %d" % (name, i))
                q.close()
        tc.clear()
        assert tc.info() == (0, 0, 0, 0)
        hb.close()


# ---- memory ---------------------------------------------------------------------------------------------------------------
def test_device_add_cycles_give_the_memory_back():
    """The criterion of test_hamming_gpu.py::test_bank_cycles_give_the_memory_back: free device memory must not drop by more
    than 4 MiB over 300 cycles."""
    torch = _torch()
    c = fastmatch_amd.Context(0)
    rng = np.random.default_rng(121)
    U = torch.from_numpy(synth.synth_sift(1500, rng)).cuda()
    Fh = (U.float() + 0.25).to(torch.float16)
    qb = c.bank(U[:NQ].cpu().numpy())
    qf = c.bank(U[:NQ].float().cpu().numpy() + 0.25, float_route=True)
    img = torch.empty((NQ, 4), dtype=torch.int32, device="cuda")
    idx = torch.empty((NQ, 4), dtype=torch.int32, device="cuda")
    dist = torch.empty((NQ, 4), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    col = c.collection()

    def cycle(k):
        f32 = k % 4 == 0
        src, q = (Fh, qf) if f32 else (U, qb)
        for n in (1000 + k % 500, 129, 700):
            _add_dev(col, src[:n])
        col.knn_dev(q, 1 + k % 4, img.data_ptr(), idx.data_ptr(), dist.data_ptr(), consumer_stream=stream)
        col.clear()

    for k in range(20):
        cycle(k)
    c.sync()
    base = c.mem_info()[0]
    for k in range(300):
        cycle(k)
    c.sync()
    after = c.mem_info()[0]
    assert base - after <= 4 << 20, (base, after)
    col.close(); qb.close(); qf.close()
    c.close()
