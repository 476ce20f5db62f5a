"""GPU: descriptors that are already on the device (fm_bank_create_dev) and results left there (fm_knn_dev, fm_xcheck1_dev,
fm_knn2_ratio_dev) against the HOST-ARRAY entry points of the same library, whose code the device forms leave untouched, and
against the oracle where the parity tests use it.  Every comparison is np.array_equal on the raw bits: no tolerance.

A bank made from a CUDA tensor must be indistinguishable from the bank the host creator makes from the same values, so every
entry point that takes banks is run on both and the outputs compared; the device-result calls must write what their host
forms return.  Ordering is exercised with real work in front: descriptors produced on a side stream behind a large matmul
with no host synchronisation, results consumed on a second stream, the source overwritten as soon as bank() returns."""
import ctypes

import numpy as np
import pytest

import fastmatch_amd
import oracle
from fastmatch_amd import _ffi, synth

pytestmark = pytest.mark.gpu

ROWS = [0, 1, 2, 127, 128, 129, 1000, 4099]
WIDTHS = [128, 61, 1]
BIN_WIDTHS = [1, 32, 64]
SOURCES = ["dense", "pitched", "pitched16"]      # a column slice at an odd offset (element loads) / at a 16-element offset
FLOATS = ["f32", "f16", "bf16"]
# (dtype, value kind, float_route): integer-valued floats go to the int8 route unless the float32 route is asked for
CASES = [("u8", "int", False), ("bin", "bits", False)] + \
        [(d, k, r) for d in FLOATS for k, r in (("int", False), ("int", True), ("frac", False), ("inf", False), ("nan", False))]


def _torch():
    import torch
    return torch


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same(a, b, what):
    assert len(a) == len(b), what
    for x, y in zip(a, b):
        x, y = np.asarray(x), np.asarray(y)
        assert x.shape == y.shape and x.dtype == y.dtype, what
        assert np.array_equal(_bits(x), _bits(y)), what


def _values(rng, dtype, kind, n, width):
    """Host values of the source tensor, as a torch CPU tensor of the source dtype."""
    torch = _torch()
    if dtype in ("u8", "bin"):
        return torch.from_numpy(rng.integers(0, 256, (n, width), dtype=np.uint8))
    if kind == "int":
        v = rng.integers(0, 256, (n, width)).astype(np.float32)
        v[rng.random((n, width)) < 0.5] = 0.0
    else:
        v = (rng.standard_normal((n, width)) * 40.0).astype(np.float32)
        if n > 0:
            v[0, 0] = 0.5        # exact in half and bfloat16: a short row of bfloat16 values can come out all integers in 0 .. 255
        if n > 0 and kind in ("inf", "nan"):
            v[n // 2, width // 2] = np.inf if kind == "inf" else np.nan
    return torch.from_numpy(v).to({"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[dtype])


def _on_device(vals, source):
    """The values as a CUDA tensor: dense, or a column slice of a wider tensor filled with other numbers."""
    torch = _torch()
    if source == "dense":
        return vals.cuda()
    off, extra = (3, 7) if source == "pitched" else (16, 32)
    wide = torch.full((vals.shape[0], vals.shape[1] + extra), 77, dtype=vals.dtype, device="cuda")
    wide[:, off:off + vals.shape[1]] = vals.cuda()
    view = wide[:, off:off + vals.shape[1]]
    assert vals.shape[0] < 2 or not view.is_contiguous()
    return view


def _host_twin(ctx, t, dtype, float_route):
    if dtype == "bin":
        return ctx.bank_binary(t.cpu().numpy())
    if dtype == "u8":
        return ctx.bank(t.cpu().numpy())
    return ctx.bank(t.float().cpu().numpy(), float_route=float_route)


def _call(f):
    """The outputs of a call, or the FM_E* code it was refused with: both banks of a pair must meet the same fate."""
    try:
        out = f()
        return out if isinstance(out, tuple) else (out,)
    except _ffi.FastMatchHipError as e:
        return ("refused", e.code)


def _outputs(ctx, q, t, binary, sd):
    """Everything the matcher entry points return for the pair (q, t); sd = self distances to attach to q."""
    out = [_call(lambda: ctx.knn2(q, t)), _call(lambda: ctx.knn(q, t, 3)), _call(lambda: ctx.xcheck1(q, t)),
           _call(lambda: ctx.knn2_ratio(q, t, 0.9))]
    if not binary:
        d2 = np.zeros((0, 2), np.float32) if isinstance(out[0][0], str) else out[0][1]
        fin = d2[:, 1][np.isfinite(d2[:, 1])] if d2.size else d2
        r = float(np.median(fin)) * 1.02 if fin.size else 1.0
        out.append(_call(lambda: ctx.radius_match(q, t, r)))
        q.set_selfdist(sd)
        out.append(_call(lambda: ctx.match_accepted(q, t, 0.95)))
    return out


def _compare_banks(ctx, dev, host, partner, binary, what):
    assert (dev.n, dev.dim, dev.kind) == (host.n, host.dim, host.kind), what
    sd = None
    if not binary:
        sd_d, sd_h = ctx.self_dist(dev), ctx.self_dist(host)
        _same([sd_d], [sd_h], what + " self_dist")
        sd = sd_h
    sdp = None if binary else ctx.self_dist(partner)
    for a, b, s, tag in ((dev, partner, sd, "as query"), (partner, dev, sdp, "as train")):
        ha, hb = (host, partner) if a is dev else (partner, host)
        got, want = _outputs(ctx, a, b, binary, s), _outputs(ctx, ha, hb, binary, s)
        for g, w, name in zip(got, want, ("knn2", "knn3", "xcheck1", "knn2_ratio", "radius_match", "match_accepted")):
            _same(g, w, "%s %s %s" % (what, tag, name))


@pytest.mark.parametrize("dtype,kind,float_route", CASES, ids=["%s-%s%s" % (d, k, "-route" if r else "") for d, k, r in CASES])
def test_bank_from_device_equals_the_host_bank(ctx, dtype, kind, float_route):
    from fastmatch_amd import torchmatch
    rng = np.random.default_rng(1000 + CASES.index((dtype, kind, float_route)))
    binary = dtype == "bin"
    for width in (BIN_WIDTHS if binary else WIDTHS):
        pvals = _values(rng, dtype, "frac" if kind in ("inf", "nan") else kind, 300, width)
        partner = _host_twin(ctx, pvals, dtype, float_route)
        for n in ROWS:
            if n == 0 and kind in ("inf", "nan"):
                continue
            vals = _values(rng, dtype, kind, n, width)
            for source in SOURCES:
                what = "%s %s route=%s n=%d width=%d %s" % (dtype, kind, float_route, n, width, source)
                t = _on_device(vals, source)
                dev = torchmatch.bank(t, binary=binary, float_route=float_route, context=ctx)
                host = _host_twin(ctx, t, dtype, float_route)
                try:
                    if n > 0:
                        want_kind = _ffi.FM_BANK_BIN if binary else \
                            _ffi.FM_BANK_I8 if (dtype == "u8" or (kind == "int" and not float_route)) else _ffi.FM_BANK_F32
                        if not binary and dtype != "u8":       # (the rule itself, from the values: integers in 0 .. 255 or not)
                            f = vals.float().numpy()
                            with np.errstate(invalid="ignore"):
                                integral = bool(np.all((f == np.rint(f)) & (f >= 0) & (f <= 255)))
                            assert integral == (kind == "int"), what
                        assert dev.kind == want_kind, what
                    _compare_banks(ctx, dev, host, partner, binary, what)
                finally:
                    dev.close(); host.close()
        partner.close()


def test_raw_pointer_form_and_no_stream(ctx):
    """Context.bank_from_device itself: an explicit pitch, stream=None after a host synchronisation."""
    torch = _torch()
    rng = np.random.default_rng(5)
    wide = torch.from_numpy(rng.integers(0, 256, (700, 200), dtype=np.uint8)).cuda()
    torch.cuda.synchronize()
    dev = ctx.bank_from_device(wide.data_ptr() + 40, _ffi.FM_DT_U8, 700, 128, pitch=200, stream=None)
    host = ctx.bank(wide[:, 40:168].cpu().numpy())
    _same(ctx.knn2(dev, host), ctx.knn2(host, host), "raw pointer")
    dev.close(); host.close()


def test_device_bank_against_the_oracle(ctx):
    """As the parity tests: uint8 rows and float32 rows (the fixed fma-chain order) from CUDA tensors against the oracle."""
    from fastmatch_amd import torchmatch
    torch = _torch()
    Q, T, _ = synth.planted_pair(900, 1300, seed=11)
    qt, tt = torch.from_numpy(Q).cuda(), torch.from_numpy(T).cuda()
    idx, dist = torchmatch.knn(qt, tt, 2)
    _same((idx.cpu().numpy(), dist.cpu().numpy()), oracle.bf_knn(Q, T, 2), "u8 knn2 vs oracle")
    tidx, d = torchmatch.mutual_nn(qt, tt)
    _same((tidx.cpu().numpy(), d.cpu().numpy()), oracle.bf_xcheck1(Q, T), "u8 xcheck vs oracle")
    rng = np.random.default_rng(12)
    Qf = (Q + rng.uniform(-0.5, 0.5, Q.shape)).astype(np.float32)
    Tf = (T + rng.uniform(-0.5, 0.5, T.shape)).astype(np.float32)
    qt, tt = torch.from_numpy(Qf).cuda(), torch.from_numpy(Tf).cuda()
    idx, dist = torchmatch.knn(qt, tt, 2)
    _same((idx.cpu().numpy(), dist.cpu().numpy()), oracle.bf_knn(Qf, Tf, 2, order=1), "f32 knn2 vs oracle")
    tidx, d = torchmatch.mutual_nn(qt, tt)
    _same((tidx.cpu().numpy(), d.cpu().numpy()), oracle.bf_xcheck1(Qf, Tf, order=1), "f32 xcheck vs oracle")
    q2, t2, d2 = torchmatch.ratio_match(qt, tt, 0.8)
    lowe = oracle.lowe_ratio(oracle.bf_knn(Qf, Tf, 2, order=1)[1])
    keep = np.nonzero(lowe < 0.8)[0].astype(np.int32)
    assert np.array_equal(q2.cpu().numpy(), keep)


# ---- device results -------------------------------------------------------------------------------------------------------
SHAPES = [(0, 5), (5, 0), (1, 1), (5, 3), (9, 7), (129, 127), (1000, 4099), (4099, 1000)]


def _kind_banks(ctx, rng, kind, nq, nt):
    if kind == "bin":
        Q, T = rng.integers(0, 256, (nq, 32), dtype=np.uint8), rng.integers(0, 256, (nt, 32), dtype=np.uint8)
        if nq and nt:
            T[: min(nq, nt) // 2] = Q[: min(nq, nt) // 2]      # planted duplicates, some a bit away: accepted ratio matches
            T[: min(nq, nt) // 4, 0] ^= 1
        return ctx.bank_binary(Q), ctx.bank_binary(T)
    Q, T = synth.synth_sift(nq, rng), synth.synth_sift(nt, rng)
    if nq and nt:
        T[: min(nq, nt) // 2] = Q[: min(nq, nt) // 2]          # planted duplicates: accepted ratio matches, zero distances
        T[: min(nq, nt) // 4, 0] ^= 1
    if kind == "f32":
        return ctx.bank(Q.astype(np.float32) + 0.25, float_route=True), ctx.bank(T.astype(np.float32) + 0.25, float_route=True)
    return ctx.bank(Q), ctx.bank(T)


@pytest.mark.parametrize("kind", ["i8", "f32", "bin"])
def test_device_results_equal_the_host_forms(ctx, kind):
    torch = _torch()
    rng = np.random.default_rng({"i8": 21, "f32": 22, "bin": 23}[kind])
    stream = torch.cuda.current_stream().cuda_stream
    for nq, nt in SHAPES:
        q, t = _kind_banks(ctx, rng, kind, nq, nt)
        what = "%s %dx%d" % (kind, nq, nt)
        for k in range(1, 9):                                   # (5, 3), (9, 7), (5, 0): a train bank smaller than k
            idx = torch.full((nq, k), -7, dtype=torch.int32, device="cuda")
            dist = torch.full((nq, k), -7.0, dtype=torch.float32, device="cuda")
            ctx.knn_dev(q, t, k, idx.data_ptr() if nq else 0, dist.data_ptr() if nq else 0, consumer_stream=stream)
            got = (idx.cpu().numpy(), dist.cpu().numpy())
            if nt == 0:                                         # the header's words, whatever the host form does with an empty bank
                _same(got, (np.full((nq, k), -1, np.int32), np.full((nq, k), np.inf, np.float32)), what + " knn k=%d, no train rows" % k)
            want = _call(lambda: ctx.knn(q, t, k))
            if nt > 0 or not isinstance(want[0], str):
                _same(got, want, what + " knn k=%d" % k)
        tidx = torch.full((nq,), -7, dtype=torch.int32, device="cuda")
        dist = torch.full((nq,), -7.0, dtype=torch.float32, device="cuda")
        ctx.xcheck1_dev(q, t, tidx.data_ptr() if nq else 0, dist.data_ptr() if nq else 0, consumer_stream=stream)
        _same((tidx.cpu().numpy(), dist.cpu().numpy()), ctx.xcheck1(q, t), what + " xcheck1")
        hq, ht, hd, _ = ctx.knn2_ratio(q, t, 0.9)
        m = hq.shape[0]
        for cap in sorted({nq, max(m // 2, 0), 0, nq + 5}):      # a cap below the accepted count: count and prefix
            rows = torch.full((max(cap, 1), 3), -7, dtype=torch.int32, device="cuda")
            count = torch.full((1,), -7, dtype=torch.int64, device="cuda")
            total = ctx.knn2_ratio_dev(q, t, 0.9, rows.data_ptr(), count.data_ptr(), cap, want_count=True, consumer_stream=stream)
            assert total == m, what
            c = int(count.item())
            assert c == min(m, cap), what
            r = rows.cpu().numpy()[:c]
            _same((r[:, 0], r[:, 1], r[:, 2].copy().view(np.float32)), (hq[:c], ht[:c], hd[:c]), what + " ratio cap=%d" % cap)
            assert (rows.cpu().numpy()[c:] == -7).all(), what + ": rows past the count were written"
            # without the host count: nothing but the device word
            count.fill_(-7)
            assert ctx.knn2_ratio_dev(q, t, 0.9, rows.data_ptr(), count.data_ptr(), cap, consumer_stream=stream) is None
            assert int(count.item()) == c
        if kind != "f32" and nq >= 1000:
            assert m > 10 and m // 2 < m                         # the truncated case is a real one
        q.close(); t.close()


def test_torchmatch_on_banks_and_tensors(ctx):
    """The tensor-level functions: resident banks, tensors, half precision, and a mix of the two."""
    from fastmatch_amd import torchmatch
    torch = _torch()
    rng = np.random.default_rng(31)
    Q = (rng.standard_normal((800, 96)) * 3).astype(np.float16)
    T = (rng.standard_normal((1500, 96)) * 3).astype(np.float16)
    qt, tt = torch.from_numpy(Q).cuda(), torch.from_numpy(T).cuda()
    hq, ht = ctx.bank(Q.astype(np.float32)), ctx.bank(T.astype(np.float32))
    for a, b in ((qt, tt), (torchmatch.bank(qt, context=ctx), tt), (qt, torchmatch.bank(tt, context=ctx))):
        for k in (1, 2, 5):
            idx, dist = torchmatch.knn(a, b, k)
            assert idx.is_cuda and idx.dtype == torch.int32 and dist.dtype == torch.float32 and tuple(idx.shape) == (800, k)
            _same((idx.cpu().numpy(), dist.cpu().numpy()), ctx.knn(hq, ht, k), "torchmatch.knn")
        tidx, dist = torchmatch.mutual_nn(a, b)
        _same((tidx.cpu().numpy(), dist.cpu().numpy()), ctx.xcheck1(hq, ht), "torchmatch.mutual_nn")
        qi, ti, di = torchmatch.ratio_match(a, b, 0.95)
        w = ctx.knn2_ratio(hq, ht, 0.95)
        _same((qi.cpu().numpy(), ti.cpu().numpy(), di.cpu().numpy()), w[:3], "torchmatch.ratio_match")
    # a tensor whose columns are strided is made contiguous first
    wide = torch.from_numpy(np.repeat(Q, 2, axis=1)).cuda()
    idx, dist = torchmatch.knn(wide[:, ::2], tt, 2)
    _same((idx.cpu().numpy(), dist.cpu().numpy()), ctx.knn(hq, ht, 2), "strided columns")


# ---- ordering -------------------------------------------------------------------------------------------------------------
def test_ordering_producer_consumer_and_source_lifetime(ctx):
    from fastmatch_amd import torchmatch
    torch = _torch()
    g = torch.Generator(device="cuda").manual_seed(3)
    A = torch.randn(4096, 4096, device="cuda", generator=g)
    Tn = torch.from_numpy(synth.synth_sift(3000, np.random.default_rng(41))).cuda()
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        B = A
        for _ in range(12):                                    # tens of milliseconds of work in front of the descriptors
            B = torch.tanh(B @ A * 0.01)
        desc = ((B[:2000, :128] * 1.0e5).abs() % 256).floor().to(torch.uint8)     # exists only once the matmuls are done
        keep = desc.clone()
        qb = torchmatch.bank(desc, context=ctx)                # producer = s1, no host synchronisation before it
        desc.zero_()                                           # the source is the caller's again
        tb = torchmatch.bank(Tn, context=ctx)
    with torch.cuda.stream(s2):
        C = A
        for _ in range(6):
            C = torch.tanh(C @ A * 0.01)
        idx = torch.empty((2000, 2), dtype=torch.int32, device="cuda")
        dist = torch.empty((2000, 2), dtype=torch.float32, device="cuda")
        idx.fill_(-7); dist.fill_(-7.0)                        # queued on s2 behind the matmuls: the library's writes must follow
        ctx.knn_dev(qb, tb, 2, idx.data_ptr(), dist.data_ptr(), consumer_stream=s2.cuda_stream)
        idx_c, dist_c = idx.clone(), dist.clone()              # consumed on s2 with no host synchronisation
        tidx, xd = torchmatch.mutual_nn(qb, tb)
        tidx_c = tidx.clone()
    s2.synchronize(); s1.synchronize()
    assert int(desc.max().item()) == 0
    K = keep.cpu().numpy()
    assert K.max() > 0 and len(np.unique(K)) > 50              # the descriptors were real
    hq, ht = ctx.bank(K), ctx.bank(Tn.cpu().numpy())
    _same((idx_c.cpu().numpy(), dist_c.cpu().numpy()), ctx.knn2(hq, ht), "knn2 behind the producer")
    _same((tidx_c.cpu().numpy(), xd.cpu().numpy()), ctx.xcheck1(hq, ht), "xcheck1 behind the producer")
    _same(ctx.knn2(qb, tb), ctx.knn2(hq, ht), "bank after its source was zeroed")


# ---- errors ---------------------------------------------------------------------------------------------------------------
def test_refusals_carry_a_code_and_a_message_and_leave_the_context_usable(ctx):
    torch = _torch()
    lib, h, P = ctx.lib, ctx.handle, ctypes.c_void_p
    NOS = _ffi._stream_arg(None)
    rng = np.random.default_rng(51)
    Q, T = synth.synth_sift(300, rng), synth.synth_sift(400, rng)
    qb, tb = ctx.bank(Q), ctx.bank(T)
    bb = ctx.bank_binary(rng.integers(0, 256, (300, 32), dtype=np.uint8))
    q32, t32 = ctx.bank(Q[:, :32]), ctx.bank(T[:, :32])              # (L2 banks of the binary bank's width: only the kind differs)
    ref = ctx.knn2(qb, tb)
    d = torch.zeros((64, 256), dtype=torch.uint8, device="cuda")
    out_i = torch.zeros((300, 8), dtype=torch.int32, device="cuda")
    out_f = torch.zeros((300, 8), dtype=torch.float32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    host = np.zeros((64, 128), np.uint8)
    EINVAL, EUNSUP = -1, -4

    def create(ptr, dtype, n, dim, pitch):
        out = P()
        rc = lib.fm_bank_create_dev(h, P(ptr) if ptr else None, dtype, n, dim, pitch, 0, NOS, ctypes.byref(out))
        assert out.value is None or rc == 0
        return rc

    cases = [
        ("host pointer", lambda: create(host.ctypes.data, _ffi.FM_DT_U8, 64, 128, 0), EINVAL),
        ("pitch below the row", lambda: create(d.data_ptr(), _ffi.FM_DT_U8, 64, 128, 64), EINVAL),
        ("misaligned pitch", lambda: create(d.data_ptr(), _ffi.FM_DT_F32, 16, 8, 34), EINVAL),
        ("misaligned half pitch", lambda: create(d.data_ptr(), _ffi.FM_DT_F16, 16, 8, 17), EINVAL),
        ("dim 129", lambda: create(d.data_ptr(), _ffi.FM_DT_U8, 64, 129, 0), EUNSUP),
        ("65 binary bytes", lambda: create(d.data_ptr(), _ffi.FM_DT_BIN, 64, 65, 0), EUNSUP),
        ("dtype 0", lambda: create(d.data_ptr(), 0, 64, 128, 0), EINVAL),
        ("dtype 9", lambda: create(d.data_ptr(), 9, 64, 128, 0), EINVAL),
        ("NULL rows", lambda: create(0, _ffi.FM_DT_U8, 64, 128, 0), EINVAL),
        ("knn NULL idx", lambda: lib.fm_knn_dev(h, qb.handle, tb.handle, 2, None, P(out_f.data_ptr()), NOS), EINVAL),
        ("knn NULL dist", lambda: lib.fm_knn_dev(h, qb.handle, tb.handle, 2, P(out_i.data_ptr()), None, NOS), EINVAL),
        ("knn host output", lambda: lib.fm_knn_dev(h, qb.handle, tb.handle, 2, P(np.zeros(600, np.int32).ctypes.data), P(out_f.data_ptr()), NOS), EINVAL),
        ("xcheck NULL", lambda: lib.fm_xcheck1_dev(h, qb.handle, tb.handle, None, None, NOS), EINVAL),
        ("ratio NULL count", lambda: lib.fm_knn2_ratio_dev(h, qb.handle, tb.handle, 0.8, 300, P(out_i.data_ptr()), None, None, NOS), EINVAL),
        ("ratio NULL rows", lambda: lib.fm_knn2_ratio_dev(h, qb.handle, tb.handle, 0.8, 300, None, P(cnt.data_ptr()), None, NOS), EINVAL),
        ("k = 0", lambda: lib.fm_knn_dev(h, qb.handle, tb.handle, 0, P(out_i.data_ptr()), P(out_f.data_ptr()), NOS), EINVAL),
        ("k = 9", lambda: lib.fm_knn_dev(h, qb.handle, tb.handle, 9, P(out_i.data_ptr()), P(out_f.data_ptr()), NOS), EUNSUP),
        ("binary against L2 (knn)", lambda: lib.fm_knn_dev(h, bb.handle, t32.handle, 2, P(out_i.data_ptr()), P(out_f.data_ptr()), NOS), EINVAL),
        ("binary against L2 (xcheck)", lambda: lib.fm_xcheck1_dev(h, q32.handle, bb.handle, P(out_i.data_ptr()), P(out_f.data_ptr()), NOS), EINVAL),
        ("binary against L2 (ratio)", lambda: lib.fm_knn2_ratio_dev(h, bb.handle, t32.handle, 0.8, 300, P(out_i.data_ptr()), P(cnt.data_ptr()), None, NOS), EINVAL),
    ]
    for name, call, want in cases:
        rc = call()
        assert rc == want, "%s: returned %d, expected %d" % (name, rc, want)
        msg = lib.fm_last_error(h)
        assert msg and len(msg.decode()) > 10, name
        _same(ctx.knn2(qb, tb), ref, "context after: " + name)           # ... and the context is still good
    # n = 0 is valid, whatever the pointer
    e = ctx.bank_from_device(0, _ffi.FM_DT_F16, 0, 61)
    assert (e.n, e.dim) == (0, 61)
    for b in (e, qb, tb, bb, q32, t32):
        b.close()


# ---- memory ---------------------------------------------------------------------------------------------------------------
GRANULE = 4 << 20        # the criterion of test_memory_soak_gpu.py: one-sided, free memory must not go down by more than two of
                         # the runtime's 2 MiB pieces


def test_200_cycles_from_device_sources_give_the_memory_back():
    from fastmatch_amd import torchmatch
    torch = _torch()
    c = fastmatch_amd.Context(0)
    rng = np.random.default_rng(61)
    Qu = torch.from_numpy(synth.synth_sift(1500, rng)).cuda()
    Tu = torch.from_numpy(synth.synth_sift(2600, rng)).cuda()
    Th = (Tu.float() + 0.25).to(torch.float16)
    Tb = Tu[:, :32].contiguous()
    idx = torch.empty((2600, 4), dtype=torch.int32, device="cuda")
    dist = torch.empty((2600, 4), dtype=torch.float32, device="cuda")
    rows = torch.empty((2600, 3), dtype=torch.int32, device="cuda")
    cnt = torch.empty(1, dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def cycle(k):
        qb, tb = torchmatch.bank(Qu, context=c), torchmatch.bank(Tu[:2000 + k % 600], context=c)
        c.knn_dev(qb, tb, 1 + k % 4, idx.data_ptr(), dist.data_ptr(), consumer_stream=stream)
        c.xcheck1_dev(qb, tb, idx.data_ptr(), dist.data_ptr(), consumer_stream=stream)
        n = c.knn2_ratio_dev(qb, tb, 0.9, rows.data_ptr(), cnt.data_ptr(), 1500, want_count=True, consumer_stream=stream)
        if k % 3 == 0:
            fb = torchmatch.bank(Th[:1200 + k % 300], context=c)
            c.knn_dev(fb, fb, 2, idx.data_ptr(), dist.data_ptr(), consumer_stream=stream)
            fb.close()
        if k % 5 == 0:
            hb = torchmatch.bank(Tb, binary=True, context=c)
            c.xcheck1_dev(hb, hb, idx.data_ptr(), dist.data_ptr(), consumer_stream=stream)
            hb.close()
        qb.close(); tb.close()
        return n

    for k in range(30):                                          # warm-up: the workspaces reach their sizes
        cycle(k)
    c.sync()
    base = c.mem_info()[0]
    for k in range(200):
        cycle(k)
    c.sync()
    after = c.mem_info()[0]
    assert base - after <= GRANULE, (base, after)
    c.close()
