"""GPU: masked radiusMatch on bank pairs -- fm_radius_match_masked, fm_radius_match_masked_dev, matchutil.bf_radius_match_masked,
BFMatcher.radiusMatch(mask=, compactResult=), torchmatch's mask= keywords -- on the integer route, the float32 route (with and
without its fp16 filter), binary rows of 8 / 32 / 64 bytes and wide float rows of 129 / 256 values.

Every result is compared bit for bit with tests/radius_masked_ref.py: the unmasked reference list with the forbidden entries
removed -- offsets, train indices, distances as uint32 bit patterns.  300 x 2100 rows: two workgroups of query rows (three on
the wide route), three train splits (five on the Hamming route), a partial last mask word."""
import ctypes

import numpy as np
import pytest

import fastmatch_amd
from fastmatch_amd import _ffi, matchutil
import radius_masked_ref as M

pytestmark = pytest.mark.gpu

P = ctypes.c_void_p
EINVAL, EUNSUPPORTED = -1, -4
INF = np.float32(np.inf)


def _ptr(a):
    return a.ctypes.data_as(P)


def _bank(c, name, rows):
    if M.kind(name) == "ham":
        return c.bank_binary(rows)
    return c.bank(rows, float_route=name.startswith("f32")) if M.kind(name) != "wide" else c.bank(rows)


def _unmasked(c, name, qb, tb, r):
    k = M.kind(name)
    return c.hamming_radius_match(qb, tb, r) if k == "ham" else c.wide_radius_match(qb, tb, r) if k == "wide" else c.radius_match(qb, tb, r)


@pytest.fixture(scope="module", params=M.PAIR_SETS)
def pair(ctx, request):
    name = request.param
    Q, T = M.data(name)
    qb, tb = _bank(ctx, name, Q), _bank(ctx, name, T)
    want_kind = {"i8": _ffi.FM_BANK_I8, "ham": _ffi.FM_BANK_BIN, "wide": _ffi.FM_BANK_F32W}.get(M.kind(name), _ffi.FM_BANK_F32)
    assert qb.kind == tb.kind == want_kind
    masks = {}

    def mask(pattern):
        if pattern not in masks:
            masks[pattern] = ctx.mask(M.NQ, M.NT).set(M.mask(pattern))
        return masks[pattern]

    yield name, qb, tb, mask
    for m in masks.values():
        m.close()
    qb.close()
    tb.close()


def test_patterns_and_radii(ctx, pair):
    """random, band (mostly zero words: the skips), third (whole query rows forbidden), first / last (single bits at train row
    0 and nt - 1) under a scalar radius, a radius per row and a mixed array with 0, a negative value, NaN and +inf."""
    name, qb, tb, mask = pair
    for pattern in ("random", "band", "third", "first", "last"):
        for what, r in M.radii(name) + [("inf", INF)]:
            M.same_pair(ctx.radius_match_masked(qb, tb, mask(pattern), r), M.want(name, r, M.mask(pattern)), (name, pattern, what))


def test_all_ones_is_the_unmasked_call_and_all_zeros_is_empty(ctx, pair):
    name, qb, tb, mask = pair
    for what, r in M.radii(name) + [("inf", INF)]:
        got = ctx.radius_match_masked(qb, tb, mask("ones"), r)
        plain = _unmasked(ctx, name, qb, tb, r)
        for a, b in zip(got, plain):
            assert a.dtype == b.dtype and np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a,
                                                         b.view(np.uint32) if b.dtype == np.float32 else b), (name, what)
        M.same_pair(got, M.want(name, r, M.mask("ones")), (name, "ones", what))
        off, idx, dist = ctx.radius_match_masked(qb, tb, mask("zeros"), r)
        assert off.shape == (M.NQ + 1,) and not off.any() and idx.size == dist.size == 0, (name, what)
    for r in (0.0, -1.0, np.nan, -np.inf):
        off, idx, dist = ctx.radius_match_masked(qb, tb, mask("ones"), np.float32(r))
        assert not off.any() and idx.size == 0


def test_the_bit_walk_lists_exactly_the_congruent_rows(ctx, pair):
    name, qb, tb, mask = pair
    got = ctx.radius_match_masked(qb, tb, mask("walk"), INF)
    M.same_pair(got, M.want(name, INF, M.mask("walk")), (name, "walk"))
    off, idx, _ = got
    for i in range(M.NQ):
        assert np.array_equal(np.sort(idx[off[i]:off[i + 1]]), np.arange(i % 64, M.NT, 64)), (name, i)


@pytest.mark.parametrize("name", ["i8", "f32", "f32all", "ham32", "wide129"])
def test_query_chunks_that_start_off_a_workgroup_boundary(name):
    """radius_ws_bytes = 65536 at r = +inf under the random mask: ~1050 entries per row, two or three rows per chunk -- every
    chunk's launch starts at another query row, and the mask pointer has to follow it."""
    c = fastmatch_amd.Context(0)
    try:
        c.set_option("radius_ws_bytes", 65536)
        Q, T = M.data(name)
        qb, tb = _bank(c, name, Q), _bank(c, name, T)
        with c.mask(M.NQ, M.NT) as mk:
            M.same_pair(c.radius_match_masked(qb, tb, mk.set(M.mask("random")), INF), M.want(name, INF, M.mask("random")), (name, "chunks"))
            rows = M.row_radii(name)
            M.same_pair(c.radius_match_masked(qb, tb, mk, rows), M.want(name, rows, M.mask("random")), (name, "chunks, rows"))
    finally:
        c.close()


def test_cap(ctx, pair):
    """Counts only (cap = 0), a cap that cuts inside a row (the longest prefix of whole rows is written, nothing behind it),
    cap = total."""
    name, qb, tb, mask = pair
    r = M.radius(name)
    want = M.want(name, r, M.mask("random"))
    woff, total = want[0], int(want[0][-1])
    fn, h, mk = ctx.lib.fm_radius_match_masked, ctx.handle, mask("random").handle
    off = np.full(M.NQ + 1, -7, np.int64)
    tot = ctypes.c_int64(-1)
    assert fn(h, qb.handle, tb.handle, mk, None, float(r), 0, _ptr(off), None, None, ctypes.byref(tot)) == 0
    assert np.array_equal(off, woff) and tot.value == total
    row = int(np.searchsorted(woff, total // 2, side="right")) - 1       # the row the cap falls into
    assert 0 < row < M.NQ and woff[row + 1] > woff[row]
    cap = int(woff[row]) + 1 if woff[row + 1] - woff[row] > 1 else int(woff[row])
    fit = int(np.searchsorted(woff, cap, side="right")) - 1             # rows whose whole lists fit
    for cp, nfit in ((cap, fit), (total, M.NQ)):
        off[:] = -7
        idx, dist = np.full(total + 3, -9, np.int32), np.full(total + 3, -9.0, np.float32)
        assert fn(h, qb.handle, tb.handle, mk, None, float(r), cp, _ptr(off), _ptr(idx), _ptr(dist), ctypes.byref(tot)) == 0
        assert np.array_equal(off, woff) and tot.value == total
        n = int(woff[nfit])
        assert np.array_equal(idx[:n], want[4][:n]) and np.array_equal(M.bits(dist[:n]), M.bits(want[3][:n]))
        assert (idx[max(n, cp):] == -9).all() and (dist[max(n, cp):] == -9.0).all()


def test_device_forms_and_torchmatch(ctx, pair):
    """Radii, mask and results in device memory: the mask set with fm_mask_set_dev from a torch bool tensor, the lists of
    fm_radius_match_masked_dev equal to the host form's."""
    import torch
    from fastmatch_amd import torchmatch
    name, qb, tb, mask = pair
    call = {"ham": torchmatch.hamming_radius_match, "wide": torchmatch.wide_radius_match}.get(M.kind(name), torchmatch.radius_match)
    mt = torch.from_numpy(M.mask("random").copy()).cuda()
    assert mt.dtype == torch.bool
    for what, r in M.radii(name):
        rt = r if np.ndim(r) == 0 else torch.from_numpy(r).cuda()
        got = tuple(x.cpu().numpy() for x in call(qb, tb, rt, mask=mt))
        M.same_pair(got, M.want(name, r, M.mask("random")), (name, "torch", what))
    # a resident Mask, and a counts call straight through the binding
    got = tuple(x.cpu().numpy() for x in call(qb, tb, float(M.radius(name)), mask=mask("band")))
    M.same_pair(got, M.want(name, M.radius(name), M.mask("band")), (name, "torch, resident"))
    offs = torch.full((M.NQ + 1,), -1, dtype=torch.int64, device="cuda")
    n = ctx.radius_match_masked_dev(qb, tb, mask("band"), 0, float(M.radius(name)), 0, offs.data_ptr(), 0, 0,
                                    consumer_stream=torch.cuda.current_stream().cuda_stream)
    assert n == got[0][-1] and np.array_equal(offs.cpu().numpy(), got[0])
    with pytest.raises(ValueError, match="mask"):
        call(qb, tb, 1.0, mask=mt[:, :-1])


def test_matchutil_and_bfmatcher(ctx, pair):
    name, qb, tb, mask = pair
    Q, T = M.data(name)
    opts = {"context": ctx}
    if M.kind(name) == "ham":
        opts["normType"] = matchutil.NORM_HAMMING
    r = M.radius(name)
    want = M.want(name, r, M.mask("third"))
    M.same_pair(matchutil.bf_radius_match_masked_arrays(Q, T, r, M.mask("third"), options=opts), want, (name, "arrays"))
    M.same_pair(matchutil.bf_radius_match_masked_arrays(qb, tb, r, mask("third"), options=opts), want, (name, "resident"))
    lists = matchutil.bf_radius_match_masked(Q, T, r, M.mask("third").view(np.uint8), options=opts)
    assert len(lists) == M.NQ and [len(x) for x in lists] == np.diff(want[0]).tolist()
    assert [m.trainIdx for x in lists for m in x] == want[4].tolist()
    bf = matchutil.BFMatcher(opts.get("normType", matchutil.NORM_L2), options={"context": ctx})
    compact = bf.radiusMatch(Q, T, r, mask=M.mask("third"), compactResult=True)
    assert len(compact) == M.NQ - len(range(0, M.NQ, 3))                 # exactly the all-zero mask rows are dropped
    assert [x for i, x in enumerate(lists) if i % 3] and \
        [[(m.queryIdx, m.trainIdx) for m in x] for x in compact] == [[(m.queryIdx, m.trainIdx) for m in x] for i, x in enumerate(lists) if i % 3]
    assert len(bf.radiusMatch(Q, T, r, mask=M.mask("third"))) == M.NQ
    if M.kind(name) in ("i8", "f32"):                                     # mask=None: the call it was
        plain = bf.radiusMatch(Q, T, r)
        assert [len(x) for x in plain] == np.diff(M.ref(name).cut(r)[0]).tolist()


# ---- grown banks ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["i8", "f32"])
def test_grown_train_banks_never_list_a_gap_row(ctx, route):
    """A train bank built with capacity + appends (every append starts on a multiple of 32 rows: gap rows inside) under an
    all-ones and a random mask over its PHYSICAL rows: the reference lists of the real rows, indices turned physical."""
    import grown_ref as G
    import radius_coll_ref as RC
    Q, T = M.data(route)
    lay = G.Layout([700, 45, 0, 1355])
    assert lay.n_real == M.NT and lay.gaps.size > 0
    qb = _bank(ctx, route, Q)
    if route == "i8":
        tb = ctx.bank_with_capacity(np.zeros((0, 128), np.uint8), lay.n_phys + 70)
    else:
        tb = ctx.bank_f32_with_capacity(128, lay.n_phys + 70, qb)
    try:
        for part, first in zip(lay.split(T), lay.first):
            assert tb.append(part) == first
        assert tb.n == lay.n_phys
        ref = M.ref(route)
        rng = np.random.default_rng(77)
        for pattern, Mp in (("ones", np.ones((M.NQ, lay.n_phys), bool)), ("random", rng.random((M.NQ, lay.n_phys)) < 0.5)):
            assert Mp[:, lay.gaps].any()                                  # the mask permits gap rows; the sweep must not
            with ctx.mask(M.NQ, lay.n_phys) as mk:
                mk.set(Mp)
                for what, r in (("scalar", M.radius(route)), ("inf", INF)):
                    off, idx, dist = ctx.radius_match_masked(qb, tb, mk, r)
                    assert not np.isin(idx, lay.gaps).any(), (route, pattern, what)
                    woff, _, _, wdist, wglob = M.filtered(ref.cut(r), Mp[:, lay.phys])
                    assert np.array_equal(off, woff) and np.array_equal(idx, lay.to_phys(wglob)), (route, pattern, what)
                    assert np.array_equal(M.bits(dist), M.bits(wdist)), (route, pattern, what)
    finally:
        tb.close()
        qb.close()


# ---- empty operands and errors --------------------------------------------------------------------------------------------
def test_empty_banks(ctx):
    Q, T = M.data("i8")
    for nq, nt in ((0, 5), (5, 0), (0, 0)):
        qb, tb = ctx.bank(np.ascontiguousarray(Q[:nq])), ctx.bank(np.ascontiguousarray(T[:nt]))
        with ctx.mask(nq, nt) as mk:
            if nq and nt:
                mk.set_all(True)
            off, idx, dist = ctx.radius_match_masked(qb, tb, mk, INF)
            assert off.shape == (nq + 1,) and not off.any() and idx.size == dist.size == 0
        qb.close()
        tb.close()


def test_errors_in_order_and_outputs_untouched(ctx):
    Q, T = M.data("i8")
    Qh, Th = M.data("ham32")
    qb, tb, t64 = ctx.bank(Q[:40].copy()), ctx.bank(T[:90].copy()), ctx.bank(np.ascontiguousarray(T[:90, :64]))
    hb = ctx.bank_binary(Th[:90].copy())
    other = fastmatch_amd.Context(0)
    coll = ctx.collection()
    coll.add(T[:90].copy())
    lib, h = ctx.lib, ctx.handle
    off = np.full(41, -7, np.int64)
    idx, dist = np.full(8, -9, np.int32), np.full(8, -9.0, np.float32)
    tot = ctypes.c_int64(-5)

    def call(q, t, m, cap=8, o=off, i=idx, d=dist, dev=False):
        if dev:
            rc = lib.fm_radius_match_masked_dev(h, q, t, m, None, 500.0, cap, _ptr(o) if o is not None else None,
                                                _ptr(i) if i is not None else None, _ptr(d) if d is not None else None, ctypes.byref(tot), None)
        else:
            rc = lib.fm_radius_match_masked(h, q, t, m, None, 500.0, cap, _ptr(o) if o is not None else None,
                                            _ptr(i) if i is not None else None, _ptr(d) if d is not None else None, ctypes.byref(tot))
        msg = lib.fm_last_error(h)
        return rc, (msg.decode() if msg else "")

    try:
        with ctx.mask(40, 90) as ok, ctx.mask(41, 90) as bad_nq, ctx.mask(40, 91) as bad_nt, other.mask(40, 90) as foreign, coll.mask(40) as cm:
            ok.set_all(True)
            for dev in (False, True):
                # (1) NULL handles, the mask included
                for args in ((None, tb.handle, ok.handle), (qb.handle, None, ok.handle), (qb.handle, tb.handle, None)):
                    rc, msg = call(*args, dev=dev)
                    assert rc == EINVAL and "NULL" in msg, msg
                # (2) the pair, in front of the mask: a width mismatch, a binary bank against one that is not
                rc, msg = call(qb.handle, t64.handle, bad_nq.handle, cap=-1, dev=dev)
                assert rc == EINVAL and "dim mismatch" in msg, msg
                rc, msg = call(qb.handle, hb.handle, bad_nq.handle, dev=dev)
                assert rc == EINVAL and ("mismatch" in msg), msg
                # (3) the mask, in front of cap and the outputs
                for m, word in ((foreign, "another context"), (bad_nq, "query rows"), (bad_nt, "train rows"), (cm, "made for a collection")):
                    rc, msg = call(qb.handle, tb.handle, m.handle, cap=-1, o=None, dev=dev)
                    assert rc == EINVAL and word in msg, (word, msg)
                # (4) cap and the outputs
                for kw, word in ((dict(cap=-1), "cap is negative"), (dict(o=None), "offsets is NULL"), (dict(i=None), "NULL with cap > 0"),
                                 (dict(d=None), "NULL with cap > 0")):
                    rc, msg = call(qb.handle, tb.handle, ok.handle, dev=dev, **kw)
                    assert rc == EINVAL and word in msg, (word, msg)
            # the device form refuses host pointers (fm_radius_match_dev's pointer checks)
            rc, msg = call(qb.handle, tb.handle, ok.handle, dev=True)
            assert rc == EINVAL and "d_offsets" in msg, msg
            assert (off == -7).all() and (idx == -9).all() and (dist == -9.0).all() and tot.value == -5      # refused calls write nothing
            rc, msg = call(qb.handle, tb.handle, ok.handle, cap=0, i=None, d=None)
            assert rc == 0 and off[0] == 0 and tot.value == off[-1]
    finally:
        coll.close()
        other.close()
        for b in (qb, tb, t64, hb):
            b.close()


def test_float32_all_path_is_what_the_f32all_set_takes(ctx):
    """The f32all pair's scales lie 45 binades apart (the filter takes 40): nothing but the mask and the exact rescoring decide.
    A mask that permits one row per query row then lists at most that row."""
    Q, T = M.data("f32all")
    qb, tb = ctx.bank(Q, float_route=True), ctx.bank(T, float_route=True)
    try:
        Mp = np.zeros((M.NQ, M.NT), bool)
        Mp[np.arange(M.NQ), (np.arange(M.NQ) * 7) % M.NT] = True
        with ctx.mask(M.NQ, M.NT) as mk:
            got = ctx.radius_match_masked(qb, tb, mk.set(Mp), INF)
        M.same_pair(got, M.want("f32all", INF, Mp), "f32all, one row each")
        assert np.array_equal(np.diff(got[0]), np.ones(M.NQ, np.int64))
    finally:
        qb.close()
        tb.close()
