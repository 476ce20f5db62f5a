"""GPU: banks that grew by appends (fm_bank_append_u8 / fm_bank_append_f32) in every dense entry point, bit for bit against
tests/grown_ref.py.  An append starts on a multiple of 32 rows; the rows skipped before it are padding rows INSIDE the
bank, below its row count, and the header promises that they are never anybody's neighbour.  The matrix-core sweeps keep that
by value (a padding row's accumulator start); kernels that mask padding by index (row < n) have to know about the gaps.

Data: uniform bytes / N(0, 1) rows, on which a gap row (uint8: every byte 128; float32: zeros) is nearer than every real
row for EVERY row of the other bank (test_grown_banks_host.py checks that in float64) -- a kernel that scores a gap row
returns it at nearly every row -- and a SIFT-like set with planted matches, where gap rows must simply be absent.

Three witnesses per call with the grown bank as the train side: the reference on the real rows with the indices remapped,
no gap row among the indices, and the same call on a fresh bank of the real rows.  With the grown bank as the query side
only the output rows of real rows are specified (a gap position is an output row like any other): those are compared, the
others must hold a valid index or -1."""
import ctypes
import os
import sys

import numpy as np
import pytest

from fastmatch_amd import _ffi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grown_ref as gr          # noqa: E402
import kat                      # noqa: E402

pytestmark = pytest.mark.gpu

INF = float("inf")
ROUTES = [("u8", 1), ("f32", 0), ("f32", 2)]              # (kind, the option "f32_filter": 0 = all pairs by K5, 2 = fp16 filter always)
ROUTE_IDS = ["u8", "f32-nofilter", "f32-filter"]
TAU = 0.9


def _bits(a):
    a = np.asarray(a)
    if a.dtype == np.float32:
        return a.view(np.uint32)
    if a.dtype == np.float64:
        return a.view(np.uint64)
    return a


def _equal(got, want):
    """Tuples of arrays: shapes, integers exactly, floats as bit patterns."""
    if len(got) < len(want):
        return False
    for g, w in zip(got, want):
        g, w = np.asarray(g), np.asarray(w)
        if g.shape != w.shape or not np.array_equal(_bits(np.ascontiguousarray(g)), _bits(np.ascontiguousarray(w))):
            return False
    return True


def _fresh(ctx, kind, rows):
    return ctx.bank(rows, float_route=kind == "f32")


def _grown(ctx, kind, lay, rows, scale_like):
    """The bank of ``rows`` appended in the layout's pieces; every *first_row is checked against the reference arithmetic."""
    dim = rows.shape[1]
    if kind == "u8":
        b = ctx.bank_with_capacity(np.zeros((0, dim), np.uint8), lay.n_phys + 70)
    else:
        b = ctx.bank_f32_with_capacity(dim, lay.n_phys + 70, scale_like)
    for part, first in zip(lay.split(rows), lay.first):
        assert b.append(part) == first
    assert b.n == lay.n_phys
    return b


class _Case(object):
    """One (route, pattern, dim, data, side): the banks, the dense matrices, and the bookkeeping of the three witnesses."""

    def __init__(self, ctx, kind, pattern, dim, data, side, rows=None):
        self.ctx, self.kind, self.side = ctx, kind, side
        self.lay, self.G, self.O = rows if rows is not None else gr.dataset(kind, pattern, dim, data)
        self.other = _fresh(ctx, kind, self.O)
        self.grown = _grown(ctx, kind, self.lay, self.G, self.other)
        self.fresh = _fresh(ctx, kind, self.G)
        self.failures = []
        if side == "train":
            self.Q, self.T, self.q, self.t, self.tf, self.qf = self.O, self.G, self.other, self.grown, self.fresh, self.other
        else:
            self.Q, self.T, self.q, self.t, self.tf, self.qf = self.G, self.O, self.grown, self.other, self.other, self.fresh
        self.nt_phys = self.t.n

    def close(self):
        for b in (self.other, self.grown, self.fresh):
            b.close()

    def mask_phys(self, M):
        """A mask over the real rows as the mask of the physical banks: every pair with a gap row PERMITTED."""
        lay = self.lay
        if self.side == "train":
            P = np.ones((M.shape[0], lay.n_phys), np.uint8)
            P[:, lay.phys] = M
        else:
            P = np.ones((lay.n_phys, M.shape[1]), np.uint8)
            P[lay.phys] = M
        return P

    def check(self, name, shape, call, want, call_fresh=None):
        """call(q, t) on the grown pair against ``want`` (computed on the real rows) and against call on the fresh pair."""
        lay = self.lay
        try:
            got = call(self.q, self.t)
            fresh = (call_fresh or call)(self.qf, self.tf)
        except _ffi.FastMatchHipError as e:
            self.failures.append("%s: %s" % (name, e))
            return
        col = 0 if shape == "lists" else 1                      # where the train indices sit
        if self.side == "train":
            want_p = lay.lists_train(want) if shape == "lists" else lay.rows_train(want)
            fresh_p = lay.lists_train(fresh) if shape == "lists" else lay.rows_train(fresh)
            if np.isin(got[col], lay.gaps).any():
                self.failures.append(name + ": a gap row among the train indices")
            got_r = got
        else:
            want_p, fresh_p = want, fresh
            idx = np.asarray(got[col])
            if not ((idx >= -1) & (idx < self.nt_phys)).all():
                self.failures.append(name + ": an index outside [-1, nt)")
            got_r = lay.lists_query(got) if shape == "lists" else lay.rows_query(got)
        if not _equal(got_r, want_p):
            self.failures.append(name + ": differs from the reference")
        if not _equal(got_r, fresh_p):
            self.failures.append(name + ": differs from the fresh bank")


def _xcheck(ctx):
    def f(q, t):
        ti, d = ctx.xcheck1(q, t)
        return ti.reshape(-1, 1), d.reshape(-1, 1)
    return f


def _xcheck_keys(ctx):
    """fm_xcheck1_keys' election keys (float32 distance bits << 32 | train row, all ones = unmatched) as LISTS."""
    def f(q, t):
        k = ctx.xcheck1_keys(q, t)
        none = k == np.uint64(0xffffffffffffffff)
        ti = np.where(none, -1, (k & np.uint64(0xffffffff)).astype(np.int64)).astype(np.int32)
        d = np.where(none, np.float32(np.inf), (k >> np.uint64(32)).astype(np.uint32).view(np.float32))
        return ti.reshape(-1, 1), d.reshape(-1, 1)
    return f


def _match_ratio(ctx):
    def f(q, t):
        ti, d = ctx.match_ratio(q, t, 0.8)[:2]
        return ti.reshape(-1, 1), d.reshape(-1, 1)
    return f


def _radii(c):
    """(scalar radius, per-row radii): the scalar above every gap-row distance and above the median third neighbour; the array
    just above each row's fifth real neighbour (adversarial data: beyond the gap rows, then), with 0, a negative value, NaN and
    +inf (every train row, every gap row included in a kernel that lists them) at several rows."""
    ref = gr.radius_coll_ref.Ref(c.Q, (c.T,))
    other = np.asarray(c.O, np.float64)
    dgap = np.sqrt(((other - gr.gap_row(c.kind, other.shape[1])[None, :]) ** 2).sum(1)).max()
    scalar = np.float32(max(float(ref.kth(3)), 1.001 * dgap))
    rows = np.nextafter(ref.dist[:, 5], np.float32(np.inf)).astype(np.float32)
    for j, v in enumerate((0.0, -3.0, np.nan, np.inf)):
        rows[7 + j::41] = v
    return scalar, rows


def _dense_calls(c):
    """Every dense entry point on the case's pair."""
    ctx, Q, T = c.ctx, c.Q, c.T
    c.check("fm_knn2", "lists", ctx.knn2, gr.ref_knn(Q, T, 2))
    for k in (1, 2, 3, 8):
        c.check("fm_knn k=%d" % k, "lists", lambda q, t: ctx.knn(q, t, k), gr.ref_knn(Q, T, k))
    c.check("fm_xcheck1", "lists", _xcheck(ctx), gr.ref_xcheck1(Q, T))
    c.check("fm_knn2_ratio", "rows", lambda q, t: ctx.knn2_ratio(q, t, TAU), gr.ref_knn2_ratio(Q, T, TAU))
    for sym in (False, True):
        c.check("fm_mutual_ratio symmetric=%d" % sym, "rows", lambda q, t: ctx.mutual_ratio(q, t, TAU, sym),
                gr.ref_mutual_ratio(Q, T, TAU, sym))
    r_all, r_rows = _radii(c)
    c.check("fm_radius_match scalar", "rows", lambda q, t: gr.radius_rows(ctx.radius_match(q, t, r_all)), gr.ref_radius(Q, T, r_all))
    r_phys = r_rows
    if c.side == "query":                                       # one radius per PHYSICAL query row; a gap position gets +inf
        r_phys = np.full(c.lay.n_phys, np.inf, np.float32)
        r_phys[c.lay.phys] = r_rows
    c.check("fm_radius_match per row", "rows", lambda q, t: gr.radius_rows(ctx.radius_match(q, t, r_phys)), gr.ref_radius(Q, T, r_rows),
            lambda q, t: gr.radius_rows(ctx.radius_match(q, t, r_rows)))
    # masks: all ones through fm_mask_set_all and through fm_mask_set_u8, and a random one whose gap pairs are all permitted
    rng = np.random.default_rng(77)
    ones = np.ones((len(Q), len(T)), np.uint8)
    rnd = (rng.random((len(Q), len(T))) < 0.3).astype(np.uint8)
    rnd[5] = 0                                                  # a row without permitted pairs
    keep = ctx.get_option("masked_mfma")
    try:
        for mname, M in (("set_all", None), ("ones", ones), ("random", rnd)):
            Mr = ones if M is None else M
            with ctx.mask(c.q.n, c.t.n) as mg, ctx.mask(c.qf.n, c.tf.n) as mf:
                if M is None:
                    mg.set_all(True)
                    mf.set_all(True)
                else:
                    mg.set(c.mask_phys(M))
                    mf.set(M)
                for k in (2, 3):
                    want = gr.ref_knn_masked(Q, T, Mr, k)
                    for mfma in (0, 1):
                        ctx.set_option("masked_mfma", mfma)
                        c.check("fm_knn_masked %s k=%d masked_mfma=%d" % (mname, k, mfma), "lists",
                                lambda q, t: ctx.knn_masked(q, t, mg, k), want, lambda q, t: ctx.knn_masked(q, t, mf, k))
    finally:
        ctx.set_option("masked_mfma", keep)
    # self distances of the grown bank, and fm_match_accepted with self distances attached to the query bank
    sd_want = gr.ref_self_dist(c.G)
    sd = ctx.self_dist(c.grown)
    if sd.shape != (c.lay.n_phys,) or not np.array_equal(_bits(sd[c.lay.phys]), _bits(sd_want)):
        c.failures.append("fm_self_dist: differs from the reference")
    if not np.array_equal(_bits(sd[c.lay.phys]), _bits(ctx.self_dist(c.fresh))):
        c.failures.append("fm_self_dist: differs from the fresh bank")
    sdq = gr.ref_self_dist(Q)
    c.qf.set_selfdist(sdq)
    if c.side == "train":
        c.q.set_selfdist(sdq)
    else:
        full = np.ones(c.lay.n_phys, np.float64)
        full[c.lay.phys] = sdq
        c.q.set_selfdist(full)
    c.check("fm_match_accepted", "rows", lambda q, t: ctx.match_accepted(q, t, 0.8), gr.ref_match_accepted(Q, T, sdq, 0.8))
    c.check("fm_match_ratio", "lists", _match_ratio(ctx), gr.ref_xcheck1(Q, T))
    c.check("fm_xcheck1_keys", "lists", _xcheck_keys(ctx), gr.ref_xcheck1(Q, T))


@pytest.mark.parametrize("side", ["train", "query"])
@pytest.mark.parametrize("data", ["adv", "sift"])
@pytest.mark.parametrize("dim", [128, 61])
@pytest.mark.parametrize("pattern", sorted(gr.PATTERNS))
@pytest.mark.parametrize("route", ROUTES, ids=ROUTE_IDS)
def test_dense_calls_on_a_grown_bank(ctx, route, pattern, dim, data, side):
    kind, filt = route
    keep = ctx.get_option("f32_filter")
    ctx.set_option("f32_filter", filt)
    c = _Case(ctx, kind, pattern, dim, data, side)
    try:
        _dense_calls(c)
    finally:
        ctx.set_option("f32_filter", keep)
        c.close()
    print("\n".join(c.failures))
    assert c.failures == []


@pytest.mark.parametrize("side", ["train", "query"])
def test_float32_root_ties_are_repaired_without_gap_rows(ctx, side):
    """Integer-route banks whose every distance lies where two d2 share a float32 root (kat.far_banks, d2 ~ 6.5e6): the lists
    and elections are redone by an exact rescan of ALL rows of the other bank, by index.  A gap row (d2 ~ 2.1e6 to every row
    here) must not come out of that rescan either."""
    lay = gr.Layout(gr.PATTERNS["in_stage"])
    rng = np.random.default_rng(7300)
    if side == "train":
        O, G = kat.far_banks(gr.N_OTHER, lay.n_real, rng)
    else:
        G, O = kat.far_banks(lay.n_real, gr.N_OTHER, rng)
    assert gr.gap_is_nearest("u8", G, O).all()
    c = _Case(ctx, "u8", None, 128, None, side, rows=(lay, G, O))
    try:
        c.check("fm_knn2", "lists", ctx.knn2, gr.ref_knn(c.Q, c.T, 2))
        c.check("fm_knn k=1", "lists", lambda q, t: ctx.knn(q, t, 1), gr.ref_knn(c.Q, c.T, 1))
        c.check("fm_knn k=3", "lists", lambda q, t: ctx.knn(q, t, 3), gr.ref_knn(c.Q, c.T, 3))
        c.check("fm_xcheck1", "lists", _xcheck(ctx), gr.ref_xcheck1(c.Q, c.T))
        c.check("fm_knn2_ratio", "rows", lambda q, t: ctx.knn2_ratio(q, t, INF), gr.ref_knn2_ratio(c.Q, c.T, INF))
        for sym in (False, True):
            c.check("fm_mutual_ratio symmetric=%d" % sym, "rows", lambda q, t: ctx.mutual_ratio(q, t, INF, sym),
                    gr.ref_mutual_ratio(c.Q, c.T, INF, sym))
    finally:
        c.close()
    print("\n".join(c.failures))
    assert c.failures == []


@pytest.fixture
def rescan_ctx(monkeypatch):
    """A context of its own that filters every float32 call ("f32_filter" = 2) and reports, with its filter statistics, how many
    output rows got a per-row exact rescan (the debug line of fm_f32_filter_stats on stderr)."""
    import fastmatch_amd
    monkeypatch.setenv("FM_F32_FILTER", "2")
    monkeypatch.setenv("FM_F32_DEBUG", "1")
    c = fastmatch_amd.Context(0)
    yield c
    c.close()


def _filter_counts(c, capfd):
    """(filtered launches, calls redone by the all-pairs kernel, output rows rescanned so far)"""
    import re
    capfd.readouterr()
    launches, redone = c.f32_filter_stats()
    m = re.search(r"redone by K5 (\d+), output rows rescanned (\d+)", capfd.readouterr().err)
    assert m is not None and int(m.group(1)) == redone
    return launches, redone, int(m.group(2))


@pytest.mark.parametrize("side", ["train", "query"])
def test_per_row_rescans_of_the_filter_route_skip_gap_rows(rescan_ctx, capfd, side):
    """The fp16 filter route has three endings: rescoring of the filter's candidates, a per-row exact rescan of the output rows
    whose lists may be incomplete, a whole-call redo by the all-pairs kernel.  The rescan goes over the other bank's rows by
    index.  gr.rescan_dataset makes EVERY row of the fresh bank need one against the grown bank (a hundred tiny rows within
    the margin of each other, the zero row nearer than all of them), as the train side of the forward sweep or as the
    query side of a cross-check's reverse sweep, and the tiny rows need one in fm_self_dist.  Asserted besides the results:
    rescans happened, as many as the data say, and no call was redone by the all-pairs kernel."""
    c = rescan_ctx
    lay, G, O, small = gr.rescan_dataset()
    case = _Case(c, "f32", None, 128, None, side, rows=(lay, G, O))
    Q, T = case.Q, case.T
    nflag = gr.RESCAN_OTHER                                        # output rows of the sweep that reduces over the grown bank
    try:
        _, redone0, rows0 = _filter_counts(c, capfd)
        if side == "train":
            case.check("fm_knn2", "lists", c.knn2, gr.ref_knn(Q, T, 2))
            _, redone, rows1 = _filter_counts(c, capfd)
            assert redone == redone0 and rows1 - rows0 >= 2 * nflag          # (the grown pair and the fresh pair: one sweep each)
            case.check("fm_knn k=1", "lists", lambda q, t: c.knn(q, t, 1), gr.ref_knn(Q, T, 1))
            case.check("fm_knn2_ratio", "rows", lambda q, t: c.knn2_ratio(q, t, INF), gr.ref_knn2_ratio(Q, T, INF))
        case.check("fm_xcheck1", "lists", _xcheck(c), gr.ref_xcheck1(Q, T))
        _, redone, rows2 = _filter_counts(c, capfd)
        assert redone == redone0 and rows2 - rows0 >= 2 * nflag
        for sym in (False, True):
            case.check("fm_mutual_ratio symmetric=%d" % sym, "rows", lambda q, t: c.mutual_ratio(q, t, INF, sym),
                       gr.ref_mutual_ratio(Q, T, INF, sym))
        sdq = gr.ref_self_dist(Q)
        case.qf.set_selfdist(sdq)
        full = np.ones(case.q.n, np.float64)
        full[lay.phys if side == "query" else np.arange(case.q.n)] = sdq
        case.q.set_selfdist(full)
        case.check("fm_match_accepted", "rows", lambda q, t: c.match_accepted(q, t, INF), gr.ref_match_accepted(Q, T, sdq, INF))
        _, _, rows3 = _filter_counts(c, capfd)
        sd = c.self_dist(case.grown)
        _, redone, rows4 = _filter_counts(c, capfd)
        assert redone == redone0 and rows4 - rows3 >= len(small)              # every tiny row, at the least
        if not np.array_equal(_bits(sd[lay.phys]), _bits(gr.ref_self_dist(G))):
            case.failures.append("fm_self_dist: differs from the reference")
        if not np.array_equal(_bits(sd[lay.phys]), _bits(c.self_dist(case.fresh))):
            case.failures.append("fm_self_dist: differs from the fresh bank")
    finally:
        case.close()
    print("\n".join(case.failures))
    assert case.failures == []


@pytest.mark.parametrize("route", ROUTES, ids=ROUTE_IDS)
def test_device_forms_equal_the_host_forms(ctx, route):
    import torch
    kind, filt = route
    keep = ctx.get_option("f32_filter")
    ctx.set_option("f32_filter", filt)
    c = _Case(ctx, kind, "in_stage" if kind == "u8" else "across", 128, "adv", "train")
    try:
        nq = c.q.n
        for k in (1, 2, 3, 8):
            idx = torch.full((nq, k), -7, dtype=torch.int32, device="cuda")
            dist = torch.full((nq, k), -7.0, dtype=torch.float32, device="cuda")
            ctx.knn_dev(c.q, c.t, k, idx.data_ptr(), dist.data_ptr(), consumer_stream=torch.cuda.current_stream().cuda_stream)
            want = ctx.knn(c.q, c.t, k)
            assert _equal((idx.cpu().numpy(), dist.cpu().numpy()), want), "fm_knn_dev k=%d" % k
            assert _equal(want, c.lay.lists_train(gr.ref_knn(c.Q, c.T, k))), "fm_knn k=%d" % k
        ti = torch.full((nq,), -7, dtype=torch.int32, device="cuda")
        d = torch.full((nq,), -7.0, dtype=torch.float32, device="cuda")
        ctx.xcheck1_dev(c.q, c.t, ti.data_ptr(), d.data_ptr(), consumer_stream=torch.cuda.current_stream().cuda_stream)
        want = ctx.xcheck1(c.q, c.t)
        assert _equal((ti.cpu().numpy(), d.cpu().numpy()), want), "fm_xcheck1_dev"
        assert not np.isin(want[0], c.lay.gaps).any()
        rows = torch.full((nq, 3), -7, dtype=torch.int32, device="cuda")
        count = torch.full((1,), -7, dtype=torch.int64, device="cuda")
        total = ctx.knn2_ratio_dev(c.q, c.t, TAU, rows.data_ptr(), count.data_ptr(), nq, want_count=True,
                                   consumer_stream=torch.cuda.current_stream().cuda_stream)
        want = ctx.knn2_ratio(c.q, c.t, TAU)
        m = want[0].shape[0]
        assert total == m == int(count.item())
        got = rows[:m].cpu().numpy()
        assert np.array_equal(got[:, 0], want[0]) and np.array_equal(got[:, 1], want[1])
        assert np.array_equal(got[:, 2].view(np.uint32), _bits(want[2])), "fm_knn2_ratio_dev"
        assert _equal(want, c.lay.rows_train(gr.ref_knn2_ratio(c.Q, c.T, TAU)))
    finally:
        ctx.set_option("f32_filter", keep)
        c.close()


def test_refusals_are_what_they_are_for_fresh_banks(ctx):
    """A grown bank is refused wherever its kind is refused today, with the same code, and answers afterwards."""
    lay, G, O = gr.dataset("u8", "across", 128, "sift")
    _, Gf, Of = gr.dataset("f32", "across", 128, "sift")
    q8, qf = ctx.bank(O), ctx.bank(Of, float_route=True)
    g8, gf = _grown(ctx, "u8", lay, G, None), _grown(ctx, "f32", lay, Gf, qf)
    f8, ff = ctx.bank(G), ctx.bank(Gf, float_route=True)
    bb = ctx.bank_binary(np.zeros((4, 32), np.uint8))
    lib, h = ctx.lib, ctx.handle
    idx, dist = np.zeros((400, 8), np.int32), np.zeros((400, 8), np.float32)
    off, tot = np.zeros(401, np.int64), ctypes.c_int64(0)
    first = ctypes.c_int64(0)
    try:
        calls = [
            lambda x, y: lib.fm_knn2(h, x.handle, y.handle, _ffi._ptr(idx), _ffi._ptr(dist)),
            lambda x, y: lib.fm_knn(h, x.handle, y.handle, 3, _ffi._ptr(idx), _ffi._ptr(dist)),
            lambda x, y: lib.fm_xcheck1(h, x.handle, y.handle, _ffi._ptr(idx), _ffi._ptr(dist)),
            lambda x, y: lib.fm_radius_match(h, x.handle, y.handle, None, 100.0, 0, _ffi._ptr(off), None, None, ctypes.byref(tot)),
        ]
        # (other bank, grown bank, the fresh bank of the grown one's rows): kinds that do not pair
        for other, grown, fresh in ((qf, g8, f8), (q8, gf, ff), (bb, g8, f8), (bb, gf, ff)):
            for call in calls:
                rc = call(other, grown)
                assert rc != 0 and rc == call(other, fresh)
                rc = call(grown, other)
                assert rc != 0 and rc == call(fresh, other)
        # a wide bank and a binary bank take no appends; a bank whose capacity is used up takes none either
        assert lib.fm_bank_append_u8(h, bb.handle, _ffi._ptr(np.zeros((1, 32), np.uint8)), 1, ctypes.byref(first)) != 0
        assert lib.fm_bank_append_u8(h, g8.handle, _ffi._ptr(np.zeros((200, 128), np.uint8)), 200, ctypes.byref(first)) != 0
        assert g8.n == lay.n_phys
        assert _equal(ctx.knn(q8, g8, 3), lay.lists_train(gr.ref_knn(O, G, 3)))
        assert _equal(ctx.knn(qf, gf, 3), lay.lists_train(gr.ref_knn(Of, Gf, 3)))
    finally:
        for b in (q8, qf, g8, gf, f8, ff, bb):
            b.close()


def _lazy_runs(ctx, feat, monkeypatch, taus):
    """The lazy device loop on a pixel target (the helpers of test_config1_plumbing.py, on a smaller image) with
    "expand_delegate" at its default and at 1 -- every round's cross-check handed to the dense kernels, on a target bank that
    grows cell by cell.  Returns the two match lists per tau, the appends the target banks saw, and the delegated rounds."""
    from fastmatch_amd import cache, fastmatch, imaging
    from imagegen import texture, warp
    img1 = texture(480, 400, seed=1)
    mild = np.array([[1.0, 0.01, 12.0], [-0.008, 1.0, -7.0], [1e-5, -5e-6, 1.0]])
    img4 = warp(img1, mild)
    kq, dq = feat(img4)
    thumb_q = imaging.get_thumbnail(img4, (360, 360))
    ktq, dtq = feat(thumb_q)
    pos = lambda kp: np.array([k.pt for k in kp], dtype=np.float64).reshape(-1, 2)
    mc = cache.Metric_Cache.from_arrays(dq, pos(kq), (480, 400), dtq, pos(ktq), (thumb_q.shape[1], thumb_q.shape[0]),
                                        options={"context": ctx})
    appends = []
    plain = _ffi.Bank.append

    def recording(self, rows):
        before = self.n
        first = plain(self, rows)
        appends.append((before, first, len(rows)))
        return first
    monkeypatch.setattr(_ffi.Bank, "append", recording)
    keep = ctx.get_option("expand_delegate")
    out = []
    try:
        for deleg in (keep, 1):
            ctx.set_option("expand_delegate", deleg)
            ctx.set_option("delegated_rounds", 0)
            st = {}
            run = fastmatch.match(mc, img1, {"context": ctx, "feature_function": feat, "stats": st, "radius": 200})
            out.append([run(tau) for tau in taus])
            assert st.get("device_loops") == len(taus) and "device_fallbacks" not in st
            delegated = ctx.get_option("delegated_rounds")
    finally:
        ctx.set_option("expand_delegate", keep)
    return out[0], out[1], appends, delegated


@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_delegated_rounds_of_the_lazy_loop_on_a_grown_target(ctx, monkeypatch, kind):
    """The lazy loop with every round's cross-check delegated to the dense kernels equals the loop that delegates none.  What
    this does NOT cover: the target bank grows as the loop happens to reach its cells, not in the append patterns above, and
    a delegated round works on a view of ONE cell's rows (bank_rows_view: one append, no interior gap, no real-row bitmap)
    against gathered query rows -- so the dense kernels never see the bank's gaps here and the bitmap is not exercised.  The
    test pins that the delegated path stays indifferent to a grown target; the bitmap's readers are tested above."""
    from fastmatch_amd import standin

    def feat(data):
        kp, ds = standin.standin_features(data)
        if kind == "u8" or ds is None or len(ds) == 0:
            return kp, ds
        d = np.asarray(ds, dtype=np.float32)
        return kp, np.sqrt(d / np.maximum(d.sum(axis=1, keepdims=True), 1.0)).astype(np.float32)
    base, deleg, appends, delegated = _lazy_runs(ctx, feat, monkeypatch, (0.8, 0.95))
    # the target bank really grew with gaps inside it: an append that started above the rows the bank had, and more after it
    gaps = [i for i, (before, first, n) in enumerate(appends) if n > 0 and first > before > 0]
    assert gaps and gaps[0] < len(appends) - 1
    assert delegated > 5
    for got, want in zip(deleg, base):
        assert len(got) == len(want) > 10
        for (ia, da), (ib, db) in zip(got, want):
            assert ia == ib and da["ratio"] == db["ratio"] and np.array_equal(da["positions"], db["positions"])
