"""GPU: the fp16 filters' margins from below -- planted pairs whose fp16 rounding errors all point against the exact order
(tests/f16_margin_ref.py; tests/test_f16_margin_host.py checks the inputs and the decision model on the CPU).

M = eps (|c|^2 + max |m|^2) must cover twice the filter's score error.  Random data realises a tenth of that error, so a margin of
half the size, an ldexpf with the wrong sign, a maximum left over from before an append or a site with another constant all pass
every other file of the suite.  Here the competitor's fp16 score beats the true neighbour's by 0.58 M (K8) / 0.51 M (K14), and a
radius hit lies 0.89 M over r^2 in fp16: each family is kept by the margin as derived and lost by one of half the size.  The
sites that apply M and what reaches them:
  K8's stream test                  t1 behind t2 in stream order (PLACES: rows 255, 299, 133)
  K8's end-of-piece list test, rescore_kernel's thr
                                    t1 in front of t2: it sits in a lane's entries when the bound rises ("f32_nsplit" 1 fuses the
                                    rescoring into the sweep, 3 and 7 leave it to rescore_kernel)
  tri_rescore_kernel's thr          fm_self_dist under "self_tri" 2, the planted row a streamed row of the piece
  radius_limits_kernel              the threshold form, scalar and per-row radii, host and device forms, bank and collection
  the wide filter's push, wide_rescore_kernel's drop
                                    the same places at 129, 160 and 256 values, the match graph and the outside-query forms
  eps_c, eps_nm, aux_mul, nscale    banks of different powers of two, both signs
  nm_max                            a bank that grew and collections whose first images have small norms (the doubled form,
                                    whose margin is two thirds max |m|^2)
Which sweep meets which family: fm_knn's k = 1 is the first column of the top-2 sweep (fm_knn2, fm_knn2_ratio, fm_mutual_ratio), and
fm_xcheck1 is one reverse top-1 sweep.  The (t1, t2) families pin the top-1 sweeps, with the banks exchanged; the (t0, t1, t2) and,
up to 128 values, (t1, t2, t3) families the top-2 sweeps, the latter the only ones a k = 1 result can show a loss through.  K14's
bound is per lane group: t0 lies in t2's group of four rows (f16_margin_ref.PLACES).
NOT pinned: the float32 round of the expansion loop (round_body_f32.h) applies the same eps_c / eps_nm; it is out of scope here.

Every result is compared bit for bit with the oracle's order-1 chain (wide_ref, xcheck_each_ref, wide_pairs_ref, wide_query_ref,
radius_coll_ref compose it), never with another entry point.  The filter is forced ("f32_filter" 2) and every call asserts from
f32_filter_stats that it ran and that no sweep fell back to the exact kernel, which would hide a lost row.  (radiusMatch has no
fallback and no option: its fp16 sweep runs whenever filter_usable says so -- finite values, scales within the window.)"""
import numpy as np
import pytest

import oracle
import f16_margin_ref as R
import radius_coll_ref as RC
import wide_pairs_ref
import wide_query_ref
import wide_ref
import xcheck_each_ref
from fastmatch_amd import _ffi

pytestmark = pytest.mark.gpu

TAU = 0.8
OPTIONS = ("f32_filter", "f32_nsplit", "self_tri", "tri_stages")
CALLS = {"knn1": lambda c, q, t: c.knn(q, t, 1), "knn2": lambda c, q, t: c.knn2(q, t),
         "ratio": lambda c, q, t: c.knn2_ratio(q, t, TAU), "xcheck1": lambda c, q, t: c.xcheck1(q, t),
         "mutual0": lambda c, q, t: c.mutual_ratio(q, t, TAU, False), "mutual1": lambda c, q, t: c.mutual_ratio(q, t, TAU, True)}
PAIR = ("knn1", "knn2", "ratio", "xcheck1", "mutual0", "mutual1")
BACK = ("xcheck1", "mutual0", "mutual1")
FORWARD = ("knn1", "knn2", "ratio")             # the calls without a reverse sweep
_WANT = {}
_CHECKED = {}


@pytest.fixture
def fctx(ctx):
    saved = {k: ctx.get_option(k) for k in OPTIONS}
    ctx.set_option("f32_filter", 2)
    yield ctx
    for k, v in saved.items():
        ctx.set_option(k, v)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same(got, want, what):
    got = got if isinstance(got, (tuple, list)) else (got,)
    want = want if isinstance(want, (tuple, list)) else (want,)
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype, (what, i, g.shape, w.shape, g.dtype, w.dtype)
        assert np.array_equal(_bits(g), _bits(w)), (what, i)


def _filtered(c, call, ran=True):
    """The call's result; the filter answered it by itself (ran False: it was not asked at all)."""
    l0, f0 = c.f32_filter_stats()
    out = call()
    l1, f1 = c.f32_filter_stats()
    assert (l1 > l0) == ran and f1 == f0, ("filter launches, sweeps redone by the exact kernel", l1 - l0, f1 - f0)
    return out


class _Tally(list):
    """Every call of a test is made and the failed ones are named together: a failure says which sweeps lost a row."""

    def check(self, what, fn):
        try:
            fn()
        except AssertionError as e:
            self.append((what, (str(e).splitlines() or [""])[0][:160]))

    def done(self):
        if self:
            raise AssertionError("failed calls:\n" + "\n".join("  %s: %s" % (w, m) for w, m in self))


def _want(name, Q, T):
    if name not in _WANT:
        _WANT[name] = {"knn1": wide_ref.knn(Q, T, 1), "knn2": wide_ref.knn(Q, T, 2), "xcheck1": wide_ref.xcheck1(Q, T),
                       "ratio": wide_ref.ratio_match(Q, T, TAU), "mutual0": wide_ref.mutual_ratio(Q, T, TAU, False),
                       "mutual1": wide_ref.mutual_ratio(Q, T, TAU, True)}
    return _WANT[name]


def _checked(name, p, eps, floor):
    """The host conditions of a set, asserted once in front of its first upload."""
    if name not in _CHECKED:
        _CHECKED[name] = R.check_competitor(p, eps, floor)
    return p


def _kept(p, name, got):
    """The planted rows in a k-NN result: the first assertion a lost t1 trips."""
    if name not in ("knn1", "knn2"):
        return
    idx = got[0]
    for f in p.fams:
        row = idx[f["q"]].tolist()
        if f["t0"] is None:
            assert row[0] == f["t1"], ("lost t1", name, f, row)
            assert name == "knn1" or row[1] == f["t2"], ("lost t2", name, f, row)
        elif name == "knn2":
            assert row == [f["t0"], f["t1"]], ("lost t1", name, f, row)


def _pair_calls(c, name, p, qb, tb, calls=PAIR, ran=True, tally=None):
    want = _want(name, p.Q, p.T)
    mine = _Tally() if tally is None else tally

    def one(k):
        got = _filtered(c, lambda: CALLS[k](c, qb, tb), ran)
        _kept(p, k, got)
        _same(got, want[k], (name, k))

    for k in calls:
        mine.check((name, k), lambda: one(k))
    # the planted rows are in the accepted lists: t0 at 0.44 of t1 passes the ratio test, and its ratio is t1's
    if "ratio" in calls and p.fams:
        assert set(f["q"] for f in p.fams if f["t0"] is not None) <= set(want["ratio"][0].tolist())
    if tally is None:
        mine.done()


def _both_ways(c, name, p, calls=PAIR, kind=_ffi.FM_BANK_F32, back=None):
    """The set forward (the planted q an output row of the forward top-2 sweep: fm_knn's k = 1 is the first column of the 2-NN
    lists, so that sweep serves knn, knn2, knn2_ratio and mutual_ratio, and the top-2 families pin it) and with the banks
    exchanged (fm_xcheck1 and mutual_ratio's other half are ONE reverse top-1 sweep, output rows = train rows: there the planted
    q is an output row of it and the top-1 families pin it)."""
    qb, tb = c.bank(p.Q), c.bank(p.T)
    tally = _Tally()
    try:
        assert qb.kind == tb.kind == kind
        _pair_calls(c, name, p, qb, tb, calls, tally=tally)
        back = (BACK if calls == PAIR else ()) if back is None else back
        if back:
            _pair_calls(c, name + " exchanged", R.swapped(p), tb, qb, back, tally=tally)
    finally:
        qb.close(); tb.close()
    tally.done()


# ---- 1. K8 bank pairs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nsplit", [0, 1, 3, 7])
@pytest.mark.parametrize("dim", [128, 61])
def test_k8_bank_pairs(fctx, dim, nsplit):
    p = _checked(("k8", dim), R.pair_set(dim), R.EPS_K8, R.FLOOR_K8)
    fctx.set_option("f32_nsplit", nsplit)
    _both_ways(fctx, "k8 %d" % dim, p)


# ---- 2. banks of different powers of two -------------------------------------------------------------------------------------
def test_k8_output_side_scaled_down(fctx):
    """A query row of magnitude 2^3: kc - km = -3.  A sweep that STREAMS that row has max |m|^2 at 64 times the planted rows',
    everything inside the margin, and goes to the exact kernel: so the calls of the forward top-2 sweep alone, and, with the
    banks exchanged, fm_xcheck1, whose one sweep then has the scaled bank on its output side again."""
    p = _checked(("k8", 128, "q3"), R.pair_set(128, "q3"), R.EPS_K8, R.FLOOR_K8)
    assert R.kscale(p.Q) - R.kscale(p.T) == -3
    _both_ways(fctx, "k8 q3", p, FORWARD, back=("xcheck1",))


@pytest.mark.parametrize("dim", [128, 61])
def test_k8_streamed_side_scaled_down(fctx, dim):
    """One train row with a single large value, its norm under the planted rows': kc - km = +2 (+1 at 61 values)."""
    p = _checked(("k8", dim, "t"), R.pair_set(dim, "t"), R.EPS_K8, R.FLOOR_K8)
    assert R.kscale(p.Q) - R.kscale(p.T) == (2 if dim == 128 else 1)
    _both_ways(fctx, "k8 t %d" % dim, p)


# ---- 3. state that changes nm_max ----------------------------------------------------------------------------------------------
def _stacked_knn(Q, images, k):
    """fm_collection_knn: the oracle on the stacked rows, hits mapped through the image sizes."""
    idx, dist = oracle.bf_knn(Q, np.concatenate(images), k, order=1)
    first = np.concatenate([[0], np.cumsum([len(im) for im in images])]).astype(np.int64)
    img = (np.searchsorted(first, idx, side="right") - 1).astype(np.int32)
    return img, (idx - first[img]).astype(np.int32), dist


def test_k8_bank_that_grew(fctx):
    """fm_bank_create_f32_cap + fm_bank_append_f32: 224 small-norm rows, a call, then the planted rows.  With the maximum of the
    first append in eps_nm the planted row is lost (test_f16_margin_host.py)."""
    c = fctx
    base = R.doubled_set(128)
    small = R.small_rows(224, 128, 1)
    p = _checked(("k8", "grown"), R.stacked(base, small), R.EPS_K8, R.FLOOR_K8)
    qb, like = c.bank(p.Q), c.bank(base.T)
    tb = c.bank_f32_with_capacity(128, len(p.T), like)
    try:
        assert tb.append(small) == 0
        _same(_filtered(c, lambda: c.knn2(qb, tb)), wide_ref.knn(p.Q, small, 2), "the small rows alone")
        assert tb.append(base.T) == 224 and tb.n == len(p.T)          # (a multiple of 32: no gap rows)
        tally = _Tally()
        _pair_calls(c, "k8 grown", p, qb, tb, tally=tally)
        _pair_calls(c, "k8 grown exchanged", R.swapped(p), tb, qb, BACK, tally=tally)
        tally.done()
    finally:
        for b in (qb, like, tb):
            b.close()


def _collection(c, images, wide=False):
    col = c.collection()
    for i, im in enumerate(images):
        assert (col.add_wide(im) if wide else col.add(im)) == i
    return col


@pytest.mark.parametrize("first", ["same_binade", "half"])
def test_k8_collection_with_small_images_first(fctx, first):
    """A float32 collection whose first images have small norms and whose last carries the planted rows.  "half": the first
    image's values are half the planted rows'; it fixes the stack's power of two, under which the planted rows' largest
    values lie in [2^14, 2^15) -- still fp16's range, so the filter stays on (a float32 collection never rescales)."""
    c = fctx
    base = _checked(("k8", "doubled"), R.doubled_set(128), R.EPS_K8, R.FLOOR_K8)
    s = 1.0 if first == "same_binade" else 0.5
    images = [R.small_rows(130, 128, 2, s), np.zeros((0, 128), np.float32), R.small_rows(257, 128, 3, s), np.array(base.T)]
    Q = np.array(base.Q)
    qb = c.bank(Q)
    col = _collection(c, images)
    tally = _Tally()

    def stacked_knn(k):
        got = _filtered(c, lambda: col.knn(qb, k))
        for f in base.fams:
            top = [f["t1"], f["t2"]] if f["t0"] is None else [f["t0"], f["t1"]]
            assert got[0][f["q"], k - 1] == 3 and got[1][f["q"]].tolist() == top[:k], ("lost t1", k, f, got[1][f["q"]])
        _same(got, _stacked_knn(Q, images, k), ("stacked", k))

    def mutual_each(rows, sym):
        got = _filtered(c, lambda: col.mutual_ratio_each(qb, TAU, sym))
        for i, im in enumerate(images):
            _same(got[i], wide_ref.mutual_ratio(rows, im, TAU, sym), ("mutual_ratio_each", sym, i))

    try:
        assert col.info()[3] == _ffi.FM_BANK_F32
        tally.check("knn 1", lambda: stacked_knn(1))
        tally.check("knn 2", lambda: stacked_knn(2))
        tally.check("knn2_each", lambda: _same(_filtered(c, lambda: col.knn2_each(qb)), wide_query_ref.knn2_each(Q, images), "knn2_each"))
        tally.check("xcheck1_each", lambda: _same(_filtered(c, lambda: col.xcheck1_each(qb)), xcheck_each_ref.xcheck_each(Q, images), "xcheck1_each"))
        tally.check("mutual_ratio_each", lambda: mutual_each(Q, False))
        tally.check("mutual_ratio_each symmetric", lambda: mutual_each(Q, True))
    finally:
        col.close(); qb.close()
    # the reverse sweeps: the planted q a row of the last image, the planted t rows in the query bank
    T = np.array(base.T)
    images = [R.small_rows(130, 128, 2, s), Q]
    qb = c.bank(T)
    col = _collection(c, images)
    try:
        tally.check("xcheck1_each exchanged",
                    lambda: _same(_filtered(c, lambda: col.xcheck1_each(qb)), xcheck_each_ref.xcheck_each(T, images), "xcheck1_each exchanged"))
        tally.check("mutual_ratio_each symmetric exchanged", lambda: mutual_each(T, True))
    finally:
        col.close(); qb.close()
    tally.done()


# ---- 4. self distances ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", sorted(R.SELF_PLACES))
def test_self_distances(fctx, n):
    """fm_self_dist on a float32 bank: the triangular sweep ("self_tri" 2, pieces of 4 stages) and the masked full sweep."""
    c = fctx
    p = R.self_bank(n)
    if ("self", n) not in _CHECKED:
        _CHECKED[("self", n)] = R.check_self(p)
    n_pad = (n + 127) // 128 * 128
    table, n_diag, used = _ffi.self_dist_plan(n_pad, 4)
    assert used == 4 and len(table) > n_diag                      # the plan has pieces off the diagonal ...
    if n == min(R.SELF_PLACES):
        assert len(_ffi.self_dist_plan(n_pad - 128, 4)[0]) == _ffi.self_dist_plan(n_pad - 128, 4)[1]      # ... one stage less has none
    X = np.array(p.Q)
    want = oracle.self_dist(X, order=1)
    _, d = oracle.bf_knn(X, X, 2, order=1)
    for f in p.fams:
        assert want[f["q"]] == np.float64(d[f["q"], 1])
    b = c.bank(X)
    try:
        assert b.kind == _ffi.FM_BANK_F32
        c.set_option("tri_stages", 4)
        for tri in (2, 0):
            c.set_option("self_tri", tri)
            got = _filtered(c, lambda: c.self_dist(b))
            for f in p.fams:
                assert got[f["q"]] == want[f["q"]], ("lost m1", tri, f, got[f["q"]], want[f["q"]])
            _same(got, want, ("self_dist", tri))
    finally:
        b.close()


# ---- 5. float32 radiusMatch ----------------------------------------------------------------------------------------------------
def _radii(p, r):
    """One radius per row: r at the planted rows and at every third row, 0 elsewhere."""
    rr = np.zeros(len(p.Q), np.float32)
    rr[::3] = r
    rr[[f["q"] for f in p.fams]] = r
    return rr


def _planted_lists(p, cut):
    """The reference itself holds each hit and no mirror."""
    off, _, _, _, gidx = cut
    for f in p.fams:
        mine = gidx[off[f["q"]]:off[f["q"] + 1]].tolist()
        assert mine == ([f["t"]] if f["kind"] == "hit" else []), (f, mine)


def test_radius_bank_pair(ctx):
    from test_radius_dev_gpu import _full
    p = R.radius_set()
    r, _ = R.check_threshold(p)
    Q, T = np.array(p.Q), np.array(p.T)
    ref = RC.Ref(Q, (T,))
    qb, tb = ctx.bank(Q), ctx.bank(T)
    try:
        assert qb.kind == tb.kind == _ffi.FM_BANK_F32
        for rr in (r, _radii(p, r)):
            cut = ref.cut(rr)
            _planted_lists(p, cut)
            for what, got in (("host", ctx.radius_match(qb, tb, rr)), ("device", _full(ctx, qb, tb, rr))):
                off, idx, dist = got
                for f in p.fams:
                    if f["kind"] == "hit":
                        assert idx[off[f["q"]]:off[f["q"] + 1]].tolist() == [f["t"]], ("lost hit", what, f)
                _same((off, idx, dist), (cut[0], cut[4], cut[3]), ("radius_match", what, np.ndim(rr)))
    finally:
        qb.close(); tb.close()


def test_radius_collection(ctx):
    from test_radius_dev_gpu import _full
    p = R.radius_set()
    r, _ = R.check_threshold(p)
    Q, T = np.array(p.Q), np.array(p.T)
    images = [R.small_rows(130, 128, 4, 0.5), T[:600], np.zeros((0, 128), np.float32), T[600:]]
    ref = RC.Ref(Q, images)
    qb = ctx.bank(Q)
    col = _collection(ctx, images)
    try:
        assert col.info()[3] == _ffi.FM_BANK_F32
        for rr in (r, _radii(p, r)):
            cut = ref.cut(rr)
            assert cut[0][-1] == sum(f["kind"] == "hit" for f in p.fams)
            RC.same_lists(col.radius_match(qb, rr), cut, "host form")
            RC.same_lists(_full(ctx, qb, col, rr), cut, "device form")
    finally:
        col.close(); qb.close()


# ---- 6. K14 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nsplit", [0, 3])
@pytest.mark.parametrize("dim", [129, 160, 256])
def test_k14_bank_pairs(fctx, dim, nsplit):
    p = _checked(("k14", dim), R.pair_set(dim), R.EPS_K14, R.FLOOR_K14)
    fctx.set_option("f32_nsplit", nsplit)
    _both_ways(fctx, "k14 %d" % dim, p, kind=_ffi.FM_BANK_F32W)


def test_k14_banks_of_different_powers_of_two(fctx):
    """A query row of magnitude 2^8 (kq - kt = -8, the last difference the filter takes) and of 2^9 (the exact kernel); one
    train row with a single large value (+2)."""
    c = fctx
    p = _checked(("k14", 160, "q8"), R.pair_set(160, "q8"), R.EPS_K14, R.FLOOR_K14)
    assert R.kscale(p.Q) - R.kscale(p.T) == -8
    _both_ways(c, "k14 q8", p, kind=_ffi.FM_BANK_F32W)          # (no per-row rescan here: the record list takes a streamed decoy)
    p = _checked(("k14", 160, "t"), R.pair_set(160, "t"), R.EPS_K14, R.FLOOR_K14)
    assert R.kscale(p.Q) - R.kscale(p.T) == 2
    _both_ways(c, "k14 t", p, kind=_ffi.FM_BANK_F32W)
    p = R.pair_set(160, "q9")
    assert R.kscale(p.Q) - R.kscale(p.T) == -9
    qb, tb = c.bank(p.Q), c.bank(p.T)
    try:
        _pair_calls(c, "k14 q9", p, qb, tb, FORWARD, ran=False)
    finally:
        qb.close(); tb.close()


@pytest.mark.parametrize("first", ["same_binade", "rescaled"])
def test_k14_match_graph(fctx, first):
    """fm_collection_pairs_mutual_ratio on a wide collection: the planted q in one image, its t rows in another, a small-norm
    image first.  (The doubled form: q and t share the stack, whose largest norm has to be a planted t's.)  "rescaled": the
    first image's values are 2^-4 of the planted rows', so the later adds lower the stack's power of two and remake its planes
    and its largest norm."""
    c = fctx
    dim = 160
    p = _checked(("k14", "doubled"), R.doubled_set(dim), R.EPS_K14, R.FLOOR_K14)
    images = [R.small_rows(130, dim, 5, 1.0 if first == "same_binade" else 2.0 ** -4), np.array(p.Q), np.array(p.T)]
    pairs = [(1, 2), (2, 1), (0, 2), (1, 0)]
    col = _collection(c, images, wide=True)
    try:
        assert col.info()[3] == _ffi.FM_BANK_F32W
        memo = {}
        tally = _Tally()
        for sym in (False, True):
            got = _filtered(c, lambda: col.pairs_mutual_ratio(pairs, TAU, sym))
            want = wide_pairs_ref.pairs_mutual_ratio(images, pairs, TAU, sym, memo)
            assert len(want[0][0]) >= sum(f["t0"] is not None for f in p.fams)
            for k, (g, w) in enumerate(zip(got, want)):
                tally.check((sym, pairs[k]), lambda: _same(g, w, ("pairs_mutual_ratio", sym, pairs[k])))
        tally.done()
    finally:
        col.close()


def _with_decoy(Q, T, diff):
    """Q with one row scaled until the two sets' powers of two differ by `diff`."""
    Qd = np.array(Q)
    mag = 2.0 ** (13 - R.kscale(T) + diff)                     # 1.25 * 2^m has the power of two 13 - m
    Qd[150] = (1.25 * mag * np.where(Qd[150] < 0, -1.0, 1.0)).astype(np.float32)
    assert R.kscale(T) - R.kscale(Qd) == diff
    return Qd


def test_k14_outside_query_forms(fctx):
    """fm_collection_wide_knn2_each and fm_collection_wide_mutual_ratio_each: forward slots (the planted q in the outside bank),
    reverse slots (the planted q in an image, its t rows outside), and an outside bank 2^8 / 2^9 above the stack's scale."""
    c = fctx
    dim = 160
    p = _checked(("k14", "doubled"), R.doubled_set(dim), R.EPS_K14, R.FLOOR_K14)
    Q, T = np.array(p.Q), np.array(p.T)
    small = R.small_rows(130, dim, 6)

    tally = _Tally()

    def each(name, query, images, ran=True):
        qb = c.bank(query)
        col = _collection(c, images, wide=True)

        def mutual(sym):
            got = _filtered(c, lambda: col.wide_mutual_ratio_each(qb, TAU, sym), ran)
            for g, w in zip(got, wide_query_ref.mutual_ratio_each(query, images, TAU, sym)):
                _same(g, w, ("wide_mutual_ratio_each", sym))

        try:
            tally.check(name + " knn2_each",
                        lambda: _same(_filtered(c, lambda: col.wide_knn2_each(qb), ran), wide_query_ref.knn2_each(query, images), "wide_knn2_each"))
            tally.check(name + " mutual_ratio_each", lambda: mutual(False))
            tally.check(name + " mutual_ratio_each symmetric", lambda: mutual(True))
        finally:
            col.close(); qb.close()

    each("forward", Q, [small, T])
    each("forward, rescaled stack", Q, [(small * np.float32(2.0 ** -4)).astype(np.float32), T])     # (the add of T rescales the stack)
    each("reverse", T, [small, Q])
    each("2^8", _with_decoy(Q, T, 8), [small, T])
    each("2^9", _with_decoy(Q, T, 9), [small, T], ran=False)
    tally.done()
