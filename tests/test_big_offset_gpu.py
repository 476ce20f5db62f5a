"""GPU: every matcher entry point on banks and train collections whose byte offsets pass 2^31 and 2^32.

A kernel addresses a plane as base + row * pitch; these tests make that product pass 2^31 and 2^32 bytes in every plane of
every bank kind (tests/big_offset_ref.py has the row counts) and compare the results bit for bit with the suite's exact
references.  Nothing of the bank's size exists on the host: the train rows are made on the device (one filler block repeated,
a few hundred planted rows written by index), the references see the compact set of a few thousand rows, and the calls with
the big bank on the query side leave their results on the device, where the planted rows' outputs are gathered.

A wrong neighbour at a planted position means an offset wrapped: the failure message names the position and the mark it sits
on, DESIGN.md ("Index widths") has the expression.  The 2^31 cases run before the 2^32 ones."""
import functools
import time

import numpy as np
import pytest

import big_offset_ref as B
from fastmatch_amd import _ffi

pytestmark = pytest.mark.gpu

TAU, TAU_ACC = 0.8, 0.5
# The wide fp16 filter keeps its candidates in ONE list (at least 2^20 records) and every split of the reduced bank starts
# with an empty bound: it records its first 16-row tile whole and then every row inside the margin of its OWN running
# bound.  With 96 output rows against millions of reduced rows the built-in rule takes 512 splits (128 per image of a
# collection), every one of which meets a copy of the same filler block: about 26 records per (output row, split) were
# measured, 1.3 million in all, the list overflows and the exact kernel redoes the call -- whatever the filler's distance,
# the margin being relative.  The results are the same either way (the tests passed bit for bit with the fallback); for the
# filter itself to be what is tested past the marks, the wide cases fix the splits with the option "f32_nsplit", which never
# changes a result: 96 * 32 * 26 = 80 000 records for a bank pair, 96 * 4 * 26 * 35 images = 350 000 for a collection.
WIDE_PAIR_NSPLIT, WIDE_COLL_NSPLIT = 32, 4
CASES = [(m, k) for m in B.MARKS for k in B.KINDS]          # the smaller mark first, inside a mark the smaller bank first
IDS = ["%s-%s" % c for c in CASES]
# device bytes per train row while a bank is built and used: source tensor + every plane (fm_internal.h) + sweep partials
BANK_BYTES = {"u8": 128 + 128 + 128 + 4 + 8 + 16 + 32,      # source, rows8, rows6, norm, aux, stat6, keys [2] + lists
              "f32": 512 + 512 + 256 + 8 + 32,
              "wide": 1024 + 1024 + 512 + 8 + 32,
              "bin": 64 + 64 + 256 + 32}


def _torch():
    import torch
    return torch


def _need_memory(ctx, nbytes, what):
    free, total = ctx.mem_info()
    if free < nbytes:
        pytest.fail("%s needs %d bytes of device memory, %d are free (of %d)" % (what, nbytes, free, total))


def _report(ctx, what, t0, free0):
    free, _ = ctx.mem_info()
    print("\n[big-offset] %s: %.2f s, %.2f GiB of device memory in use beyond the start" % (what, time.time() - t0, (free0 - free) / 2.0 ** 30))


def _same(case, name, got, want, base=0):
    """Bit-for-bit equality of a result tuple; a mismatch names the planted positions of the first rows that differ."""
    assert len(got) == len(want), name
    for j, (g, w) in enumerate(zip(got, want)):
        g, w = np.asarray(g), np.asarray(w)
        if g.dtype.kind == "f":
            assert g.dtype == w.dtype, name
            ok = g.shape == w.shape and np.array_equal(B.bits(g), B.bits(w))
        else:
            ok = g.shape == w.shape and np.array_equal(g.astype(np.int64), w.astype(np.int64))
        if not ok:
            where = ""
            if g.shape == w.shape and g.size:
                bad = np.nonzero((B.bits(g) != B.bits(w)) if g.dtype.kind == "f" else (g.astype(np.int64) != w.astype(np.int64)))
                rows = np.unique(bad[0])[:4]
                where = " at rows %s of the result" % rows.tolist()
                if w.dtype.kind != "f" and j <= 1:
                    where += "; expected there: " + case.describe(np.asarray(w)[rows].reshape(-1) + base) + \
                             "; got: " + case.describe(np.maximum(np.asarray(g)[rows].reshape(-1), 0) + base)
            pytest.fail("%s %s %s: field %d differs%s (shapes %s / %s)" % (case.kind, case.lay.mark, name, j, where, g.shape, w.shape))


class _Options(object):
    """Context options for a block of calls, put back afterwards (the context is the session's)."""

    def __init__(self, ctx, **opts):
        self.ctx, self.opts, self.old = ctx, opts, {}

    def __enter__(self):
        for k, v in self.opts.items():
            self.old[k] = self.ctx.get_option(k)
            self.ctx.set_option(k, v)
        return self

    def __exit__(self, *exc):
        for k, v in self.old.items():
            self.ctx.set_option(k, v)
        return False


def _query_bank(ctx, case, sd):
    kind = case.kind
    if kind == "bin":
        qb = ctx.bank_binary(case.Q)
        qb.set_hamming_selfdist(sd)
    elif kind == "wide":
        qb = ctx.bank(case.Q)
        qb.set_wide_selfdist(sd)
    else:
        qb = ctx.bank(case.Q, float_route=kind == "f32")
        if kind == "u8":
            qb.set_selfdist(sd)
    return qb


# ---- bank pairs ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=CASES, ids=IDS)
def pair(request, ctx):
    """(case, query bank, train bank made from a device tensor, expected results, source tensor)."""
    from fastmatch_amd import torchmatch
    torch = _torch()
    mark, kind = request.param
    case = B.make_case(kind, mark)
    Tc, gmap = case.compact()
    radius = B.radius_for(kind)
    B.check_condition(kind, case.Q, Tc, case.block, k=4, radius=radius)
    sd = B.self_dist(kind, case.Q)
    want = B.expected(kind, case.Q, Tc, gmap, TAU, TAU_ACC, radius, sd)
    _need_memory(ctx, case.n * BANK_BYTES[kind] + (1 << 30), "the %s bank of %d rows" % (kind, case.n))
    free0 = ctx.mem_info()[0]
    t0 = time.time()
    src = case.on_device(torch)
    tb = torchmatch.bank(src, binary=kind == "bin", float_route=kind == "f32", context=ctx)
    qb = _query_bank(ctx, case, sd)
    assert (tb.n, tb.kind) == (case.n, {"u8": _ffi.FM_BANK_I8, "f32": _ffi.FM_BANK_F32, "wide": _ffi.FM_BANK_F32W, "bin": _ffi.FM_BANK_BIN}[kind])
    _report(ctx, "%s %s: bank of %d rows built" % (mark, kind, case.n), t0, free0)
    yield {"case": case, "q": qb, "t": tb, "want": want, "sd": sd, "radius": radius, "src": src, "free0": free0}
    qb.close()
    tb.close()
    del src
    ctx.sync()
    torch.cuda.empty_cache()


def _pair_calls(ctx, p, deep):
    """The calls of one bank kind with the small bank as the query, against `want`.  deep: every entry point; else the ones
    that differ under the filter options."""
    case, q, t, want, radius = p["case"], p["q"], p["t"], p["want"], p["radius"]
    kind = case.kind

    def check(name, call, key):
        s0 = ctx.f32_filter_stats()
        got = call()
        s1 = ctx.f32_filter_stats()
        if s1 != s0:
            print("[big-offset] %s %s %s: %d fp16-filter launches, %d fallbacks" % (case.lay.mark, kind, name, s1[0] - s0[0], s1[1] - s0[1]))
        _same(case, name, got, want[key])

    check("knn2", lambda: ctx.knn2(q, t), "knn2")
    check("xcheck1", lambda: ctx.xcheck1(q, t), "xcheck1")
    check("mutual_ratio", lambda: ctx.mutual_ratio(q, t, TAU), "mutual")
    check("mutual_ratio symmetric", lambda: ctx.mutual_ratio(q, t, TAU, symmetric=True), "mutual_sym")
    rad = {"bin": ctx.hamming_radius_match, "wide": ctx.wide_radius_match}.get(kind, ctx.radius_match)
    check("radius_match", lambda: rad(q, t, radius), "radius")
    check("radius_match per row", lambda: rad(q, t, np.full(case.nq, radius, np.float32)), "radius")
    if kind == "wide":
        check("wide_match_accepted", lambda: ctx.wide_match_accepted(q, t, TAU_ACC), "accepted")
    if not deep:
        return
    check("knn2_ratio", lambda: ctx.knn2_ratio(q, t, TAU), "ratio")
    if kind != "wide":                                       # (k >= 3 is not built for wide banks)
        check("knn k=3", lambda: ctx.knn(q, t, 3), "knn3")
    if kind == "bin":
        check("hamming_match_accepted", lambda: ctx.hamming_match_accepted(q, t, TAU_ACC), "accepted")


def test_small_query_against_the_big_bank(ctx, pair):
    case, kind = pair["case"], pair["case"].kind
    t0 = time.time()
    if kind in ("f32", "wide"):
        for setting in (0, 2):
            # (wide: WIDE_PAIR_NSPLIT, see there)
            with _Options(ctx, f32_filter=setting, **({"f32_nsplit": WIDE_PAIR_NSPLIT} if kind == "wide" else {})):
                l0, f0 = ctx.f32_filter_stats()
                _pair_calls(ctx, pair, deep=setting == 0)
                l1, f1 = ctx.f32_filter_stats()
            if setting == 2:
                assert l1 > l0, "f32_filter = 2: no launch went through the fp16 filter"
                assert f1 == f0, "f32_filter = 2: %d calls fell back to the exact kernel" % (f1 - f0)
    else:
        _pair_calls(ctx, pair, deep=True)
        if kind == "u8":
            _accepted_u8(ctx, pair)
    _report(ctx, "%s %s: small query against the big bank" % (case.lay.mark, kind), t0, pair["free0"])


def _accepted_u8(ctx, p):
    """Integer route: fm_match_ratio / fm_match_accepted put the big bank on the output-row side of K1; with "fp6_filter" at
    its default the sweep is the FP6 matrix-core filter, and its counters show that it ran."""
    case, q, t, want = p["case"], p["q"], p["t"], p["want"]
    assert ctx.get_option("fp6_filter") == 1
    for setting in (1, 0):
        with _Options(ctx, fp6_filter=setting):
            _same(case, "match_accepted fp6_filter=%d" % setting, ctx.match_accepted(q, t, TAU_ACC), want["accepted"])
            if setting == 1:
                rec, fb = ctx.get_option("fp6_records"), ctx.get_option("fp6_fallbacks")
                assert rec >= case.nq and fb == 0, "the FP6 filter did not serve the call: %d records, %d fallbacks" % (rec, fb)
            tidx, dist, ratio, passed, npass = ctx.match_ratio(q, t, TAU_ACC)
            _same(case, "match_ratio fp6_filter=%d" % setting, (tidx, dist), want["xcheck1"])
            acc = want["accepted"]
            assert npass == len(acc[0]) and np.array_equal(np.nonzero(passed)[0], acc[0])
            assert np.array_equal(B.bits(ratio[acc[0]]), B.bits(acc[3]))


def test_big_bank_on_the_query_side_with_device_results(ctx, pair):
    """fm_knn_dev with the big bank as the query: 2-NN lists of millions of rows stay on the device; the planted rows' lists and
    those of the last filler block are gathered there and compared."""
    torch = _torch()
    case, q, t, kind = pair["case"], pair["q"], pair["t"], pair["case"].kind
    _need_memory(ctx, case.n * 48 + (1 << 28), "the device lists of %d rows" % case.n)
    t0 = time.time()
    idx = torch.full((case.n, 2), -7, dtype=torch.int32, device="cuda")
    dist = torch.full((case.n, 2), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    tail = np.arange(case.n - case.block, case.n, dtype=np.int64)
    rows = np.unique(np.concatenate([case.pos, tail]))
    sel = torch.from_numpy(rows).cuda()
    planted = np.isin(rows, case.pos)
    content = np.array(case.filler)[rows % case.block]
    content[planted] = case.rows[np.searchsorted(case.pos, rows[planted])]
    wi, wd = B.knn(kind, content, case.Q, 2)
    settings = (0, 2) if kind in ("f32", "wide") else (None,)
    for setting in settings:
        idx.fill_(-7)
        with _Options(ctx, **({} if setting is None else {"f32_filter": setting})):
            ctx.knn_dev(t, q, 2, idx.data_ptr(), dist.data_ptr(), consumer_stream=stream)
        gi, gd = idx[sel].cpu().numpy(), dist[sel].cpu().numpy()
        bad = np.nonzero((gi != wi).any(axis=1) | (B.bits(gd) != B.bits(wd)).any(axis=1))[0]
        assert len(bad) == 0, "%s %s knn_dev (f32_filter %s): the lists of %s differ" % (kind, case.lay.mark, setting, case.describe(rows[bad[:4]]))
        assert int((idx < 0).sum().item()) == 0 and int((idx >= case.nq).sum().item()) == 0
    del idx, dist
    _report(ctx, "%s %s: big bank as the query, device results" % (case.lay.mark, kind), t0, pair["free0"])


# ---- train collections ---------------------------------------------------------------------------------------------------------
PLANE_BYTES = {"u8": 128 + 128 + 4 + 8 + 16, "f32": 512 + 256 + 8, "wide": 1024 + 512 + 8, "bin": 64 + 256}
TAU_PAIRS = 0.99


def _locate(first, g):
    g = np.asarray(g, np.int64)
    img = np.searchsorted(first, np.maximum(g, 0), side="right") - 1
    return np.where(g >= 0, img, -1), np.where(g >= 0, g - first[np.maximum(img, 0)], -1)


@pytest.fixture(scope="module", params=CASES, ids=IDS)
def coll(request, ctx):
    """A collection grown image by image (2^17 rows each, device tensors) past the mark: the repeated adds take the stack
    through its doubling growth and the device copies that go with it.  Every image is the filler; the distinct ones -- the
    image that straddles the mark (and the marks of the other planes), the one behind it and the last one -- carry planted
    rows."""
    from fastmatch_amd import torchmatch
    torch = _torch()
    mark, kind = request.param
    case = B.make_collection_case(kind, mark)
    first = case.first_row
    ni = len(first) - 1
    # (growth: the old arrays and new ones of up to twice the size are alive together)
    _need_memory(ctx, 3 * case.n * PLANE_BYTES[kind] + case.n * 64 + (2 << 30), "the %s collection of %d rows" % (kind, case.n))
    free0 = ctx.mem_info()[0]
    t0 = time.time()
    sd = B.self_dist(kind, case.Q)
    qb = _query_bank(ctx, case, sd)
    tc = torchmatch.Collection(context=ctx)
    filler = case.on_device(torch, 0, B.IMAGE_ROWS)            # (rows [0, 2^17) hold no planted row)
    assert case.pos.min() >= first[1]
    for i in range(ni):
        lo, hi = int(first[i]), int(first[i + 1])
        img = case.on_device(torch, lo, hi) if i in case.images else filler[:hi - lo]
        got = tc.add_wide(img) if kind == "wide" else tc.add(img, binary=kind == "bin")
        assert got == i
        del img
    c = tc._collection()
    assert c.info()[:2] == (ni, case.n) and np.array_equal(c.image_rows(), np.diff(first))
    _report(ctx, "%s %s: collection of %d images, %d rows built" % (mark, kind, ni, case.n), t0, free0)
    yield {"case": case, "q": qb, "c": c, "tc": tc, "sd": sd, "first": first, "free0": free0}
    qb.close()
    tc.close()
    del filler
    ctx.sync()
    torch.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def _image_refs(kind, mark):
    """Per distinct image the bank-pair reference of that image alone, and the one of a filler image (two filler blocks: the
    second neighbour of a row of the first is its copy in the second)."""
    case = B.make_collection_case(kind, mark)
    first = case.first_row
    sd = B.self_dist(kind, case.Q)
    big = np.float32(0.0)
    refs = {}
    for i in case.images:
        Tc, gmap = case.compact(int(first[i]), int(first[i + 1]))
        B.check_condition(kind, case.Q, Tc, case.block, k=4)
        refs[i] = B.expected(kind, case.Q, Tc, gmap, TAU, TAU_ACC, big, sd, stacked=False)
    two = np.concatenate([case.filler, case.filler])
    refs[-1] = B.expected(kind, case.Q, two, np.arange(len(two), dtype=np.int64), TAU, TAU_ACC, big, sd, stacked=False)
    return refs


def test_collection_image_by_image(ctx, coll):
    case, q, c, first = coll["case"], coll["q"], coll["c"], coll["first"]
    kind, ni = case.kind, len(coll["first"]) - 1
    refs = _image_refs(kind, case.lay.mark)
    t0 = time.time()
    settings = (0, 2) if kind in ("f32", "wide") else (None,)
    for setting in settings:
        opts = {} if setting is None else {"f32_filter": setting}
        if kind == "wide":
            opts["f32_nsplit"] = WIDE_COLL_NSPLIT
        with _Options(ctx, **opts):
            s0 = ctx.f32_filter_stats()
            out = {}
            idx, dist = c.wide_knn2_each(q) if kind == "wide" else c.knn2_each(q)
            out["knn2"] = [(idx[i], dist[i]) for i in range(ni)]
            if kind == "wide":
                out["accepted"] = c.wide_match_accepted_each(q, TAU_ACC)
                out["mutual"] = c.wide_mutual_ratio_each(q, TAU)
                out["mutual_sym"] = c.wide_mutual_ratio_each(q, TAU, symmetric=True)
            else:
                tx, dx = c.xcheck1_each(q)
                out["xcheck1"] = [(tx[i], dx[i]) for i in range(ni)]
                out["mutual"] = c.mutual_ratio_each(q, TAU)
                out["mutual_sym"] = c.mutual_ratio_each(q, TAU, symmetric=True)
                if kind == "u8":
                    out["accepted"] = c.match_accepted_each(q, TAU_ACC)
                elif kind == "bin":
                    out["accepted"] = c.hamming_match_accepted_each(q, TAU_ACC)
            s1 = ctx.f32_filter_stats()
        for name, per_image in out.items():
            for i in range(ni):
                _same(case, "%s of image %d (f32_filter %s)" % (name, i, setting), per_image[i], refs[i if i in refs else -1][name], base=int(first[i]))
        if setting == 2:
            assert s1[0] > s0[0], "f32_filter = 2: no launch went through the fp16 filter"
            assert s1[1] == s0[1], "f32_filter = 2: %d sweeps fell back to the exact kernel" % (s1[1] - s0[1])
    _report(ctx, "%s %s: collection, image by image" % (case.lay.mark, kind), t0, coll["free0"])


def test_collection_stacked_and_masked(ctx, coll):
    import masked_ref
    torch = _torch()
    case, q, c, first = coll["case"], coll["q"], coll["c"], coll["first"]
    kind = case.kind
    t0 = time.time()
    Tc, gmap = case.compact()
    radius = B.radius_for(kind)
    B.check_condition(kind, case.Q, Tc, case.block, k=4, radius=radius)
    want = B.expected(kind, case.Q, Tc, gmap, TAU, TAU_ACC, radius, coll["sd"])
    off, gi, gd = want["radius"]
    wimg, wloc = _locate(first, gi)
    rad = {"bin": c.hamming_radius_match, "wide": c.wide_radius_match}.get(kind, c.radius_match)
    settings = (0, 2) if kind == "f32" else (None,)
    for setting in settings:
        with _Options(ctx, **({} if setting is None else {"f32_filter": setting})):
            o, img, idx, dist = rad(q, radius)
            _same(case, "collection radius_match", (o, idx + first[img], img, dist), (off, gi, wimg, gd))
            if kind == "wide":
                continue                                     # (the stacked k-NN forms are not built for wide collections)
            img, idx, dist = c.knn(q, 3)
            _same(case, "collection knn k=3", (idx + first[img], img, dist), (want["knn3"][0], _locate(first, want["knn3"][0])[0], want["knn3"][1]))
            qi, img, ti, dist, ratio = c.knn2_ratio(q, TAU)
            w = want["ratio"]
            _same(case, "collection knn2_ratio", (qi, ti + first[img], dist, ratio), w)
    if kind != "wide":
        # one mask: nothing permitted but the distinct images, minus every query row's first planted neighbour there
        sel = np.isin(np.searchsorted(first, case.pos, side="right") - 1, case.images)
        assert sel.all()
        keep = np.ones((case.nq, len(Tc)), bool)
        keep[:, :case.block] = False
        firsts = (case.rank == 0)
        keep[case.owner[firsts], case.block + np.nonzero(firsts)[0]] = False
        with c.mask(case.nq) as mk:
            for i in case.images:
                lo, hi = int(first[i]), int(first[i + 1])
                m = torch.ones((case.nq, hi - lo), dtype=torch.uint8, device="cuda")
                inside = firsts & (case.pos >= lo) & (case.pos < hi)
                m[torch.from_numpy(case.owner[inside].astype(np.int64)).cuda(), torch.from_numpy(case.pos[inside] - lo).cuda()] = 0
                torch.cuda.synchronize()
                mk.set_dev(m.data_ptr(), img=i, pitch=m.stride(0))
                del m
            # reference: the planted rows alone (the permitted filler is farther than four permitted planted rows)
            Tp = Tc[case.block:]
            for k in (2, 3):
                wi, wd = masked_ref.knn({"u8": "u8", "f32": "f32", "bin": "bin"}[kind], case.Q, Tp, keep[:, case.block:], k)
                wg = np.where(wi >= 0, gmap[case.block:][np.maximum(wi, 0)], -1)
                img, idx, dist = c.knn_masked(q, mk, k)
                _same(case, "collection knn_masked k=%d" % k, (idx + first[img], img, dist), (wg, _locate(first, wg)[0], wd))
    _report(ctx, "%s %s: collection, stacked and masked calls" % (case.lay.mark, kind), t0, coll["free0"])


def test_collection_pairs(ctx, coll):
    """fm_collection_pairs_mutual_ratio on a pair of images that both lie past the mark, in both orders, and on pairs that
    start in the image that straddles it.  Reference: big_offset_ref.pairs_mutual_ratio -- a filler row's nearest row in the other
    image is its copy at distance 0, more than once, so no filler row is ever accepted and only the planted rows decide."""
    case, c, first = coll["case"], coll["c"], coll["first"]
    kind = case.kind
    t0 = time.time()
    s = [i for i in case.images if first[i] < case.lay.m < first[i + 1]][0]
    last = len(first) - 2
    pairs = [(s + 1, last), (last, s), (s, s + 1)]
    sets = {i: case.compact(int(first[i]), int(first[i + 1])) for i in {p for ab in pairs for p in ab}}
    for sym in (False, True):
        got = c.pairs_mutual_ratio(pairs, TAU_PAIRS, symmetric=sym)
        for (a, b), g in zip(pairs, got):
            (Ta, ma), (Tb, mb) = sets[a], sets[b]
            w = B.pairs_mutual_ratio(kind, Ta, Tb, case.block, TAU_PAIRS, sym)
            assert len(w[0]) > 0
            _same(case, "pairs_mutual_ratio (%d, %d) symmetric=%s" % (a, b, sym), (g[0] + first[a], g[1] + first[b], g[2], g[3]),
                  (ma[w[0]] + first[a], mb[w[1]] + first[b], w[2], w[3]))
    _report(ctx, "%s %s: collection, image pairs" % (case.lay.mark, kind), t0, coll["free0"])
