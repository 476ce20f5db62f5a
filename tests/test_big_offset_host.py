"""CPU: the generator and the compact reference of tests/big_offset_ref.py, proved on banks small enough to expand.

The marks are scaled down to 256 rows (the 2^31-byte mark) and 512 rows (2^32), every row is expanded on the host and every
result is computed by brute force over ALL rows -- int64 for the integer and Hamming kinds, the float32 chain for the float
kinds with float64 confirming the order -- and compared with the compact reference: the index map, the tie rule (the lower
row wins) and check_condition.  The layout's row counts are checked against the pitches of csrc/fm_internal.h."""
import os
import re

import numpy as np
import pytest

import big_offset_ref as B
import oracle

SCALED = dict(nq=32, base=256, block=16, tail=256)
CASES = [(k, m) for m in B.MARKS for k in B.KINDS]


# ---- brute force over every row, from one [nq, n] matrix of float32 distances --------------------------------------------------
def _distances(kind, Q, T):
    """(float32 distances as the kernels report them, exact distances for the order)."""
    D = B.exact_distances(kind, Q, T)
    if kind == "bin":
        return D.astype(np.float32), D
    if kind == "u8":
        return np.sqrt(D.astype(np.float32)), D
    idx, dist = oracle.bf_knn(Q, T, len(T), order=1)              # the float32 chain s = fmaf(v, v, s), k ascending
    F = np.empty(D.shape, np.float32)
    np.put_along_axis(F, idx.astype(np.int64), dist, axis=1)
    return F, D


def _lists(F, k):
    order = np.argsort(F, axis=1, kind="stable")[:, :k]          # (distance, index): a stable sort over ascending indices
    return order.astype(np.int64), np.take_along_axis(F, order, axis=1)


def _ratios(d):
    with np.errstate(divide="ignore", invalid="ignore"):
        return d[:, 0].astype(np.float64) / d[:, 1].astype(np.float64)


def _brute(F, sd, tau, tau_acc, radius):
    nq, n = F.shape
    out = {}
    i2, d2 = _lists(F, 2)
    out["knn2"] = (i2, d2)
    out["knn3"] = _lists(F, 3)
    elect = np.argmin(F, axis=0)                                  # every train row's query: the lowest index on a tie
    tx = np.full(nq, -1, np.int64)
    dx = np.full(nq, np.inf, np.float32)
    for t in range(n):                                            # ascending train order, strict <
        q = elect[t]
        if F[q, t] < dx[q]:
            tx[q], dx[q] = t, F[q, t]
    out["xcheck1"] = (tx, dx)
    fwd = _ratios(d2)
    q = np.nonzero(fwd < tau)[0].astype(np.int32)
    out["ratio"] = (q, i2[q, 0], d2[q, 0], fwd[q])
    with np.errstate(divide="ignore", invalid="ignore"):
        ra = dx.astype(np.float64) / sd
        ok = (tx >= 0) & (ra < tau_acc)
    q = np.nonzero(ok)[0].astype(np.int32)
    out["accepted"] = (q, tx[q], dx[q], ra[q])
    ri, rd = _lists(np.ascontiguousarray(F.T), 2)                 # every train row's two nearest query rows
    rev = _ratios(rd)
    t0 = i2[:, 0]
    for name, sym in (("mutual", False), ("mutual_sym", True)):
        keep = (fwd < tau) & (ri[t0, 0] == np.arange(nq))
        ratio = fwd
        if sym:
            keep &= rev[t0] < tau
            ratio = np.maximum(fwd, rev[t0])
        q = np.nonzero(keep)[0].astype(np.int32)
        out[name] = (q, t0[q], d2[q, 0], ratio[q])
    order, srt = _lists(F, n)
    m = srt < np.float32(radius)
    out["radius"] = (np.concatenate([[0], np.cumsum(m.sum(axis=1))]).astype(np.int64), order[m], srt[m])
    return out


def _same(got, want, what):
    assert len(got) == len(want), what
    for g, w in zip(got, want):
        g, w = np.asarray(g), np.asarray(w)
        if g.dtype.kind == "f":
            assert g.dtype == w.dtype, what
            assert np.array_equal(B.bits(g), B.bits(w)), what
        else:
            assert np.array_equal(g.astype(np.int64), w.astype(np.int64)), what


@pytest.mark.parametrize("kind,mark", CASES, ids=["%s-%s" % (m, k) for k, m in CASES])
def test_compact_reference_equals_brute_force_over_every_row(kind, mark):
    case = B.make_case(kind, mark, **SCALED)
    T = case.expand()
    assert T.shape == (case.n, B.WIDTH[kind]) and case.n == case.lay.m + SCALED["tail"]
    Tc, gmap = case.compact()
    radius = B.radius_for(kind)
    B.check_condition(kind, case.Q, Tc, case.block, k=4, radius=radius)
    assert np.array_equal(T[gmap], Tc) and (np.diff(gmap) > 0).all()
    F, D = _distances(kind, case.Q, T)
    if kind in ("f32", "wide"):
        # float64 confirms the float32 order wherever float64 tells two of the five nearest rows apart
        o32 = np.argsort(F, axis=1, kind="stable")[:, :5]
        d64 = np.take_along_axis(D, o32, axis=1)
        assert (np.diff(d64, axis=1) >= 0).all()
    sd = B.self_dist(kind, case.Q)
    want = _brute(F, sd, 0.8, 0.5, radius)
    got = B.expected(kind, case.Q, Tc, gmap, 0.8, 0.5, radius, sd)
    for name in ("knn2", "knn3", "xcheck1", "ratio", "accepted", "radius", "mutual", "mutual_sym"):
        _same(got[name], want[name], "%s %s %s" % (kind, mark, name))
    # the construction does what it says: every critical position is some query's first or second neighbour, the tie is
    # exact and the lower row has it, every query row is accepted by every test
    first2 = set(got["knn2"][0].reshape(-1).tolist())
    assert set(case.lay.crit.tolist()) <= first2, case.describe(sorted(set(case.lay.crit.tolist()) - first2))
    i3, d3 = got["knn3"]
    assert np.array_equal(B.bits(d3[:, 1]), B.bits(d3[:, 2])) and (i3[:, 1] < case.lay.m).all() and (i3[:, 2] >= case.lay.m).all()
    assert (d3[:, 0] < d3[:, 1]).all()
    for name in ("ratio", "accepted", "mutual", "mutual_sym"):
        assert np.array_equal(got[name][0], np.arange(case.nq)), name
    assert np.array_equal(np.diff(got["radius"][0]), np.full(case.nq, 4))
    assert np.array_equal(got["knn2"][0][:, 0], case.first_neighbour())


@pytest.mark.parametrize("kind", B.KINDS)
def test_collection_case_is_a_bank_whose_groups_are_images(kind):
    """The stack of a collection case, expanded: per distinct image the compact reference of the image alone equals brute
    force on its rows, and the merged compact reference equals brute force on the stack."""
    case = B.make_collection_case(kind, "4g", nq=16, base=4096, block=16, image_rows=512)
    T = case.expand()
    fr = case.first_row
    assert fr[1] == 256 and (np.diff(fr[1:]) == 512).all() and fr[-1] == case.n
    s = [i for i in case.images if fr[i] < case.lay.m < fr[i + 1]]
    assert len(s) == 1 and {s[0] + 1, len(fr) - 2} <= set(case.images)
    sd = B.self_dist(kind, case.Q)
    radius = B.radius_for(kind)
    for i in case.images:
        lo, hi = int(fr[i]), int(fr[i + 1])
        Tc, gmap = case.compact(lo, hi)
        B.check_condition(kind, case.Q, Tc, case.block, k=4)
        F, _ = _distances(kind, case.Q, T[lo:hi])
        big = np.float32(1e30)
        want = _brute(F, sd, 0.8, 0.5, big)
        got = B.expected(kind, case.Q, Tc, gmap, 0.8, 0.5, big, sd)
        for name in ("knn2", "xcheck1", "accepted", "mutual", "mutual_sym"):
            _same(got[name], want[name], "%s image %d %s" % (kind, i, name))
    Tc, gmap = case.compact()
    B.check_condition(kind, case.Q, Tc, case.block, k=4, radius=radius)
    F, _ = _distances(kind, case.Q, T)
    want = _brute(F, sd, 0.8, 0.5, radius)
    got = B.expected(kind, case.Q, Tc, gmap, 0.8, 0.5, radius, sd)
    for name in ("knn3", "ratio", "radius"):
        _same(got[name], want[name], "%s stacked %s" % (kind, name))


@pytest.mark.parametrize("kind", B.KINDS)
def test_pairs_reference_equals_the_mutual_ratio_of_the_expanded_images(kind):
    case = B.make_collection_case(kind, "2g", nq=16, base=4096, block=16, image_rows=512)
    T, fr = case.expand(), case.first_row
    a, b = case.images[-1], case.images[0]
    A, Bm = T[fr[a]:fr[a + 1]], T[fr[b]:fr[b + 1]]
    Fab, _ = _distances(kind, A, Bm)
    for sym in (False, True):
        # brute force over every row of both images: fm_mutual_ratio's rules on the full 2-NN lists
        i2, d2 = _lists(Fab, 2)
        ri, rd = _lists(np.ascontiguousarray(Fab.T), 2)
        with np.errstate(invalid="ignore"):
            fwd, rev = _ratios(d2), _ratios(rd)
            keep = (fwd < 0.99) & (ri[i2[:, 0], 0] == np.arange(len(A)))
            ratio = fwd
            if sym:
                keep &= rev[i2[:, 0]] < 0.99
                ratio = np.maximum(fwd, rev[i2[:, 0]])
        q = np.nonzero(keep)[0]
        (Ta, ma), (Tb, mb) = case.compact(int(fr[a]), int(fr[a + 1])), case.compact(int(fr[b]), int(fr[b + 1]))
        w = B.pairs_mutual_ratio(kind, Ta, Tb, case.block, 0.99, sym)
        assert len(q) > 0
        _same((ma[w[0]], mb[w[1]], w[2], w[3]), (q, i2[q, 0], d2[q, 0], ratio[q]), "%s pairs symmetric=%s" % (kind, sym))


@pytest.mark.parametrize("kind", B.KINDS)
def test_check_condition_rejects_a_filler_row_inside_the_planted_distances(kind):
    case = B.make_case(kind, "2g", **SCALED)
    Tc, _ = case.compact()
    B.check_condition(kind, case.Q, Tc, case.block, k=4)
    bad = Tc.copy()
    q = 5
    mine = np.nonzero((case.owner == q) & (case.rank == 1))[0][0]
    bad[3] = case.rows[mine]                     # a filler row as close to query row 5 as its second neighbour
    with pytest.raises(AssertionError, match="query rows \\[5\\]"):
        B.check_condition(kind, case.Q, bad, case.block, k=4)
    # ... and a radius that reaches the filler
    far = np.float32(1e6)
    with pytest.raises(AssertionError, match="radius"):
        B.check_condition(kind, case.Q, Tc, case.block, k=4, radius=far)


def _header_pitches():
    """Bytes per row of every plane named in PITCH, from the Bank struct's comments in csrc/fm_internal.h."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fast-match_amd", "csrc", "fm_internal.h")).read()
    size = {"int8_t": 1, "uint8_t": 1, "uint16_t": 2, "float": 4}
    out = {}
    for plane in ("rows8", "rows6", "rowsf", "rowsh", "wrows", "wrowsh", "rowsb", "rows4"):
        m = re.search(r"^\s*(\w+)\*\s+%s\s*=\s*nullptr;(.*)$" % plane, src, re.M)
        assert m, plane
        elem = size[m.group(1)]
        d = re.search(r"\[n_pad\]\[(\d+)( ksteps)?\]", m.group(2))
        if d is None:                            # rows8: described in the layout comment at the top of the file
            d = re.search(r"//\s*%s\s*:\s*\w+\s*\[n_pad\]\[(\d+)( ksteps)?\]" % plane, src)
        assert d, plane
        out[plane] = elem * int(d.group(1)) * (4 if d.group(2) else 1)      # (64-byte binary rows: 4 K steps)
    return out


@pytest.mark.parametrize("kind", B.KINDS)
def test_layout_row_counts_follow_the_pitches(kind):
    pitches = _header_pitches()
    for plane, pitch in B.PITCH[kind]:
        assert pitches[plane] == pitch, plane
    first = B.PITCH[kind][0][1]
    assert first == max(p for _, p in B.PITCH[kind]) or kind == "bin"     # (bin: the packed rows are the issue's plane)
    for mark, nbytes in (("2g", 1 << 31), ("4g", 1 << 32)):
        lay = B.layout(kind, mark)
        assert lay.m * first == nbytes and lay.n == lay.m + 4096
        want = {lay.n - 1}
        for plane, pitch in B.PITCH[kind]:
            for b in (1 << 31, 1 << 32):
                if b // pitch <= lay.m:
                    assert (b // pitch) in lay.marks
                    want |= {b // pitch + d for d in (-33, -1, 0, 1, 31, 32, 33)}
        assert set(lay.crit.tolist()) == want
        assert (lay.crit >= 4096).all() and lay.crit[-1] == lay.n - 1
    assert {k: B.layout(k, "2g").m for k in B.KINDS} == {"wide": 1 << 21, "f32": 1 << 22, "u8": 1 << 24, "bin": 1 << 25}


def test_full_size_cases_meet_the_condition():
    """The cases the GPU tests run, at full size: planted rows only -- nothing of the bank's size exists here."""
    for mark in B.MARKS:
        for kind in B.KINDS:
            case = B.make_case(kind, mark)
            Tc, gmap = case.compact()
            assert len(Tc) == case.block + 5 * case.nq and gmap[-1] == case.n - 1
            B.check_condition(kind, case.Q, Tc, case.block, k=4, radius=B.radius_for(kind))
