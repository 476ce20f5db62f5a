"""Inputs and references for banks whose byte offsets pass 2^31 and 2^32 (tests/test_big_offset_host.py, _gpu.py).  No GPU
code: the module imports on a machine without one.

A bank of millions of rows is described by a few thousand of them.  Row r of the bank is filler[r % block] -- one block of
random rows repeated -- except at the PLANTED positions, which sit around every row count at which a plane's byte offset
row * pitch reaches 2^31 or 2^32, at the last row, and spread over the rest.  Every query row owns, in every group of rows
(a bank is one group; a collection has one per distinct image), five planted rows at known, growing distances
(levels 1, 2, 2, 3, 4: ranks 1 and 2 are an exact tie, the lower row on the lower side of the mark), all far closer than any
filler row.  So the k nearest rows of every query, k <= 4, are planted rows, and the exact references of this suite applied
to the COMPACT set -- the first filler block followed by the planted rows in ascending position -- give, with the indices
mapped back, the results on the whole bank: the map keeps the order, so a later copy of a filler row never beats the first
one.  check_condition() asserts the premise for every query row."""
import functools
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (_HERE, os.path.dirname(_HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import grown_ref            # noqa: E402
import hamming_fast_ref     # noqa: E402
import hamming_radius_ref   # noqa: E402
import hamming_ref          # noqa: E402
import mutual_ratio_ref     # noqa: E402
import oracle               # noqa: E402
import radius_coll_ref      # noqa: E402
import wide_fast_ref        # noqa: E402
import wide_radius_ref      # noqa: E402
import wide_ref             # noqa: E402

KINDS = ("wide", "f32", "u8", "bin")            # ascending bank bytes at a mark's row count
MARKS = ("2g", "4g")
# bytes per row of the planes a kernel indexes with row * pitch, the plane that passes a mark first in front (fm_internal.h)
PITCH = {"u8": (("rows8", 128), ("rows6", 128)),
         "f32": (("rowsf", 512), ("rowsh", 256)),
         "wide": (("wrows", 1024), ("wrowsh", 512)),
         "bin": (("rowsb", 64), ("rows4", 256))}
WIDTH = {"u8": 128, "f32": 128, "wide": 256, "bin": 64}     # elements per row (bin: bytes)
NEAR = (-33, -1, 0, 1, 31, 32, 33)                          # planted positions around a mark
LEVEL = (1, 2, 2, 3, 4)                                     # distance level of a query's five rows in a group (ranks 1, 2: the tie)
NQ = 96
BLOCK = 4096
TAIL = 4096
RADIUS_LEVEL = 3.5                                          # a radius that takes levels 1 .. 3 of group 0 and nothing else


def rows_at(kind, nbytes, plane=0):
    """The row whose offset in a plane of `kind` is `nbytes`."""
    pitch = PITCH[kind][plane][1]
    assert nbytes % pitch == 0
    return nbytes // pitch


class Layout(object):
    """n rows; `marks` {row: [what passes there]}; `crit` the planted positions that every case has, ascending; `m` the row of
    the case's own mark (2^31 or 2^32 bytes into the kind's first plane)."""

    def __init__(self, kind, mark, base=None, tail=TAIL, n=None):
        prim = PITCH[kind][0][1]
        unit = rows_at(kind, 1 << 31) if base is None else int(base)      # rows of the first plane in 2^31 bytes
        self.kind, self.mark = kind, mark
        self.m = unit * (1 if mark == "2g" else 2)
        self.n = self.m + tail if n is None else int(n)
        assert self.n >= self.m + 34
        self.marks = {}
        for plane, pitch in PITCH[kind]:
            for name, mult in (("2^31", 1), ("2^32", 2)):
                assert (unit * prim * mult) % pitch == 0
                r = unit * prim * mult // pitch
                if r <= self.m:
                    self.marks.setdefault(r, []).append("%s bytes of %s" % (name, plane))
        pos = {self.n - 1}
        for r in self.marks:
            pos.update(r + d for d in NEAR)
        self.crit = np.array(sorted(pos), np.int64)

    def label(self, row):
        """What a row of the bank is to the marks: for failure messages."""
        row = int(row)
        for r in sorted(self.marks):
            if abs(row - r) <= 33:
                return "row %d = mark %+d (%s)" % (row, row - r, ", ".join(self.marks[r]))
        below = [r for r in self.marks if r <= row]
        where = "past " + ", ".join(self.marks[max(below)]) if below else "below every mark"
        return "row %d (%s%s)" % (row, "the last row, " if row == self.n - 1 else "", where)

    def far_from_marks(self, rows):
        ok = rows != self.n - 1
        for r in self.marks:
            ok &= np.abs(rows - r) > 34
        return ok


def layout(kind, mark, base=None, tail=TAIL):
    return Layout(kind, mark, base, tail)


def _spread(lay, lo, hi, need):
    """`need` distinct rows of [lo, hi) away from the marks, evenly spread."""
    if need == 0:
        return np.zeros(0, np.int64)
    cand = np.unique(np.linspace(lo, hi - 1, 8 * need + 16).astype(np.int64))
    cand = cand[lay.far_from_marks(cand)]
    assert len(cand) >= need, "no room for %d planted rows in [%d, %d)" % (need, lo, hi)
    return cand[np.unique(np.linspace(0, len(cand) - 1, need).astype(np.int64))] if need > 1 else cand[:1]


def _plan(lay, nq, groups, seed):
    """(position, query, rank, group) of every planted row.  A critical position goes to a query of its own as its first
    neighbour (rank 0) or, every other one below the mark, as the lower row of its tie (rank 1: the second neighbour)."""
    rng = np.random.default_rng(seed)
    out = []
    claimed = set()
    for g, (lo, hi) in enumerate(groups):
        crit = [int(c) for c in lay.crit if lo <= c < hi]
        claimed.update(crit)
        assert len(crit) <= nq, "more critical positions than query rows"
        split = lay.m if lo < lay.m < hi else (lo + hi) // 2
        have = {}
        for k, c in enumerate(crit):
            q = (5 * k + 3 * g) % nq
            have[(q, 1 if (k % 2 == 1 and c < split) else 0)] = c
        assert len(have) == len(crit)
        want_lo = [(q, r) for q in range(nq) for r in (1, 3) if (q, r) not in have] + \
                  [(q, 0) for q in range(0, nq, 2) if (q, 0) not in have]
        want_hi = [(q, r) for q in range(nq) for r in (2, 4)] + [(q, 0) for q in range(1, nq, 2) if (q, 0) not in have]
        for want, a, b in ((want_lo, lo, split), (want_hi, split, hi)):
            rows = _spread(lay, a, b, len(want))
            assert len(rows) == len(want)
            for j, p in zip(rng.permutation(len(want)), rows):
                have[want[j]] = int(p)
        for (q, r), p in have.items():
            out.append((p, q, r, g))
        for q in range(nq):
            assert have[(q, 1)] < split <= have[(q, 2)]          # the tie: opposite sides, the lower row is rank 1
    assert claimed == set(int(c) for c in lay.crit), "a critical position lies in no group"
    out.sort()
    a = np.array(out, np.int64)
    assert len(np.unique(a[:, 0])) == len(a)
    return a[:, 0], a[:, 1].astype(np.int32), a[:, 2].astype(np.int32), a[:, 3].astype(np.int32)


def _random_rows(kind, rng, n):
    w = WIDTH[kind]
    if kind == "u8":
        return rng.integers(8, 200, (n, w)).astype(np.uint8)
    if kind == "bin":
        return rng.integers(0, 256, (n, w), dtype=np.uint8)
    return (rng.standard_normal((n, w)) * 40.0).astype(np.float32)         # (non-integer values: the float32 route)


def _planted_row(kind, q, i, g, r):
    """Query row q's planted row of rank r in group g: the query plus its level in one dimension (binary: level flipped bits).
    Ranks 1 and 2 are at one distance exactly -- integer kinds: the same step in another dimension, float kinds: the same row."""
    w = WIDTH[kind]
    level = 5 * g + LEVEL[r]
    row = q.copy()
    if kind == "bin":
        start = (37 * i + 101 * r + 211 * g) % (8 * w)
        for j in range(level):
            b = (start + 3 * j) % (8 * w)
            row[b >> 3] ^= np.uint8(1 << (b & 7))
        return row
    if kind == "u8":
        row[(7 * i + 13 * g + 29 * r) % w] += np.uint8(level)
        return row
    rr = 1 if r == 2 else r
    d = (7 * i + 13 * g + 29 * rr) % w
    row[d] = np.float32(row[d] + np.float32(0.25 * level))
    return row


class Case(object):
    """One bank (or one collection's stack) of `n` rows: Q [nq], filler [block], planted `rows` at `pos` (ascending), and per
    planted row its query, rank and group."""

    def __init__(self, kind, lay, nq, block, groups, seed):
        rng = np.random.default_rng(seed)
        self.kind, self.lay, self.nq, self.block, self.n = kind, lay, nq, block, lay.n
        self.groups = tuple(groups)
        assert all(lo >= block for lo, _ in self.groups), "the first filler block is never overwritten"
        self.Q = _random_rows(kind, rng, nq)
        self.filler = _random_rows(kind, rng, block)
        self.pos, self.owner, self.rank, self.group = _plan(lay, nq, self.groups, seed + 1)
        self.rows = np.stack([_planted_row(kind, self.Q[i], int(i), int(g), int(r))
                              for i, r, g in zip(self.owner, self.rank, self.group)])
        for a in (self.Q, self.filler, self.rows, self.pos):
            a.setflags(write=False)

    # ---- the three forms of the train rows ----
    def compact(self, lo=0, hi=None):
        """(rows, map): the first filler block of [lo, hi) -- lo is a multiple of the block -- then its planted rows ascending;
        map[j] = the row of compact row j, counted from lo."""
        hi = self.n if hi is None else hi
        assert lo % self.block == 0 and hi - lo >= self.block
        sel = (self.pos >= lo) & (self.pos < hi)
        assert not ((self.pos[sel] - lo) < self.block).any()
        rows = np.concatenate([self.filler, self.rows[sel]])
        gmap = np.concatenate([np.arange(self.block, dtype=np.int64), self.pos[sel] - lo])
        return rows, gmap

    def expand(self):
        """Every row on the host (scaled-down cases only)."""
        assert self.n <= 1 << 16, "a full-size bank never exists on the host"
        T = np.tile(self.filler, (-(-self.n // self.block), 1))[:self.n].copy()
        T[self.pos] = self.rows
        return T

    def on_device(self, torch, lo=0, hi=None, device="cuda"):
        """Rows [lo, hi) as a device tensor: the filler repeated, the planted rows written with an index."""
        hi = self.n if hi is None else hi
        assert lo % self.block == 0
        n = hi - lo
        t = torch.from_numpy(np.array(self.filler)).to(device).repeat(-(-n // self.block), 1)
        if t.shape[0] != n:
            t = t[:n]
        sel = (self.pos >= lo) & (self.pos < hi)
        if sel.any():
            t[torch.from_numpy(self.pos[sel] - lo).to(device)] = torch.from_numpy(np.array(self.rows[sel])).to(device)
        assert t.is_contiguous()
        return t

    def describe(self, rows):
        return "; ".join(self.lay.label(r) for r in np.unique(np.asarray(rows).reshape(-1)) if r >= self.block)

    def first_neighbour(self, lo=0, hi=None):
        """Per query row, its nearest row of [lo, hi): the rank-0 row of the first group inside (counted from lo)."""
        hi = self.n if hi is None else hi
        out = np.full(self.nq, -1, np.int64)
        sel = (self.pos >= lo) & (self.pos < hi) & (self.rank == 0)
        for p, q in zip(self.pos[sel][::-1], self.owner[sel][::-1]):
            out[q] = p - lo
        assert (out >= 0).all()
        return out


@functools.lru_cache(maxsize=None)
def make_case(kind, mark, nq=NQ, base=None, block=BLOCK, tail=TAIL, seed=0):
    """The bank-pair case: one group, the whole bank behind its first filler block."""
    lay = Layout(kind, mark, base, tail)
    return Case(kind, lay, nq, block, [(block, lay.n)], 7700 + 10 * KINDS.index(kind) + MARKS.index(mark) + seed)


IMAGE_ROWS = 1 << 17


@functools.lru_cache(maxsize=None)
def make_collection_case(kind, mark, nq=NQ, base=None, block=BLOCK, image_rows=IMAGE_ROWS, seed=0):
    """A collection's stack as one bank: a first image of half the size, so that an image STRADDLES the mark, then whole
    images up to two behind the straddling one.  Groups: the straddling image, the next one and the last one.  Returns
    (case, first_row): first_row[i] = first row of image i, first_row[-1] = n."""
    half = image_rows // 2
    assert half % block == 0
    lay0 = Layout(kind, mark, base, 64)
    s = 1 + (lay0.m - half) // image_rows                # the image that holds row m
    n_images = s + 3
    first = np.concatenate([[0], half + image_rows * np.arange(n_images, dtype=np.int64)])
    assert first[s] < lay0.m - 33 and lay0.m + 33 < first[s + 1]
    lay = Layout(kind, mark, base, n=int(first[-1]))
    # (marks of the other planes may fall into other images: those images become groups too)
    imgs = sorted({int(np.searchsorted(first, c, side="right") - 1) for c in lay.crit} | {s, s + 1, n_images - 1})
    assert imgs[0] >= 1
    groups = [(int(first[i]) + block, int(first[i + 1])) for i in imgs]       # (an image keeps its own first filler block)
    case = Case(kind, lay, nq, block, groups, 8800 + 10 * KINDS.index(kind) + MARKS.index(mark) + seed)
    case.images = tuple(imgs)
    case.first_row = first
    return case


def build_on_host(kind, mark, **kw):
    return make_case(kind, mark, **kw).expand()


def build_on_device(torch, kind, mark, **kw):
    return make_case(kind, mark, **kw).on_device(torch)


# ---- the premise of the compact reference -----------------------------------------------------------------------------------
def exact_distances(kind, Q, T):
    """[nq, nt] in exact arithmetic: int64 squared distances / Hamming distances, float64 squared distances."""
    if kind == "bin":
        return hamming_ref.distances(Q, T).astype(np.int64)
    if kind == "u8":
        a, b = Q.astype(np.int64), T.astype(np.int64)
        return (a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2 * (a @ b.T)
    a, b = Q.astype(np.float64), T.astype(np.float64)
    return np.stack([((b - q) ** 2).sum(1) for q in a])


def check_condition(kind, Q, T, block, k=4, radius=None):
    """Asserts, for EVERY query row: at least k rows behind the first `block` rows of the compact set T (the planted rows) are
    strictly closer than every one of its first `block` rows (the filler) -- and the radius, if one is given, lies below the
    nearest filler row.  Float kinds: in float64 and in the float32 chain the kernels compute."""
    assert len(T) > block
    D = exact_distances(kind, Q, T)
    views = [(D[:, :block].min(axis=1), np.sort(D[:, block:], axis=1)[:, :k], kind == "bin")]
    if kind in ("f32", "wide"):
        # the float32 chain the kernels compute: the nearest filler row and the k nearest planted rows
        _, fd = oracle.bf_knn(Q, T[:block], 1, order=1)
        _, pd = oracle.bf_knn(Q, T[block:], k, order=1)
        views.append((fd[:, 0].astype(np.float64), pd.astype(np.float64), True))
    for nearest_filler, planted, plain in views:
        bad = np.nonzero(~(planted < nearest_filler[:, None]).all(axis=1))[0]
        assert len(bad) == 0, "query rows %s have fewer than %d planted rows closer than every filler row" % (bad[:8].tolist(), k)
        if radius is not None:
            r = np.broadcast_to(np.asarray(radius, np.float64), (len(Q),))
            assert ((r if plain else r * r) < nearest_filler).all(), "a radius reaches the filler"


# ---- references on a compact set, indices mapped back --------------------------------------------------------------------------
def _order(kind):
    return 1 if kind in ("f32", "wide") else 0


def knn(kind, Q, T, k):
    if kind == "bin":
        return hamming_ref.knn(Q, T, k)
    if kind == "wide":
        return wide_ref.knn(Q, T, k)
    return oracle.bf_knn(Q, T, k, order=_order(kind))


def xcheck1(kind, Q, T):
    if kind == "bin":
        return hamming_ref.xcheck(Q, T)
    if kind == "wide":
        return wide_ref.xcheck1(Q, T)
    return oracle.bf_xcheck1(Q, T, order=_order(kind))


def self_dist(kind, Q):
    if kind == "bin":
        return hamming_fast_ref.self_dist(Q)
    if kind == "wide":
        return wide_fast_ref.self_dist(Q)
    return oracle.self_dist(Q, order=_order(kind))


def _remap(idx, gmap):
    idx = np.asarray(idx)
    return np.where(idx >= 0, gmap[np.maximum(idx, 0)], -1).astype(np.int64)


def expected(kind, Q, T, gmap, tau=0.8, tau_acc=0.5, radius=RADIUS_LEVEL, sd=None, stacked=True):
    """Every result the tests compare, from the compact rows T, train indices mapped through gmap (int64):
    knn2, knn3 (idx, dist); xcheck1 (tidx, dist); ratio, accepted, mutual, mutual_sym (qidx, tidx, dist, ratio);
    radius (offsets, idx, dist).  stacked=False: without knn3 and radius (the per-image calls of a collection have neither)."""
    sd = self_dist(kind, Q) if sd is None else sd
    out = {}
    i2, d2 = knn(kind, Q, T, 2)
    out["knn2"] = (_remap(i2, gmap), d2)
    if stacked:
        i3, d3 = knn(kind, Q, T, 3)
        out["knn3"] = (_remap(i3, gmap), d3)
    tx, dx = xcheck1(kind, Q, T)
    out["xcheck1"] = (_remap(tx, gmap), dx)
    r = mutual_ratio_ref.ratios(i2, d2)
    with np.errstate(invalid="ignore"):
        q = np.nonzero(r < tau)[0].astype(np.int32)
    out["ratio"] = (q, _remap(i2[q, 0], gmap), d2[q, 0], r[q])
    if kind == "bin":
        acc = hamming_fast_ref.match_accepted(Q, T, sd, tau_acc)
    elif kind == "wide":
        acc = wide_fast_ref.fast_match(Q, T, tau_acc, sd)
    else:
        hit = np.nonzero(tx >= 0)[0].astype(np.int32)
        ratio, ok = oracle.ratio_filter(dx[hit], sd, tau_acc, qrows=hit)
        acc = (hit[ok], tx[hit][ok], dx[hit][ok], ratio[ok])
    out["accepted"] = (acc[0].astype(np.int32), _remap(acc[1], gmap), acc[2], acc[3])
    for name, sym in (("mutual", False), ("mutual_sym", True)):
        if kind == "bin":
            m = mutual_ratio_ref.mutual_ratio(Q, T, tau, sym, binary=True)
        elif kind == "wide":
            m = wide_ref.mutual_ratio(Q, T, tau, sym)
        else:
            m = grown_ref.ref_mutual_ratio(Q, T, tau, sym)
        out[name] = (m[0].astype(np.int32), _remap(m[1], gmap), m[2], m[3])
    if not stacked:
        return out
    if kind == "bin":
        ref = hamming_radius_ref.Ref(Q, T)
    elif kind == "wide":
        ref = wide_radius_ref.Ref(Q, (T,))
    else:
        ref = radius_coll_ref.Ref(Q, (T,))
    off, _, _, dist, idx = ref.cut(radius)
    out["radius"] = (off, _remap(idx, gmap), np.asarray(dist, np.float32))
    return out


def pairs_mutual_ratio(kind, Ta, Tb, block, tau, symmetric):
    """fm_mutual_ratio(a, b) of two images given as compact sets (first filler block, then planted rows), as far as the
    PLANTED rows of a go: (row of Ta, row of Tb, dist, ratio) of the accepted ones.  The filler rows of a need no reference: in
    the full images each has its exact copy in b more than once, d0 = d1 = 0, and 0 / 0 is never accepted.  The 2-NN lists
    come from knn() above; the three rules are fm_mutual_ratio's (tests/mutual_ratio_ref.py, wide_ref.py)."""
    Pa = Ta[block:]
    fi, fd = knn(kind, Pa, Tb, 2)
    t0 = fi[:, 0]
    ri, rd = knn(kind, Tb[t0], Ta, 2)
    fwd, rev = mutual_ratio_ref.ratios(fi, fd), mutual_ratio_ref.ratios(ri, rd)
    with np.errstate(invalid="ignore"):
        keep = (fwd < tau) & (ri[:, 0] == block + np.arange(len(Pa)))
        ratio = fwd
        if symmetric:
            keep &= rev < tau
            ratio = np.maximum(fwd, rev)
    q = np.nonzero(keep)[0]
    return (block + q).astype(np.int64), t0[q].astype(np.int64), fd[q, 0], ratio[q]


def radius_for(kind):
    """RADIUS_LEVEL in the kind's distance unit: levels 1 .. 3 of group 0 inside, level 4 and every other group outside."""
    return np.float32(RADIUS_LEVEL * (0.25 if kind in ("f32", "wide") else 1.0))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a
