"""Reference side of the grown-bank tests (test_grown_banks_host.py, test_grown_banks_gpu.py); not a test.

A bank that grows (fm_bank_append_u8 / fm_bank_append_f32) places every append at the next multiple of 32 rows; the rows
skipped in between are padding rows INSIDE the bank ("gap rows").  ``Layout`` restates that arithmetic from the header's
contract -- physical row of every real row, the gap rows, the dense matrix of the real rows -- and the ``ref_*`` functions
compute what a dense call must return: the oracle (``oracle.bf_knn`` / ``bf_xcheck1``, ``order=1`` for float32) and the NumPy
compositions of the other reference modules, on the REAL rows only, with the indices turned into physical rows afterwards.

Results come in two shapes, which is all the remapping needs to know:
  LISTS  (idx int32 [n, k], dist float32 [n, k])                  one output row per query row (knn, xcheck1 as k = 1)
  ROWS   (qidx int32 [m], tidx int32 [m], dist float32 [m], ...)  accepted / listed pairs, ascending query row (knn2_ratio,
         mutual_ratio, match_accepted; radius lists flattened to one row per entry)
Nothing here calls the code under test."""
import functools
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (_HERE, os.path.dirname(_HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import masked_ref           # noqa: E402
import mutual_ratio_ref     # noqa: E402
import oracle               # noqa: E402
import radius_coll_ref      # noqa: E402
from fastmatch_amd import synth   # noqa: E402

TILE = 32                                   # an append starts on a whole MFMA tile
PATTERNS = {"in_stage": (1, 31, 32, 33, 0, 100, 64, 5),      # gaps inside one 128-row stage, an empty append, 357 physical rows
            "across": (129, 1, 127)}                          # gaps that run across a stage boundary, 319 physical rows
N_OTHER = 300                               # rows of the bank on the other side: two 256-row workgroups


class Layout(object):
    """Where the rows of a list of appends (row counts or row arrays, possibly empty) land."""

    def __init__(self, appends):
        sizes = [int(a) if np.ndim(a) == 0 else int(np.asarray(a).shape[0]) for a in appends]
        self.sizes = sizes
        self.first = []                     # *first_row of every append, the empty ones included
        n = 0                               # the bank's row count so far (bank->n)
        phys = []
        for s in sizes:
            off = (n + TILE - 1) // TILE * TILE
            self.first.append(off)
            if s:
                phys.extend(range(off, off + s))
                n = off + s
        self.n_phys = n
        self.phys = np.asarray(phys, dtype=np.int64)                                  # physical row of real row i
        self.n_real = self.phys.shape[0]
        self.real_of = np.full(n, -1, dtype=np.int64)                                 # real row of physical row p, -1: a gap row
        self.real_of[self.phys] = np.arange(self.n_real)
        self.gaps = np.nonzero(self.real_of < 0)[0]

    def dense(self, appends):
        """The real rows of the row arrays ``appends`` as one matrix."""
        return np.concatenate([np.asarray(a) for a in appends if np.asarray(a).shape[0]])

    def split(self, rows):
        """The dense matrix cut back into this layout's appends."""
        cuts = np.cumsum(self.sizes)[:-1]
        return [np.ascontiguousarray(p) for p in np.split(rows, cuts)]

    def to_phys(self, idx):
        """Real-row indices -> physical rows; -1 stays -1."""
        idx = np.asarray(idx)
        return np.where(idx >= 0, self.phys[np.maximum(idx, 0)], -1).astype(idx.dtype)

    def to_real(self, idx):
        """Physical rows -> real-row indices; -1 stays -1, a gap row becomes -2."""
        idx = np.asarray(idx)
        return np.where(idx >= 0, np.where(self.real_of[np.maximum(idx, 0)] >= 0, self.real_of[np.maximum(idx, 0)], -2), -1).astype(idx.dtype)

    # --- remapping of results ---------------------------------------------------------------------------------------------
    def lists_train(self, res):
        """LISTS computed against the real train rows -> against the grown train bank."""
        return (self.to_phys(res[0]),) + tuple(res[1:])

    def rows_train(self, res):
        return (res[0], self.to_phys(res[1])) + tuple(res[2:])

    def lists_query(self, res):
        """LISTS a call returned for a grown QUERY bank -> its output rows at the real positions."""
        return tuple(np.asarray(a)[self.phys] for a in res)

    def rows_query(self, res):
        """ROWS a call returned for a grown QUERY bank -> the rows of real query rows, numbered as real rows."""
        q = self.real_of[np.asarray(res[0], dtype=np.int64)]
        keep = q >= 0
        return (q[keep].astype(np.int32),) + tuple(np.asarray(a)[keep] for a in res[1:])


def gap_row(kind, dim):
    """What a gap row holds, in the caller's units: uint8 banks store byte - 128 and a padding row of zeros, float32 banks a
    zero row."""
    return np.full(dim, 128.0) if kind == "u8" else np.zeros(dim)


def d2_f64(A, B):
    a, b = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    return (a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2.0 * (a @ b.T)


def gap_is_nearest(kind, grown_rows, other_rows):
    """Per row of ``other_rows``: is a gap row strictly nearer (float64) than EVERY real row of the grown bank?"""
    other = np.asarray(other_rows, dtype=np.float64)
    dgap = ((other - gap_row(kind, other.shape[1])[None, :]) ** 2).sum(1)
    return dgap < d2_f64(other, grown_rows).min(axis=1)


def _draw(kind, n, dim, rng):
    if kind == "u8":
        return rng.integers(0, 256, (n, dim), dtype=np.uint8)           # uniform bytes: d2 to the all-128 row ~ dim * 5461
    return rng.normal(0.0, 1.0, (n, dim)).astype(np.float32)            # N(0, 1): |row|^2 ~ dim against 2 dim to a real row


def adversarial(kind, dim, n_grown, n_other, seed):
    """(grown rows, other rows) on which a kernel that scores gap rows fails at EVERY row of the other bank: uniform bytes /
    N(0, 1) values, where a gap row lies at about half the squared distance of a real row.  "About" leaves a tail (a few rows
    in a hundred at dim 61), so the other bank's rows are the first n_other draws for which the gap row really is nearer than
    every real row; gap_is_nearest checks the outcome in float64."""
    rng = np.random.default_rng(seed)
    G = _draw(kind, n_grown, dim, rng)
    out = []
    have = 0
    for _ in range(64):
        C = _draw(kind, 4 * n_other, dim, rng)
        C = C[gap_is_nearest(kind, G, C)]
        out.append(C)
        have += C.shape[0]
        if have >= n_other:
            break
    O = np.concatenate(out)[:n_other]
    assert O.shape[0] == n_other, "adversarial: too few rows with a gap row nearest"
    return G, np.ascontiguousarray(O)


def siftlike(kind, dim, n_grown, n_other, seed):
    """(grown rows, other rows) SIFT-like with planted matches (synth.planted_pair): gap rows lie far from everything and must
    simply be absent.  float32: the same rows off the integers."""
    O, G, _ = synth.planted_pair(n_other, n_grown, seed=seed, dim=dim)
    if kind != "u8":
        rng = np.random.default_rng(seed + 1)
        G, O = radius_coll_ref.floaty(G, rng), radius_coll_ref.floaty(O, rng)
    return G, O


RESCAN_PATTERN = (1, 31, 32, 33, 0, 60)      # 157 real rows in 220 physical ones (gaps inside a stage and across one): as output
                                             # rows of fm_self_dist all 220 may need a rescan, which 256 rows of a call can get
RESCAN_SMALL = 100                           # tiny rows among them
RESCAN_OTHER = 200                           # rows of the other bank: all of them get a per-row rescan, which takes 256 at most


@functools.lru_cache(maxsize=None)
def rescan_dataset(seed=7400):
    """(Layout, grown rows, other rows), float32, for the fp16 filter route's per-row exact rescan (filter_f16.hip): an output
    row whose candidate list may be incomplete -- a lane's last kept entry lies within the filter's margin, about
    1e-3 (|row|^2 + the bank's largest |row|^2) -- is scanned again over ALL rows of the other bank, by index.
      grown bank : RESCAN_SMALL tiny rows (0.005 N(0, 1), in the upper 64 dimensions only) among full N(0, 1) rows, shuffled;
      other bank : N(0, 1) in the lower 64 dimensions only.
    Every other-bank row o is at d2 = |o|^2 + |c|^2 from every tiny row c (orthogonal supports): a hundred candidates within
    3e-3 of each other, far inside the margin (~0.3), so its list cannot be known complete; the full rows lie at
    |o|^2 + ~128.  A gap row (zeros) is at |o|^2: strictly nearer than every real row.  Among themselves the tiny rows are
    the same: neighbours at ~|c|^2 + |c'|^2, the zero row at |c|^2 (fm_self_dist)."""
    rng = np.random.default_rng(seed)
    lay = Layout(RESCAN_PATTERN)
    G = rng.normal(0.0, 1.0, (lay.n_real, 128)).astype(np.float32)
    small = rng.permutation(lay.n_real)[:RESCAN_SMALL]
    tiny = np.zeros((RESCAN_SMALL, 128), np.float32)
    tiny[:, 64:] = (0.005 * rng.normal(0.0, 1.0, (RESCAN_SMALL, 64))).astype(np.float32)
    G[small] = tiny
    O = np.zeros((RESCAN_OTHER, 128), np.float32)
    O[:, :64] = rng.normal(0.0, 1.0, (RESCAN_OTHER, 64)).astype(np.float32)
    G.setflags(write=False)
    O.setflags(write=False)
    return lay, G, O, np.sort(small)


@functools.lru_cache(maxsize=None)
def dataset(kind, pattern, dim, data):
    """(Layout, the grown bank's real rows, the other bank's rows) of a test case; kind "u8" / "f32", data "adv" / "sift".
    Computed once, read-only."""
    lay = Layout(PATTERNS[pattern])
    seed = 7100 + 1000 * sorted(PATTERNS).index(pattern) + dim + (500 if kind == "u8" else 0)
    G, O = (adversarial if data == "adv" else siftlike)(kind, dim, lay.n_real, N_OTHER, seed)
    G, O = np.ascontiguousarray(G), np.ascontiguousarray(O)
    G.setflags(write=False)
    O.setflags(write=False)
    return lay, G, O


def order_of(rows):
    return 1 if np.asarray(rows).dtype == np.float32 else 0


# --- expected results on the real rows (Q, T dense matrices) ---------------------------------------------------------------
def ref_knn(Q, T, k):
    return oracle.bf_knn(Q, T, k, order=order_of(Q))


def ref_xcheck1(Q, T):
    t, d = oracle.bf_xcheck1(Q, T, order=order_of(Q))
    return t.reshape(-1, 1), d.reshape(-1, 1)


def ref_knn2_ratio(Q, T, tau):
    idx, dist = ref_knn(Q, T, 2)
    r = mutual_ratio_ref.ratios(idx, dist)
    with np.errstate(invalid="ignore"):
        q = np.nonzero(r < tau)[0]
    return q.astype(np.int32), idx[q, 0], dist[q, 0], r[q]


def ref_mutual_ratio(Q, T, tau, symmetric):
    """mutual_ratio_ref.mutual_ratio's three rules on 2-NN lists in the device's float32 order (that module asks the oracle
    in its default order, which is OpenCV's)."""
    k_idx, k_dist = ref_knn(Q, T, 2)
    r_idx, r_dist = ref_knn(T, Q, 2)
    fwd, rev_t = mutual_ratio_ref.ratios(k_idx, k_dist), mutual_ratio_ref.ratios(r_idx, r_dist)
    t0 = k_idx[:, 0]
    with np.errstate(invalid="ignore"):
        keep = (fwd < tau) & (r_idx[t0, 0] == np.arange(len(Q)))
        ratio = fwd
        if symmetric:
            keep &= rev_t[t0] < tau
            ratio = np.maximum(fwd, rev_t[t0])
    q = np.nonzero(keep)[0]
    return q.astype(np.int32), t0[q].astype(np.int32), k_dist[q, 0], ratio[q]


def ref_radius(Q, T, r):
    """ROWS (qidx, tidx, dist): every pair with dist < r_i, per query row ascending (distance bits, train row)."""
    off, _, _, dist, idx = radius_coll_ref.Ref(Q, (T,)).cut(r)
    q = np.repeat(np.arange(len(Q), dtype=np.int32), np.diff(off))
    return q, idx.astype(np.int32), dist


def radius_rows(res):
    """Context.radius_match's (offsets, idx, dist) as ROWS."""
    off, idx, dist = res
    return np.repeat(np.arange(len(off) - 1, dtype=np.int32), np.diff(off)), idx, dist


def ref_knn_masked(Q, T, mask, k):
    return masked_ref.knn("f32" if order_of(Q) else "u8", Q, T, mask, k)


def ref_self_dist(T):
    return oracle.self_dist(T, order=order_of(T))


def ref_match_accepted(Q, T, selfdist, tau):
    t, d = oracle.bf_xcheck1(Q, T, order=order_of(Q))
    q = np.nonzero(t >= 0)[0].astype(np.int32)
    ratio, ok = oracle.ratio_filter(d[q], selfdist, tau, qrows=q)
    return q[ok], t[q][ok], d[q][ok], ratio[ok]
