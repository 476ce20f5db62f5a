"""Shared by test_hamming_radius_host.py and test_hamming_radius_gpu.py: the reference of Hamming radiusMatch, the tests'
data and a restatement of the sweep's split rule.  Nothing here touches the GPU.

Contract (include/fastmatch_hip.h, "Hamming radiusMatch"): h(q, t) = popcount(q XOR t), dist = (float32)h; train row j is in
query row i's list iff float32(h) < r_i (strict; r <= 0 or NaN nothing, r = +inf or r > W everything); a list ascends by
(h, train index) -- against a collection by (h, image, row inside the image), the global row turned into (image, row)
through the cumulative image sizes as radius_coll_ref.Ref does.  Every value is an integer: all comparisons are exact."""
import functools

import numpy as np

import hamming_ref

FLIPS = (0, 1, 2, 5, 17, 40)
NBASE = 24


def sweep_splits(nq, nt):
    """(splits, 128-row stages per split) of radius_ham_kernel's launch: a restatement of r_ham_stages_per_split
    (csrc/radius.hip) -- 256 query rows per workgroup, ~2048 workgroups, a split of at least 4 whole stages (K11's rule)."""
    qg = (nq + 255) // 256
    nstages = (nt + 127) // 128
    ns = max(1, min((2048 + qg - 1) // qg, (nstages + 3) // 4, 65535))
    sps = (nstages + ns - 1) // ns
    return ((nstages + sps - 1) // sps if sps else 1), sps


def clustered(n, nbytes, rng, base):
    """n rows: a random one of `base`'s rows with k of FLIPS (k <= W) random bits flipped."""
    W = 8 * nbytes
    rows = base[rng.integers(0, len(base), n)].copy()
    ks = [k for k in FLIPS if k <= W]
    for i in range(n):
        k = ks[rng.integers(0, len(ks))]
        if k:
            bits = rng.choice(W, k, replace=False)
            np.bitwise_xor.at(rows[i], bits >> 3, (1 << (bits & 7)).astype(np.uint8))
    return rows


@functools.lru_cache(maxsize=None)
def data(nbytes, nq=300, nt=2100, seed=0):
    """(Q, T) of the clustered recipe; train row nt // 2 is the bitwise complement of query row 5 (h = W)."""
    rng = np.random.default_rng(9100 + 131 * nbytes + seed)
    base = rng.integers(0, 256, (NBASE, nbytes), dtype=np.uint8)
    Q, T = clustered(nq, nbytes, rng, base), clustered(nt, nbytes, rng, base)
    if nq > 5 and nt > 0:
        T[nt // 2] = ~Q[5]
    Q.setflags(write=False)
    T.setflags(write=False)
    return Q, T


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class Ref(object):
    """All distances of Q against T (or against the stacked images), computed once; cut per call."""

    def __init__(self, Q, T_or_images):
        images = list(T_or_images) if isinstance(T_or_images, (list, tuple)) else [T_or_images]
        self.nq = len(Q)
        self.W = 8 * Q.shape[1]
        sizes = [im.shape[0] for im in images]
        self.total = int(sum(sizes))
        T = np.concatenate(images) if images else np.zeros((0, Q.shape[1]), np.uint8)
        self.h = hamming_ref.distances(Q, T).astype(np.float32) if self.nq and self.total else np.zeros((self.nq, self.total), np.float32)
        # (h, index) ascending per row: a stable sort of h over ascending indices
        self.order = np.argsort(self.h, axis=1, kind="stable").astype(np.int32)
        self.sorted = np.take_along_axis(self.h, self.order, axis=1)
        fr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        self.img = (np.searchsorted(fr, self.order, side="right") - 1).astype(np.int32)
        self.loc = (self.order - fr[self.img]).astype(np.int32)

    def cut(self, r):
        """(offsets int64 [nq + 1], img, idx inside the image, dist, global idx) of the lists float32(h) < r_i, flat."""
        rr = np.broadcast_to(np.asarray(r, dtype=np.float32), (self.nq,))
        with np.errstate(invalid="ignore"):
            m = self.sorted < rr[:, None]
        off = np.concatenate([[0], np.cumsum(m.sum(axis=1))]).astype(np.int64)
        return off, self.img[m], self.loc[m], self.sorted[m], self.order[m]

    def counts(self, r):
        return np.diff(self.cut(r)[0])


@functools.lru_cache(maxsize=None)
def data_ref(nbytes, nq=300, nt=2100, seed=0):
    return Ref(*data(nbytes, nq, nt, seed))


def mixed_radii(ref, seed=1):
    """One radius per row from the reference's own distances -- h exactly (alternate rows) or nextafter(h, +inf) -- with
    0, a negative value, NaN and +inf at several rows each."""
    rng = np.random.default_rng(seed)
    hi = min(40, ref.total - 1)
    r = np.array([ref.sorted[i, rng.integers(0, hi + 1)] for i in range(ref.nq)], np.float32)
    r[1::2] = np.nextafter(r[1::2], np.float32(np.inf))
    for j, v in enumerate((0.0, -3.0, np.nan, np.inf)):
        r[7 + j::41] = v
    return r


def same_pair_lists(got, want, what=""):
    """got = (offsets, idx, dist); want = Ref.cut(...).  Indices exactly, distances as bit patterns."""
    off, idx, dist = got
    woff, _, _, wdist, wglobal = want
    assert off.dtype == np.int64 and np.array_equal(off, woff), what + " offsets"
    assert idx.shape == dist.shape == (int(woff[-1]),), what + " sizes"
    assert np.array_equal(idx, wglobal), what + " idx"
    assert np.array_equal(bits(dist), bits(wdist)), what + " dist"


def same_coll_lists(got, want, what=""):
    off, img, idx, dist = got
    woff, wimg, widx, wdist = want[:4]
    assert off.dtype == np.int64 and np.array_equal(off, woff), what + " offsets"
    assert img.shape == idx.shape == dist.shape == (int(woff[-1]),), what + " sizes"
    assert np.array_equal(img, wimg), what + " img"
    assert np.array_equal(idx, widx), what + " idx"
    assert np.array_equal(bits(dist), bits(wdist)), what + " dist"
