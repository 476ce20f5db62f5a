"""Shared by test_collection_radius_gpu.py and test_radius_dev_gpu.py: the collection layout of the radius tests, their
data, and the reference lists -- oracle.bf_knn on the concatenated rows with k = all rows (full lists: no k_cap to satisfy),
cut at dist < r_i, every global row turned into (image, row) through the cumulative image sizes.  The oracle runs once
per data set (cached); nothing here touches the GPU."""
import functools

import numpy as np

import oracle
from fastmatch_amd import synth

# 1920 physical rows, 1423 real: padding in the middle, a full stage (128), a stage whose second 64-row half is all
# padding (1, 65, 129), an empty image; the sweep cuts the 1920 rows into two splits of 960, inside the 128-row stage
# [896, 1024) of the 129-row image.
SIZES = [300, 0, 128, 1, 65, 129, 700, 100]
NQ = 300                                    # not a multiple of 256: two workgroups
ROUTES = ["i8", "f32"]


def pad128(n):
    return (n + 127) // 128 * 128


def sweep_splits(nq, nt):
    """(splits, rows per split) of K10's sweeps: a restatement of r_splits / r_sweep (csrc/radius.hip) -- 256 query rows per
    workgroup, ~2048 workgroups, a split of at least 1024 train rows, rounded up to the 64-row stage."""
    qg = (nq + 255) // 256
    s = max(1, min((2048 + qg - 1) // qg, (nt + 1023) // 1024, 65535))
    per = ((nt + s - 1) // s + 63) // 64 * 64
    return s, per


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def floaty(U, rng):
    """Non-integer float32 rows on the SIFT range."""
    return (U + rng.uniform(-0.5, 0.5, U.shape)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def layout(route, variant=""):
    """(Q, images) of the standard layout.  variant "wide" (float32 route): the last image times 10 leaves fp16's range under
    the scale the first image fixed, which switches the collection's fp16 filter off (the all-pairs path)."""
    rng = np.random.default_rng(20250 + len(variant))
    U = synth.synth_sift(NQ + sum(SIZES), rng)
    if route == "f32":
        U = floaty(U, rng)
    Q, rest = U[:NQ], U[NQ:]
    cuts = np.cumsum(SIZES)[:-1]
    images = [im.copy() for im in np.split(rest, cuts)]
    if variant == "wide":
        images[-1] = (images[-1] * np.float32(10.0)).astype(np.float32)
    Q.setflags(write=False)
    for im in images:
        im.setflags(write=False)
    return Q, tuple(images)


class Ref(object):
    """The full ascending lists of Q against the stacked images (computed once), cut per call."""

    def __init__(self, Q, images):
        self.nq = len(Q)
        sizes = [im.shape[0] for im in images]
        self.total = int(sum(sizes))
        if self.nq and self.total:
            T = np.concatenate([im for im in images if im.shape[0]])
            order = 1 if T.dtype == np.float32 else 0
            self.idx, self.dist = oracle.bf_knn(Q, T, self.total, order=order) if order else oracle.bf_knn(Q, T, self.total)
        else:
            self.idx = np.zeros((self.nq, 0), np.int32)
            self.dist = np.zeros((self.nq, 0), np.float32)
        fr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        self.img = (np.searchsorted(fr, self.idx, side="right") - 1).astype(np.int32)
        self.loc = (self.idx - fr[self.img]).astype(np.int32) if self.total else self.idx

    def cut(self, r):
        """(offsets int64 [nq + 1], img, idx, dist, global idx) of the lists dist < r_i, flat."""
        rr = np.broadcast_to(np.asarray(r, dtype=np.float32), (self.nq,))
        with np.errstate(invalid="ignore"):
            m = self.dist < rr[:, None]
        off = np.concatenate([[0], np.cumsum(m.sum(axis=1))]).astype(np.int64)
        return off, self.img[m], self.loc[m], self.dist[m], self.idx[m]

    def kth(self, k):
        """A scalar radius that gives about k hits per row: the median k-th distance, nudged up."""
        return np.nextafter(np.float32(np.median(self.dist[:, k])), np.float32(np.inf))


@functools.lru_cache(maxsize=None)
def layout_ref(route, variant=""):
    return Ref(*layout(route, variant))


def mixed_radii(ref, seed=1):
    """One radius per row: 0, a negative value, NaN and +inf among ordinary ones (each special value at several rows)."""
    rng = np.random.default_rng(seed)
    r = np.array([ref.dist[i, rng.integers(0, 12)] for i in range(ref.nq)], np.float32)
    r = np.nextafter(r, np.float32(np.inf))
    for j, v in enumerate((0.0, -3.0, np.nan, np.inf)):
        r[7 + j::41] = v
    return r


def same_lists(got, want, what=""):
    """got = (offsets, img, idx, dist) NumPy arrays; want = Ref.cut(...).  Indices exactly, distances as bit patterns."""
    off, img, idx, dist = got
    woff, wimg, widx, wdist = want[:4]
    assert off.dtype == np.int64 and np.array_equal(off, woff), what + " offsets"
    assert img.shape == idx.shape == dist.shape == (int(woff[-1]),), what + " sizes"
    assert np.array_equal(img, wimg), what + " img"
    assert np.array_equal(idx, widx), what + " idx"
    assert np.array_equal(bits(dist), bits(wdist)), what + " dist"
