"""The reference of radiusMatch on wide float descriptors (129 .. 256 values per row), shared by test_wide_radius_host.py,
test_wide_radius_gpu.py and test_wide_radius_collection_gpu.py.  oracle.bf_knn(Q, T, k = all rows, order=1) -- the float32
chain s = fmaf(v, v, s), k ascending, which takes any dim -- gives every query row's full list ascending by (distance, train
index); a call's answer is that list cut at dist < r_i, a strict float32 compare.  The oracle lists no NaN and no +inf
distance (they come back as -1 / +inf behind the real entries), and inf < inf is false: such a pair is in no list, whatever r.
For a collection the train rows are the images' rows concatenated, and a global row becomes (image, row inside the image)
through the cumulative image sizes, as in radius_coll_ref.Ref.  The oracle runs once per data set; nothing here touches the GPU
or the library under test."""
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (_HERE, os.path.dirname(_HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import oracle           # noqa: E402

DIMS = [129, 160, 161, 192, 193, 224, 255, 256]     # K steps of 32: 5, 5, 6, 6, 7, 7, 8, 8 -- both sides of every boundary
KSTEPS = {129: 5, 160: 5, 161: 6, 192: 6, 193: 7, 224: 7, 255: 8, 256: 8}
SHAPES = [(0, 5), (5, 0), (1, 1), (1, 300), (127, 129), (129, 127), (300, 1100)]
SMALL = SHAPES[:4]                                  # at every dim; the others at 129 and 256 only
SIZES = [300, 0, 128, 1, 65, 129, 700, 100]         # radius_coll_ref.SIZES: padding behind every image, an empty image, a
NQ = 300                                            # split inside an image; 300 query rows


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class Ref(object):
    """The full ascending lists of Q against the stacked images (a bank pair: one image), cut per call."""

    def __init__(self, Q, images):
        Q = np.ascontiguousarray(Q, np.float32)
        images = [np.ascontiguousarray(im, np.float32) for im in images]
        self.nq = len(Q)
        sizes = [im.shape[0] for im in images]
        self.total = int(sum(sizes))
        if self.nq and self.total:
            T = np.concatenate([im for im in images if im.shape[0]])
            self.idx, self.dist = oracle.bf_knn(Q, T, self.total, order=1)
        else:
            self.idx = np.zeros((self.nq, 0), np.int32)
            self.dist = np.zeros((self.nq, 0), np.float32)
        fr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        safe = np.maximum(self.idx, 0)
        self.img = (np.searchsorted(fr, safe, side="right") - 1).astype(np.int32)
        self.loc = (safe - fr[self.img]).astype(np.int32) if self.total else self.idx
        self.idx.setflags(write=False)
        self.dist.setflags(write=False)

    def cut(self, r):
        """(offsets int64 [nq + 1], img, idx inside the image, dist, global idx) of the lists dist < r_i, flat."""
        rr = np.broadcast_to(np.asarray(r, dtype=np.float32), (self.nq,))
        with np.errstate(invalid="ignore"):
            m = (self.dist < rr[:, None]) & (self.idx >= 0)
        off = np.concatenate([[0], np.cumsum(m.sum(axis=1))]).astype(np.int64)
        return off, self.img[m], self.loc[m], self.dist[m], self.idx[m]

    def kth(self, k):
        """A scalar radius that gives about k hits per row: the median k-th distance, nudged up."""
        k = min(k, self.dist.shape[1] - 1)
        fin = self.dist[:, k][np.isfinite(self.dist[:, k])]
        return np.nextafter(np.float32(np.median(fin)), np.float32(np.inf))


def mixed_radii(ref, seed=1):
    """One radius per row.  Even rows: EXACTLY one of the row's own distances (that entry and its ties are excluded: the
    compare is strict); odd rows: the float32 after it (included).  0, a negative value, NaN and +inf at several rows, and one
    row with a radius beyond every finite distance (it lists every train row that has a finite distance)."""
    rng = np.random.default_rng(seed)
    n = ref.dist.shape[1]
    r = np.empty(ref.nq, np.float32)
    for i in range(ref.nq):
        d = ref.dist[i, rng.integers(0, min(12, n))] if n else np.float32(1.0)
        if not np.isfinite(d):
            d = np.float32(1.0)
        r[i] = d if i % 2 == 0 else np.nextafter(np.float32(d), np.float32(np.inf))
    for j, v in enumerate((0.0, -3.0, np.nan, np.inf)):
        r[7 + j::41] = v
    if ref.nq > 3 and n:
        r[3] = np.float32(3.0e38)
    return r


def same_pair(got, want, what=""):
    """got = (offsets, idx, dist) of a bank pair; want = Ref.cut(...).  Indices exactly, distances as bit patterns."""
    off, idx, dist = got
    woff, _, _, wdist, wglobal = want
    assert off.dtype == np.int64 and np.array_equal(off, woff), "%s offsets" % (what,)
    assert idx.shape == dist.shape == (int(woff[-1]),), "%s sizes" % (what,)
    assert np.array_equal(idx, wglobal), "%s idx" % (what,)
    assert np.array_equal(bits(dist), bits(wdist)), "%s dist" % (what,)


def same_lists(got, want, what=""):
    """got = (offsets, img, idx, dist) of a collection; want = Ref.cut(...)."""
    off, img, idx, dist = got
    woff, wimg, widx, wdist = want[:4]
    assert off.dtype == np.int64 and np.array_equal(off, woff), "%s offsets" % (what,)
    assert img.shape == idx.shape == dist.shape == (int(woff[-1]),), "%s sizes" % (what,)
    assert np.array_equal(img, wimg), "%s img" % (what,)
    assert np.array_equal(idx, widx), "%s idx" % (what,)
    assert np.array_equal(bits(dist), bits(wdist)), "%s dist" % (what,)


def split_images(T, sizes=SIZES):
    """T's rows cut into images of the given sizes."""
    assert len(T) == sum(sizes)
    return [np.ascontiguousarray(im) for im in np.split(T, np.cumsum(sizes)[:-1])]
