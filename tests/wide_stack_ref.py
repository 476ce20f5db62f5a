"""The reference of the stacked knnMatch calls on a wide train collection (fm_collection_wide_knn, _wide_knn2_ratio,
_wide_votes), shared by test_wide_stack_host.py and test_wide_stack_gpu.py.  wide_ref.knn (oracle.bf_knn, order 1: the float32
chain s = fmaf(v, v, s), k ascending) on the images' rows CONCATENATED gives every query row's list ascending by (distance
bits, global row); a global row becomes (image, row inside the image) by searchsorted on the images' first rows -- global
order is (image, row) order, so ties fall to the earlier image, then the earlier row.  The concatenation holds real rows only:
the reference cannot return one of the stack's padding rows, whatever lies nearer.  Nothing here touches the GPU or the
library under test."""
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)
import wide_ref                     # noqa: E402
from wide_radius_ref import SIZES   # noqa: E402,F401   [300, 0, 128, 1, 65, 129, 700, 100]: padding of 0 / 1 / 63 / 127 rows, an empty image

SIZES_EMPTY_ENDS = [0] + SIZES + [0]        # the same with an empty image first and one last
NQS = [0, 1, 127, 129, 300]
FULL_DIMS = [129, 256]
SMALL_DIMS = [160, 161, 192, 193, 224, 255]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def concat(images, dim):
    live = [np.ascontiguousarray(im, np.float32) for im in images if len(im)]
    return np.concatenate(live) if live else np.zeros((0, dim), np.float32)


def first_rows(images):
    return np.concatenate([[0], np.cumsum([len(im) for im in images])]).astype(np.int64)


def locate(images, g):
    """Global rows of the concatenation -> (image, row inside the image); -1 stays -1 / -1.  searchsorted from the right skips
    the empty images that share a first row."""
    fr = first_rows(images)
    g = np.asarray(g, np.int64)
    img = (np.searchsorted(fr, np.maximum(g, 0), side="right") - 1).astype(np.int32)
    loc = (np.maximum(g, 0) - fr[img]).astype(np.int32)
    return np.where(g >= 0, img, -1).astype(np.int32), np.where(g >= 0, loc, -1).astype(np.int32)


def knn(Q, images, k):
    """fm_collection_wide_knn: (img, idx, dist) [nq, k]."""
    Q = np.ascontiguousarray(Q, np.float32)
    g, dist = wide_ref.knn(Q, concat(images, Q.shape[1]), k)
    img, loc = locate(images, g)
    return img, loc, np.ascontiguousarray(dist, np.float32)


def ratio_match(Q, images, tau):
    """fm_collection_wide_knn2_ratio with cap = nq: (qidx, img, tidx, dist, ratio), ascending query index; float64 d0 / d1 < tau,
    a missing or zero second distance fails (x / 0 is inf or NaN: neither is < tau unless tau is +inf, which d1 == 0 excludes
    by rule)."""
    img, loc, dist = knn(Q, images, 2)
    r = wide_ref.ratios(loc, dist)
    with np.errstate(invalid="ignore"):
        keep = (r < tau) & (dist[:, 1] != 0)
    q = np.nonzero(keep)[0]
    return q.astype(np.int32), img[q, 0], loc[q, 0], dist[q, 0], r[q]


def votes(Q, images, tau, mode):
    """fm_collection_wide_votes: int64 [n_images].  Mode 0: ratio_match's rows counted at their image; mode 1: the same test on
    every image's own 2-NN lists, counted at that image."""
    out = np.zeros(len(images), np.int64)
    if mode == 0:
        np.add.at(out, ratio_match(Q, images, tau)[1], 1)
    else:
        for i, im in enumerate(images):
            out[i] = len(ratio_match(Q, [im], tau)[0])
    return out


def votes_from_each(idx, dist, tau):
    """Mode 1's counts from per-image lists [n_images, nq, 2] (fm_collection_wide_knn2_each's)."""
    out = np.zeros(idx.shape[0], np.int64)
    for i in range(idx.shape[0]):
        r = wide_ref.ratios(idx[i], dist[i])
        with np.errstate(invalid="ignore"):
            out[i] = int(((r < tau) & (dist[i][:, 1] != 0)).sum())
    return out


# ---- data ---------------------------------------------------------------------------------------------------------------------
def split(T, sizes):
    assert len(T) == sum(sizes)
    return [np.ascontiguousarray(im) for im in np.split(T, np.cumsum(sizes)[:-1])]


def unit_images(nq, sizes, dim, seed):
    """Unrelated unit-norm rows: every real neighbour lies at about 1.41, a zero (padding) row at exactly |q| = 1.0 -- NEARER
    than every real row."""
    rng = np.random.default_rng(seed)
    Q = wide_ref._unit(rng.standard_normal((nq, dim)))
    T = wide_ref._unit(rng.standard_normal((sum(sizes), dim)))
    return Q, split(T, sizes)


def clustered_images(nq, sizes, dim, seed):
    """wide_ref.clustered cut into images: every query row a near copy of a train row."""
    Q, T = wide_ref.clustered(nq, max(sum(sizes), 1), dim, seed)
    return Q, split(T[:sum(sizes)], sizes)


def tied_images(dim, seed):
    """(Q, images): query rows 0 .. 9 are EXACT copies of a row that is present twice in image 1 and once in image 3; the other
    query rows have no copy.  The top-2 of a copied row is (image 1, the lower row) then (image 1, the higher row), distance 0."""
    Q, images = clustered_images(40, [150, 200, 0, 130], dim, seed)
    for j in range(10):
        row = images[0][j].copy()
        Q[j] = row
        images[1][190 - 3 * j] = row
        images[1][20 + j] = row
        images[3][5 + j] = row
        images[0][j] = images[0][100 + j]          # (the source row itself goes: image 0 holds no copy)
    return Q, images


def overflow_images(seed=11):
    """wide_masked_ref.overflow_cluster's shape -- 2100 copies of one row among 2304 train rows, 600 query rows next to it, dim
    129 -- with the train rows cut into two images, so the copies are spread over both: 600 x 2100 = 1.26 million pairs lie
    inside the filter's margin, against 2^20 list records.  fewer: the same with all but 700 of the copies replaced -- 420000
    pairs, which fit."""
    import wide_masked_ref
    Q, T, _ = wide_masked_ref.overflow_cluster(seed)
    # the copied row: the most frequent row of T
    _, inv, cnt = np.unique(T, axis=0, return_inverse=True, return_counts=True)
    copies = np.nonzero(inv.ravel() == cnt.argmax())[0]
    assert len(copies) == 2100
    sizes = [1000, 1304]
    assert 0 < (copies < 1000).sum() < 2100
    rng = np.random.default_rng(seed + 1)
    F = T.copy()
    F[copies[700:]] = rng.standard_normal((1400, T.shape[1])).astype(np.float32)
    return Q, split(T, sizes), split(F, sizes)
