"""NumPy reference of fm_collection_xcheck1_each: cv2.BFMatcher(norm, crossCheck=True).match(Q, image) image by image
(oracle.bf_xcheck1 for NORM_L2 -- the fma chain, order 1, for float32 rows --, hamming_ref.xcheck for binary rows), the
max_dist filter, and the compacted rows of the device form."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hamming_ref               # noqa: E402
import oracle                    # noqa: E402


def xcheck_pair(Q, T, binary=False):
    """(tidx int32 [nq], dist float32 [nq]) of one image: -1 / inf where no row of T that elects the query row exists."""
    nq = Q.shape[0]
    if nq == 0 or T.shape[0] == 0:
        return np.full(nq, -1, np.int32), np.full(nq, np.inf, np.float32)
    if binary:
        return hamming_ref.xcheck(Q, T)
    return oracle.bf_xcheck1(Q, T, order=1 if Q.dtype == np.float32 else 0)


def keep(tidx, dist, max_dist=np.inf):
    """A match stays iff dist < max_dist, a strict float32 compare (NaN and values <= 0 keep none); the dropped entries
    read -1 / inf.  Returns new arrays."""
    tidx, dist = np.array(tidx, np.int32), np.array(dist, np.float32)
    with np.errstate(invalid="ignore"):
        stay = (tidx >= 0) & (dist < np.float32(max_dist))
    tidx[~stay] = -1
    dist[~stay] = np.inf
    return tidx, dist


def xcheck_each(Q, images, binary=False, max_dist=np.inf):
    """(tidx int32 [n_images, nq], dist float32 [n_images, nq])"""
    nq = Q.shape[0]
    tidx, dist = np.full((len(images), nq), -1, np.int32), np.full((len(images), nq), np.inf, np.float32)
    for i, im in enumerate(images):
        tidx[i], dist[i] = keep(*xcheck_pair(Q, im, binary), max_dist=max_dist)
    return tidx, dist


def counts(tidx):
    return (np.asarray(tidx) >= 0).sum(axis=1).astype(np.int64)


def compact(tidx, dist, cap=None):
    """The device form's outputs from the dense arrays: (rows int32 [n_images, cap, 3] = (query, row inside the image,
    float32 distance bits) ascending in query index, filled with -7 behind the rows that are there; counts int64
    [n_images] = min(count, cap); full int64 [n_images])."""
    tidx, dist = np.asarray(tidx, np.int32), np.asarray(dist, np.float32)
    ni, nq = tidx.shape
    cap = nq if cap is None else cap
    rows = np.full((ni, cap, 3), -7, np.int32)
    full = counts(tidx)
    for i in range(ni):
        q = np.nonzero(tidx[i] >= 0)[0][:cap]
        rows[i, :len(q), 0] = q
        rows[i, :len(q), 1] = tidx[i, q]
        rows[i, :len(q), 2] = dist[i, q].view(np.int32)
    return rows, np.minimum(full, cap), full
