"""NumPy reference of fm_collection_wide_mutual_ratio_each / fm_collection_wide_knn2_each (a wide query bank against every image
of a wide collection), straight from the contract in include/fastmatch_hip.h: image i is wide_ref.mutual_ratio(Q, image_i) --
the oracle's order-1 chain at any dim -- the knn2 form is wide_ref.knn(Q, image_i, 2), and the packed output is
pairs_ref.pack's with "image" for "pair".  Shares no code with the product."""
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)
import pairs_ref            # noqa: E402
import wide_pairs_ref       # noqa: E402
import wide_ref             # noqa: E402

pack = pairs_ref.pack
unit = wide_pairs_ref.unit
SIZES = [0, 1, 127, 128, 129, 1000, 5, 0]


def mutual_ratio_each(Q, images, tau, symmetric=False):
    """One (qidx, tidx, dist, ratio) per image: the images are independent of each other."""
    return [wide_ref.mutual_ratio(Q, im, tau, symmetric) for im in images]


def knn2_each(Q, images):
    """(idx int32, dist float32) [n_images, nq, 2]; -1 / +inf where an image has fewer than two rows."""
    idx = np.full((len(images), len(Q), 2), -1, np.int32)
    dist = np.full((len(images), len(Q), 2), np.inf, np.float32)
    for i, im in enumerate(images):
        idx[i], dist[i] = wide_ref.knn(Q, im, 2)
    return idx, dist


def query(images, dim, seed, nq=300, big=5):
    """nq rows of wide_pairs_ref.images' recipe; every second row is a noisy view (sigma = 0.02 / sqrt(dim), renormalised) of
    row (3 r) % rows of image ``big``; row 7 is a copy of row 6 (the lowest query index must win the reverse tie)."""
    Q = wide_pairs_ref.images([nq], dim, seed)[0]
    rng = np.random.default_rng(seed + 1)
    rows = np.arange(0, nq, 2)
    src = images[big]
    Q[rows] = unit(src[(3 * rows) % src.shape[0]].astype(np.float64) + 0.02 / np.sqrt(dim) * rng.standard_normal((len(rows), dim)))
    if nq > 7:
        Q[7] = Q[6]
    return Q


def data(dim):
    """(images, query) of the GPU test at one width."""
    images = wide_pairs_ref.images(SIZES, dim, 9100 + dim, big=5)
    return images, query(images, dim, 9200 + dim)
