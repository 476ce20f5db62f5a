"""NumPy reference of fm_collection_pairs_mutual_ratio on a WIDE collection (images of 129 .. 256 float values per row), straight
from the contract in include/fastmatch_hip.h: pair (a, b) is wide_ref.mutual_ratio(image a, image b) -- the oracle's order-1
chain at any dim -- and the packed output is pairs_ref.pack's.  Shares no code with the product."""
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)
import pairs_ref            # noqa: E402
import wide_ref             # noqa: E402

all_pairs = pairs_ref.all_pairs
pack = pairs_ref.pack


def pairs_mutual_ratio(images, pairs, tau, symmetric=False, memo=None):
    """One (qidx, tidx, dist, ratio) per pair, in the order of ``pairs`` (None: all_pairs).  ``memo``: a dict the caller keeps
    for ONE list of images, so a pair that several tests ask for is computed once."""
    if pairs is None:
        pairs = all_pairs(len(images))
    out = []
    for a, b in pairs:
        key = (int(a), int(b), float(tau), bool(symmetric))
        if memo is None or key not in memo:
            r = wide_ref.mutual_ratio(images[a], images[b], tau, symmetric)
            if memo is None:
                out.append(r)
                continue
            memo[key] = r
        out.append(memo[key])
    return out


def unit(a):
    return (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)


def images(sizes, dim, seed, big=None):
    """wide_ref.clustered's recipe per image: unit-norm rows on a shared 16-D subspace plus noise.  ``big``: the index of the
    image whose rows the others see again -- every third row of each other image of two rows or more is a noisy view
    (sigma = 0.02 / sqrt(dim)) of one of its rows."""
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((16, dim))
    out = []
    for n in sizes:
        if n == 0:
            out.append(np.zeros((0, dim), np.float32))
        else:
            out.append(unit(rng.standard_normal((n, 16)) @ B + 0.05 * rng.standard_normal((n, dim))))
    if big is not None:
        src = out[big]
        for i, im in enumerate(out):
            if i == big or im.shape[0] < 2:
                continue
            rows = np.arange(0, im.shape[0], 3)
            im[rows] = unit(src[(rows * 7) % src.shape[0]].astype(np.float64) + 0.02 / np.sqrt(dim) * rng.standard_normal((len(rows), dim)))
    return out
