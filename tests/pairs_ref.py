"""NumPy reference of fm_collection_pairs_mutual_ratio, straight from the contract in include/fastmatch_hip.h: pair (a, b) is
mutual_ratio_ref.mutual_ratio(image a, image b), and the packed output follows fm_radius_match's rules with "pair" for
"query row".  Shares no code with the product."""
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)
import mutual_ratio_ref     # noqa: E402


def all_pairs(n_images):
    """pairs == NULL: every (i, j) with i < j, lexicographic."""
    return [(i, j) for i in range(n_images) for j in range(i + 1, n_images)]


def pairs_mutual_ratio(images, pairs, tau, symmetric=False, binary=False):
    """One (qidx, tidx, dist, ratio) per pair, in the order of ``pairs`` (None: all_pairs)."""
    if pairs is None:
        pairs = all_pairs(len(images))
    return [mutual_ratio_ref.mutual_ratio(images[a], images[b], tau, symmetric, binary) for a, b in pairs]


def pack(per_pair, cap):
    """(offsets int64 [n_pairs + 1] with the FULL counts, rows written, (qidx, tidx, dist, ratio) of the longest prefix of
    whole pairs that fits in cap)."""
    offsets = np.zeros(len(per_pair) + 1, np.int64)
    for p, r in enumerate(per_pair):
        offsets[p + 1] = offsets[p] + r[0].shape[0]
    whole = 0
    while whole < len(per_pair) and offsets[whole + 1] <= cap:
        whole += 1
    kept = per_pair[:whole]
    cols = []
    for c, dt in enumerate((np.int32, np.int32, np.float32, np.float64)):
        cols.append(np.concatenate([r[c] for r in kept]).astype(dt) if kept else np.zeros(0, dt))
    return offsets, int(offsets[whole]), tuple(cols)
