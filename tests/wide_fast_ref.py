"""NumPy reference of Fast-Match's self-distance test on wide float descriptors (FM_BANK_F32W, 129 .. 256 values per row),
composed from tests/wide_ref.py -- the oracle's order-1 chain -- with float64 ratios.  Shares no code with the product.

* self_dist(X): float64 [n], row i's distance to its nearest OTHER row: wide_ref.knn(X, X, 2), per row the entry whose index
  is the row itself dropped if it is there, the first remaining distance; +inf if none remains (a bank of one row, a row
  that holds a NaN or an infinite value: such a row has no finite distance, and is nobody's neighbour).
* match_ratio(Q, T, sd, tau): wide_ref.xcheck1, then ratio = (double)dist / sd[q] in float64 and accepted iff ratio < tau:
  d / 0 = +inf and 0 / 0 = NaN are rejected, d / inf = 0 is accepted for every tau > 0.  (tidx, dist, ratio, passed) per
  query row; an unmatched row is -1 / +inf / NaN and not passed.
* fast_match(Q, T, tau, sd=None): the accepted rows (qidx, tidx, dist, ratio), ascending query index; sd defaults to
  self_dist(Q).
* fast_match_each(Q, images, tau): a loop of that over the images."""
import numpy as np

import wide_ref


def self_dist(X):
    X = np.ascontiguousarray(X, np.float32)
    n = len(X)
    out = np.full(n, np.inf, np.float64)
    if n < 2:
        return out
    idx, dist = wide_ref.knn(X, X, 2)
    for i in range(n):
        for k in range(2):
            if idx[i, k] >= 0 and idx[i, k] != i:
                out[i] = np.float64(dist[i, k])
                break
    return out


def match_ratio(Q, T, sd, tau):
    tidx, dist = wide_ref.xcheck1(Q, T)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = dist.astype(np.float64) / np.asarray(sd, np.float64)
    ratio[tidx < 0] = np.nan                      # (an unmatched row has no ratio: fm_match_ratio's NaN)
    with np.errstate(invalid="ignore"):
        passed = (tidx >= 0) & (ratio < tau)      # (NaN < tau is False)
    return tidx, dist, ratio, passed


def fast_match(Q, T, tau, sd=None):
    sd = self_dist(Q) if sd is None else sd
    tidx, dist, ratio, passed = match_ratio(Q, T, sd, tau)
    q = np.nonzero(passed)[0].astype(np.int32)
    return q, tidx[q], dist[q], ratio[q]


def fast_match_each(Q, images, tau, sd=None):
    sd = self_dist(Q) if sd is None else sd
    return [fast_match(Q, T, tau, sd) for T in images]


def same_f64(a, b):
    """Bit-for-bit equality of two float64 arrays; NaNs compare by position (0 / 0 has no fixed sign or payload)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64))
