"""NumPy reference of Fast-Match's self-distance test on binary descriptors (Hamming).

* self_dist(B): float64 [n], row i's distance to its nearest OTHER row -- min over j != i of popcount(B[i] XOR B[j]), by a
  byte-wise XOR and a 256-entry popcount table; +inf for a bank of one row, 0 for a row that has a duplicate.
* match_ratio(Q, T, sd, tau): the cross-checked 1-NN of tests/hamming_ref.py (xcheck, imported unchanged), then
  ratio = (double)dist / sd[q] in float64 and accepted iff ratio < tau: d / 0 = +inf and 0 / 0 = NaN are rejected, d / inf = 0
  is accepted for every tau > 0.  Returns (tidx, dist, ratio, passed) per query row; an unmatched row is -1 / +inf / NaN and
  not passed.
* match_accepted(Q, T, sd, tau): the accepted rows (qidx, tidx, dist, ratio), ascending query index."""
import numpy as np

from hamming_ref import xcheck

POPCOUNT = np.array([bin(v).count("1") for v in range(256)], np.uint8)


def self_dist(B):
    B = np.ascontiguousarray(B, dtype=np.uint8)
    n = len(B)
    out = np.full(n, np.inf, np.float64)
    if n < 2:
        return out
    blk = max(1, (1 << 24) // (n * B.shape[1]))
    for s in range(0, n, blk):
        h = POPCOUNT[B[s:s + blk, None, :] ^ B[None, :, :]].sum(axis=2, dtype=np.int64)
        h[np.arange(h.shape[0]), np.arange(s, s + h.shape[0])] = np.iinfo(np.int64).max      # j != i
        out[s:s + blk] = h.min(axis=1).astype(np.float64)
    return out


def match_ratio(Q, T, sd, tau):
    tidx, dist = xcheck(Q, T)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = dist.astype(np.float64) / np.asarray(sd, np.float64)
    ratio[tidx < 0] = np.nan                      # (an unmatched row has no ratio: fm_match_ratio's NaN)
    passed = (tidx >= 0) & (ratio < tau)          # (NaN < tau is False)
    return tidx, dist, ratio, passed


def same_f64(a, b):
    """Bit-for-bit equality of two float64 arrays; NaNs compare by position (0 / 0 has no fixed sign or payload)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64))


def match_accepted(Q, T, sd, tau):
    tidx, dist, ratio, passed = match_ratio(Q, T, sd, tau)
    q = np.nonzero(passed)[0].astype(np.int32)
    return q, tidx[q], dist[q], ratio[q]
