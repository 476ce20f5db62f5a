"""NumPy reference of cv2.BFMatcher(NORM_HAMMING2): cv::normHamming(a, b, n, cellSize = 2) -- h2(q, t) = the number of 2-bit
cells (bits 2c, 2c + 1 of a byte) of q XOR t that are non-zero, from OpenCV's 256-entry cell-count table.

* distances(Q, T): h2 as int32 [nq, nt], by the table.
* knn / xcheck / ratio_match: the shapes and rules of hamming_ref with h2 for h -- (h2, train index) ascending, the earlier
  row wins a tie, -1 / +inf where T has fewer than k rows; d0 / d1 < tau in float64, d1 == 0 rejected.
* mutual_ratio(Q, T, tau, symmetric): fm_mutual_ratio's rule -- the ratio test on the forward 2-NN list, the first neighbour's
  nearest query row (lowest index on ties) is the row itself, and (symmetric) the reverse ratio passes too; the ratio reported
  is then the larger of the two.
* Ref / radius_match: the shapes of hamming_radius_ref.Ref: float32(h2) < r_i, strict, lists ascending (h2, train index).
* encode(rows): the +-1 tetrahedral image the matrix cores multiply, [n, 12 * bytes] int8 (csrc/hamming2.hip): cell (a, b)
  -> (s_a, s_b, s_a s_b), s = +1 for a 1 bit, -1 for a 0 bit; encode(q) . encode(t) = 3 P - 4 h2 with P = 4 * bytes cells.
* fp4_steps(bytes): K steps of 128 FP4 values per row."""
import numpy as np

import hamming_ref

# OpenCV's popCountTable2: entry v = the number of non-zero 2-bit cells of the byte v
TABLE2 = np.array([sum(1 for c in range(4) if (v >> (2 * c)) & 3) for v in range(256)], np.int32)

_BLOCK = 1 << 22


def distances(Q, T):
    Q = np.ascontiguousarray(Q, dtype=np.uint8)
    T = np.ascontiguousarray(T, dtype=np.uint8)
    nq, nt, b = len(Q), len(T), Q.shape[1]
    out = np.empty((nq, nt), np.int32)
    blk = max(1, _BLOCK // max(1, nt * b))
    for s in range(0, nq, blk):
        out[s:s + blk] = TABLE2[Q[s:s + blk, None, :] ^ T[None, :, :]].sum(axis=2, dtype=np.int32)
    return out


def distances_by_mask(Q, T):
    """h2 by the vector-ALU kernel's rule: popcount((x | x >> 1) & 0x55) of x = q XOR t, byte by byte."""
    x = np.ascontiguousarray(Q, dtype=np.uint8)[:, None, :] ^ np.ascontiguousarray(T, dtype=np.uint8)[None, :, :]
    return np.bitwise_count((x | (x >> 1)) & 0x55).sum(axis=2, dtype=np.int32)


def encode(rows):
    rows = np.ascontiguousarray(rows, dtype=np.uint8)
    n, b = rows.shape
    cells = np.stack([(rows >> (2 * c)) & 3 for c in range(4)], axis=2).reshape(n, 4 * b)      # cell 4 * byte + c
    sa = np.where(cells & 1, 1, -1).astype(np.int8)
    sb = np.where(cells & 2, 1, -1).astype(np.int8)
    return np.stack([sa, sb, sa * sb], axis=2).reshape(n, 12 * b)


def fp4_steps(nbytes):
    return (12 * nbytes + 127) // 128


def knn(Q, T, k):
    nq, nt = len(Q), len(T)
    idx = np.full((nq, k), -1, np.int32)
    dist = np.full((nq, k), np.inf, np.float32)
    if nq == 0 or nt == 0:
        return idx, dist
    kk = min(k, nt)
    key = distances(Q, T).astype(np.int64) * nt + np.arange(nt, dtype=np.int64)       # (h2, index): unique, lexicographic
    pk = np.sort(key, axis=1)[:, :kk]
    idx[:, :kk] = (pk % nt).astype(np.int32)
    dist[:, :kk] = (pk // nt).astype(np.float32)
    return idx, dist


def xcheck(Q, T):
    nq, nt = len(Q), len(T)
    if nq == 0 or nt == 0:
        return np.full(nq, -1, np.int32), np.full(nq, np.inf, np.float32)
    ridx, rdist = knn(T, Q, 1)
    return hamming_ref.scatter_min(ridx[:, 0], rdist[:, 0], nq)


def _ratios(idx, dist):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(idx[:, 1] >= 0, dist[:, 0].astype(np.float64) / dist[:, 1].astype(np.float64), np.nan)


def ratio_match(Q, T, tau):
    """(qidx, tidx, dist = d0, ratio) of the accepted matches, ascending query index."""
    idx, dist = knn(Q, T, 2)
    r = _ratios(idx, dist)
    ok = r < tau
    return np.nonzero(ok)[0].astype(np.int32), idx[ok, 0], dist[ok, 0], r[ok]


def mutual_ratio(Q, T, tau, symmetric=False):
    """(qidx, tidx, dist, ratio) of fm_mutual_ratio, ascending query index."""
    nq = len(Q)
    idx, dist = knn(Q, T, 2)
    r = _ratios(idx, dist)
    keep = r < tau
    if nq and len(T):
        ridx, rdist = knn(T, Q, 2)
        rr = _ratios(ridx, rdist)
        for i in np.nonzero(keep)[0]:
            t = idx[i, 0]
            keep[i] = ridx[t, 0] == i
            if keep[i] and symmetric:
                keep[i] = rr[t] < tau
                if keep[i] and rr[t] > r[i]:
                    r[i] = rr[t]
    return np.nonzero(keep)[0].astype(np.int32), idx[keep, 0], dist[keep, 0], r[keep]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class Ref(object):
    """All distances of Q against T, computed once; cut per call (hamming_radius_ref.Ref's shape, for a bank pair)."""

    def __init__(self, Q, T):
        self.nq, self.total = len(Q), len(T)
        self.P = 4 * Q.shape[1]
        self.h = distances(Q, T).astype(np.float32) if self.nq and self.total else np.zeros((self.nq, self.total), np.float32)
        self.order = np.argsort(self.h, axis=1, kind="stable").astype(np.int32)
        self.sorted = np.take_along_axis(self.h, self.order, axis=1)

    def cut(self, r):
        """(offsets int64 [nq + 1], idx, dist) of the lists float32(h2) < r_i, flat."""
        rr = np.broadcast_to(np.asarray(r, dtype=np.float32), (self.nq,))
        with np.errstate(invalid="ignore"):
            m = self.sorted < rr[:, None]
        off = np.concatenate([[0], np.cumsum(m.sum(axis=1))]).astype(np.int64)
        return off, self.order[m], self.sorted[m]


def radius_match(Q, T, r):
    return Ref(Q, T).cut(r)


def same_lists(got, want, what=""):
    """Indices exactly, distances as bit patterns."""
    off, idx, dist = got
    woff, widx, wdist = want
    assert off.dtype == np.int64 and np.array_equal(off, woff), what + " offsets"
    assert idx.shape == dist.shape == (int(woff[-1]),), what + " sizes"
    assert np.array_equal(idx, widx), what + " idx"
    assert np.array_equal(bits(dist), bits(wdist)), what + " dist"
