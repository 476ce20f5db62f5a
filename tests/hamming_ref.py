"""NumPy reference of cv2.BFMatcher(NORM_HAMMING): cv::batchDistance with dtype CV_32S, h(q, t) = popcount(q XOR t).

* knn(Q, T, k): per query row the k smallest (h, train index), ascending -- a stable order, so the earlier train row
  wins a tie (OpenCV's strict insertion in ascending train order); -1 / +inf where T has fewer than k rows.
* xcheck(Q, T): every train row elects its nearest query row (strict <: the lowest query index on ties); each query
  keeps the closest electing train row (strict <, ascending train order: the lowest train index on ties); -1 / +inf
  for a query nobody elects.
* ratio_match(Q, T, tau): the classic ratio match of the 2-NN lists, d0 / d1 < tau in float64, d1 == 0 rejected.
Rows are XORed as uint64 words (zero padded) and counted with np.bitwise_count, blocked by query rows."""
import numpy as np

_BLOCK_ELEMS = 1 << 22          # uint64 words per XOR block


def words(a):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    n, b = a.shape
    wb = max(8, (b + 7) // 8 * 8)
    p = np.zeros((n, wb), np.uint8)
    p[:, :b] = a
    return p.view(np.uint64)


def distances(Q, T):
    """h[i, j] = popcount(Q[i] XOR T[j]) as int32 [nq, nt]."""
    qw, tw = words(Q), words(T)
    nq, nt, w = qw.shape[0], tw.shape[0], qw.shape[1]
    out = np.empty((nq, nt), np.int32)
    blk = max(1, _BLOCK_ELEMS // max(1, nt * w))
    for s in range(0, nq, blk):
        x = qw[s:s + blk, None, :] ^ tw[None, :, :]
        out[s:s + blk] = np.bitwise_count(x).sum(axis=2, dtype=np.int32)
    return out


def knn(Q, T, k):
    nq, nt = len(Q), len(T)
    idx = np.full((nq, k), -1, np.int32)
    dist = np.full((nq, k), np.inf, np.float32)
    if nq == 0 or nt == 0:
        return idx, dist
    kk = min(k, nt)
    qw = words(Q)
    blk = max(1, _BLOCK_ELEMS // max(1, nt * qw.shape[1]))
    cols = np.arange(nt, dtype=np.int64)
    for s in range(0, nq, blk):
        h = distances(Q[s:s + blk], T).astype(np.int64)
        key = h * nt + cols                                   # (h, index): unique, lexicographic
        if kk < nt:
            part = np.argpartition(key, kk - 1, axis=1)[:, :kk]
        else:
            part = np.broadcast_to(cols, key.shape).copy()
        pk = np.take_along_axis(key, part, axis=1)
        order = np.argsort(pk, axis=1, kind="stable")
        pk = np.take_along_axis(pk, order, axis=1)
        idx[s:s + blk, :kk] = (pk % nt).astype(np.int32)
        dist[s:s + blk, :kk] = (pk // nt).astype(np.float32)
    return idx, dist


def scatter_min(elect, h, nq):
    """Step 2 of crossCheck: elect[t] = the query row train row t elects, h[t] its distance -> (tidx, dist) per query."""
    nt = len(elect)
    best = np.full(nq, np.iinfo(np.int64).max, np.int64)
    if nt:
        np.minimum.at(best, elect.astype(np.int64), h.astype(np.int64) * nt + np.arange(nt, dtype=np.int64))
    hit = best != np.iinfo(np.int64).max
    tidx = np.where(hit, best % max(nt, 1), -1).astype(np.int32)
    dist = np.where(hit, (best // max(nt, 1)).astype(np.float32), np.float32(np.inf)).astype(np.float32)
    return tidx, dist


def xcheck(Q, T):
    nq, nt = len(Q), len(T)
    if nq == 0 or nt == 0:
        return np.full(nq, -1, np.int32), np.full(nq, np.inf, np.float32)
    ridx, rdist = knn(T, Q, 1)                                # per train row: nearest query, lowest index on ties
    return scatter_min(ridx[:, 0], rdist[:, 0], nq)


def ratio_match(Q, T, tau):
    """(qidx, tidx, dist = d0, ratio) of the accepted matches, ascending query index."""
    idx, dist = knn(Q, T, 2)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(idx[:, 1] >= 0, dist[:, 0].astype(np.float64) / dist[:, 1].astype(np.float64), np.nan)
    ok = r < tau
    q = np.nonzero(ok)[0].astype(np.int32)
    return q, idx[ok, 0], dist[ok, 0], r[ok]
