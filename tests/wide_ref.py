"""Data generators and the reference for wide float banks (FM_BANK_F32W, 129 .. 256 values per row).  The distances are the
oracle's order-1 chain -- oracle.bf_knn(order=1) / oracle.bf_xcheck1(order=1), which take any dim; the ratio match and the
mutual ratio match are composed from them in NumPy with float64 ratios, following include/fastmatch_hip.h's rules word for
word.  Shares no code with the product."""
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (_HERE, os.path.dirname(_HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import oracle           # noqa: E402

DIMS = [129, 159, 160, 161, 192, 255, 256]      # one value past a K step of 32, an exact step, the last partial step
SHAPES = [(0, 5), (5, 0), (1, 1), (2, 2), (1, 300), (127, 129), (129, 127), (300, 257), (1000, 4099), (4099, 1000)]
LARGE = [(1000, 4099), (4099, 1000)]            # at dims 129 and 256 only


# ---- reference ---------------------------------------------------------------------------------------------------------------
def knn(Q, T, k):
    """(idx int32 [nq, k], dist float32 [nq, k]); -1 / +inf where T has fewer than k rows."""
    Q = np.ascontiguousarray(Q, np.float32)
    T = np.ascontiguousarray(T, np.float32)
    if len(Q) == 0 or len(T) == 0:
        return np.full((len(Q), k), -1, np.int32), np.full((len(Q), k), np.inf, np.float32)
    return oracle.bf_knn(Q, T, k, order=1)


def xcheck1(Q, T):
    Q = np.ascontiguousarray(Q, np.float32)
    T = np.ascontiguousarray(T, np.float32)
    if len(Q) == 0 or len(T) == 0:
        return np.full(len(Q), -1, np.int32), np.full(len(Q), np.inf, np.float32)
    return oracle.bf_xcheck1(Q, T, order=1)


def ratios(idx, dist):
    """float64 d0 / d1 per row, NaN where the second neighbour is missing (0 / 0 is NaN by itself)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        r = dist[:, 0].astype(np.float64) / dist[:, 1].astype(np.float64)
    return np.where(idx[:, 1] >= 0, r, np.nan)


def ratio_match(Q, T, tau):
    """fm_knn2_ratio: (qidx, tidx, dist, ratio) of the rows with d0 / d1 < tau, ascending query index."""
    idx, dist = knn(Q, T, 2)
    r = ratios(idx, dist)
    with np.errstate(invalid="ignore"):
        q = np.nonzero(r < tau)[0]
    return q.astype(np.int32), idx[q, 0].astype(np.int32), dist[q, 0].astype(np.float32), r[q]


def mutual_ratio(Q, T, tau, symmetric=False):
    """fm_mutual_ratio: a query row is kept iff its forward ratio passes, it is the nearest query row of its first neighbour
    and -- symmetric -- that train row's own ratio over the query rows passes too; the ratio is then the larger one."""
    nq = len(Q)
    k_idx, k_dist = knn(Q, T, 2)
    r_idx, r_dist = knn(T, Q, 2)
    fwd, rev_t = ratios(k_idx, k_dist), ratios(r_idx, r_dist)
    t0 = k_idx[:, 0]
    has = t0 >= 0
    safe = np.where(has, t0, 0)
    with np.errstate(invalid="ignore"):
        keep = fwd < tau
    if len(T):
        keep = keep & has & (r_idx[safe, 0] == np.arange(nq))
        rev = np.where(has, rev_t[safe], np.nan)
    else:
        keep = np.zeros(nq, bool)
        rev = np.full(nq, np.nan)
    ratio = fwd
    if symmetric:
        with np.errstate(invalid="ignore"):
            keep = keep & (rev < tau)
        ratio = np.maximum(fwd, rev)
    q = np.nonzero(keep)[0]
    return q.astype(np.int32), t0[q].astype(np.int32), k_dist[q, 0].astype(np.float32), ratio[q].astype(np.float64)


# ---- data --------------------------------------------------------------------------------------------------------------------
def _unit(a):
    return (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)


def clustered(nq, nt, dim, seed):
    """Unit-norm rows on a 16-D subspace plus noise; every query row a near copy of a train row."""
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((16, dim))
    T = _unit(rng.standard_normal((nt, 16)) @ B + 0.05 * rng.standard_normal((nt, dim)))
    Q = _unit(T[rng.integers(0, nt, nq)].astype(np.float64) + 0.02 / np.sqrt(dim) * rng.standard_normal((nq, dim)))
    return Q, T


def gaussian(nq, nt, dim, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((nq, dim)).astype(np.float32), rng.standard_normal((nt, dim)).astype(np.float32)


def spread(nq, nt, dim, seed):
    """Row magnitudes spread over 1e-3 .. 1e3."""
    rng = np.random.default_rng(seed)
    Q, T = gaussian(nq, nt, dim, seed + 1)
    return ((Q.T * 10.0 ** rng.uniform(-3, 3, nq)).T.astype(np.float32), (T.T * 10.0 ** rng.uniform(-3, 3, nt)).T.astype(np.float32))


def integers(nq, nt, dim, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (nq, dim)).astype(np.float32), rng.integers(0, 256, (nt, dim)).astype(np.float32)


def copies(nq, nt, dim, seed):
    """600 exact copies of one train row (fewer when the bank is smaller), the first half of the query rows next to it."""
    Q, T = clustered(nq, nt, dim, seed)
    rng = np.random.default_rng(seed + 1)
    rows = rng.permutation(nt)[:min(600, nt - 1)]
    T[rows] = T[rows[0]]
    Q[:nq // 2] = T[rows[0]] + (1e-3 * rng.standard_normal((nq // 2, dim))).astype(np.float32)
    return Q, T


def dup_queries(nq, nt, dim, seed):
    Q, T = clustered(nq, nt, dim, seed)
    Q[1::3] = Q[0::3][:len(Q[1::3])]
    return Q, T


def nonfinite(nq, nt, dim, seed):
    """One +inf value and one NaN row on each side."""
    Q, T = gaussian(nq, nt, dim, seed)
    Q[nq // 3, dim // 2] = np.inf
    Q[nq // 2] = np.nan
    T[nt // 3, dim - 1] = np.inf
    T[nt // 2] = np.nan
    return Q, T


REGIMES = {"clustered": clustered, "gaussian": gaussian, "spread": spread, "integers": integers, "copies": copies,
           "dup_queries": dup_queries, "nonfinite": nonfinite}
FILTERED = {"clustered", "gaussian", "spread", "integers", "copies", "dup_queries"}     # every value finite: the filter runs


def margin_census(Q, T):
    """Per query row, the number of train rows with d2 <= d2 of the second neighbour + 4 M, in float64, with M = 1.1 * 2^-10 *
    (|q|^2 + max |t|^2) (K8's margin; scale free, so taken on the unscaled rows)."""
    Q = Q.astype(np.float64)
    T = T.astype(np.float64)
    tn = (T * T).sum(1)
    out = np.empty(len(Q), np.int64)
    for i in range(0, len(Q), 512):
        q = Q[i:i + 512]
        qn = (q * q).sum(1)
        d2 = np.maximum(qn[:, None] + tn[None, :] - 2.0 * (q @ T.T), 0.0)
        second = np.partition(d2, 1, axis=1)[:, 1]
        M = 1.1 * 2.0 ** -10 * (qn + tn.max())
        out[i:i + 512] = (d2 <= (second + 4.0 * M)[:, None]).sum(1)
    return out
