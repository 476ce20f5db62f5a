"""NumPy reference of fm_mutual_ratio, straight from the contract in include/fastmatch_hip.h: the 2-NN lists in both
directions -- oracle.bf_knn (L2) or hamming_ref.knn (Hamming) -- then the three rules per query row.  Shares no code with
the product."""
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (_HERE, os.path.dirname(_HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import hamming_ref      # noqa: E402
import oracle           # noqa: E402


def knn2(A, B, binary=False):
    """(idx int32 [na, 2], dist float32 [na, 2]) of the rows of A over the rows of B; -1 / inf where B has fewer than 2 rows."""
    if binary:
        return hamming_ref.knn(A, B, 2)
    if len(A) == 0 or len(B) == 0:
        return np.full((len(A), 2), -1, np.int32), np.full((len(A), 2), np.inf, np.float32)
    return oracle.bf_knn(A, B, 2)


def ratios(idx, dist):
    """float64 d0 / d1 per row, NaN where the second neighbour is missing (0 / 0 is NaN by itself)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        r = dist[:, 0].astype(np.float64) / dist[:, 1].astype(np.float64)
    return np.where(idx[:, 1] >= 0, r, np.nan)


def classes(Q, T, tau, binary=False):
    """Per query row: (t0, d0, forward ratio, passes the ratio test, is mutual, reverse ratio of t0)."""
    nq = len(Q)
    k_idx, k_dist = knn2(Q, T, binary)
    r_idx, r_dist = knn2(T, Q, binary)
    fwd = ratios(k_idx, k_dist)
    rev_t = ratios(r_idx, r_dist)
    t0 = k_idx[:, 0]
    has = t0 >= 0
    safe = np.where(has, t0, 0)
    with np.errstate(invalid="ignore"):
        ok = fwd < tau
    mutual = has & (r_idx[safe, 0] == np.arange(nq)) if len(T) else np.zeros(nq, bool)
    rev = np.where(has, rev_t[safe], np.nan) if len(T) else np.full(nq, np.nan)
    return t0, k_dist[:, 0], fwd, ok, mutual, rev


def mutual_ratio(Q, T, tau, symmetric=False, binary=False):
    """(qidx int32, tidx int32, dist float32, ratio float64) of the accepted rows, ascending query index."""
    t0, d0, fwd, ok, mutual, rev = classes(Q, T, tau, binary)
    keep = ok & mutual
    ratio = fwd
    if symmetric:
        with np.errstate(invalid="ignore"):
            keep = keep & (rev < tau)
        ratio = np.maximum(fwd, rev)
    q = np.nonzero(keep)[0]
    return q.astype(np.int32), t0[q].astype(np.int32), d0[q].astype(np.float32), ratio[q].astype(np.float64)


def mutual_ratio_each(Q, images, tau, symmetric=False, binary=False):
    return [mutual_ratio(Q, im, tau, symmetric, binary) for im in images]


def structured(seed, binary=False):
    """The 300 x 257 construction: train rows = noisy copies of 150 of 200 base rows + random rows; query rows = two noisy
    views each of 60 base rows (50 of them in the train set: only the nearer view can be mutual, and two close views spoil the
    train row's reverse ratio), one view of 40 more, + random rows; shuffled."""
    rng = np.random.default_rng(seed)
    w = 32 if binary else 128

    def rand(n):
        if binary:
            return rng.integers(0, 256, (n, w), dtype=np.uint8)
        return rng.integers(0, 120, (n, w)).astype(np.uint8)

    def noisy(rows, amount):
        out = rows.copy()
        if binary:
            for r in out:
                for _ in range(int(amount)):
                    r[rng.integers(0, w)] ^= np.uint8(1 << rng.integers(0, 8))
            return out
        return np.clip(out.astype(np.int32) + rng.integers(-amount, amount + 1, out.shape), 0, 255).astype(np.uint8)

    base = rand(200)
    a = 12
    T = np.concatenate([noisy(base[:150], a), rand(107)])
    near = np.concatenate([noisy(base[100:130], a), noisy(base[130:160], 2 * a)])
    far = np.concatenate([noisy(base[100:130], 3 * a), noisy(base[130:160], 2.5 * a)])
    Q = np.concatenate([near, far, noisy(base[160:200], a), rand(140)])
    assert T.shape[0] == 257 and Q.shape[0] == 300
    return Q[rng.permutation(300)], T[rng.permutation(257)]
