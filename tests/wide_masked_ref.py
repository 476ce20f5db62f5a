"""Reference, data and mask generators for knnMatch under a mask on wide float banks (fm_wide_knn_masked); not a test.

* ``knn``: ``masked_ref.knn_f32`` -- the oracle's order-1 chain (``oracle.bf_knn(order=1)``, which takes any dim) per query row
  over that row's permitted train rows, indices mapped back; -1 / +inf where fewer than k rows are permitted.
* data: ``wide_ref.REGIMES`` (``data``), the planted pair (``planted``) and the duplicate cluster that overflows the filter's
  record list (``overflow_cluster``).
* ``MASKS``: the mask generators of the GPU tests, each ``f(nq, nt, k, seed) -> uint8 [nq, nt]``.
Nothing here calls the code under test."""
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)
import masked_ref       # noqa: E402
import wide_ref         # noqa: E402

DIMS = [129, 160, 161, 200, 256]                # K steps of 32: 5, 5, 6, 7, 8
SHAPES = [(0, 5), (5, 0), (1, 1), (127, 129), (129, 127), (300, 257)]
LARGE = (1000, 4099)                            # at dims 129 and 256 only; split and 64-row word boundaries inside the bank
REGIMES = ["clustered", "spread", "copies", "nonfinite"]


def knn(Q, T, mask, k):
    return masked_ref.knn_f32(Q, T, mask, k)


def data(regime, nq, nt, dim, seed=7):
    if nq == 0 or nt == 0 or (nt == 1 and regime in ("clustered", "copies")):
        return wide_ref.gaussian(nq, nt, dim, seed)
    return wide_ref.REGIMES[regime](nq, nt, dim, seed)


# ---- masks -------------------------------------------------------------------------------------------------------------------
def ones(nq, nt, k, seed):
    return np.ones((nq, nt), np.uint8)


def zeros(nq, nt, k, seed):
    return np.zeros((nq, nt), np.uint8)


def half(nq, nt, k, seed):
    return (np.random.default_rng(seed).random((nq, nt)) < 0.5).astype(np.uint8)


def sparse(nq, nt, k, seed):
    """Density 0.01: many rows have fewer than k permitted train rows."""
    return (np.random.default_rng(seed).random((nq, nt)) < 0.01).astype(np.uint8)


def band(nq, nt, k, seed):
    """64 train rows round i * nt / nq (clipped to the bank): whole 16-row tiles without a permitted pair."""
    m = np.zeros((nq, nt), np.uint8)
    for i in range(nq):
        c = i * nt // nq
        m[i, max(0, c - 32):min(nt, c + 32)] = 1
    return m


def exactly_one(nq, nt, k, seed):
    m = np.zeros((nq, nt), np.uint8)
    if nt:
        m[np.arange(nq), np.random.default_rng(seed).integers(0, nt, nq)] = 1
    return m


def k_minus_one(nq, nt, k, seed):
    """Exactly k - 1 permitted train rows per query row (none for k = 1)."""
    m = np.zeros((nq, nt), np.uint8)
    rng = np.random.default_rng(seed)
    for i in range(nq):
        m[i, rng.permutation(nt)[:min(k - 1, nt)]] = 1
    return m


def last_word(nq, nt, k, seed):
    """Bits only in the last, partial 64-bit word of a mask row (the train rows from 64 * ((nt - 1) // 64) on)."""
    m = np.zeros((nq, nt), np.uint8)
    if nt:
        lo = (nt - 1) // 64 * 64
        m[:, lo:] = np.random.default_rng(seed).random((nq, nt - lo)) < 0.5
    return m


MASKS = {"ones": ones, "zeros": zeros, "half": half, "sparse": sparse, "band": band, "exactly_one": exactly_one,
         "k_minus_one": k_minus_one, "last_word": last_word}


# ---- special cases -----------------------------------------------------------------------------------------------------------
def planted(nq, nt, dim, seed):
    """(Q, T, mask, rows): every query row has an exact copy of itself at train row rows[i], and that copy -- the one train row
    at distance 0 -- is forbidden; everything else is permitted."""
    Q, T = wide_ref.clustered(nq, nt, dim, seed)
    T = T.copy()
    rows = np.random.default_rng(seed + 1).permutation(nt)[:nq]
    T[rows] = Q
    mask = np.ones((nq, nt), np.uint8)
    mask[np.arange(nq), rows] = 0
    return Q, T, mask, rows


def overflow_cluster(seed=11):
    """(Q, T, mask): 2100 copies of one row among 2304 train rows, 600 query rows next to it, dim 129; the mask forbids every
    10th copy.  600 x 1890 = 1.13 million permitted pairs lie inside the filter's margin, against 2^20 list records."""
    rng = np.random.default_rng(seed)
    T = rng.standard_normal((2304, 129)).astype(np.float32)
    copies = np.sort(rng.permutation(2304)[:2100])
    T[copies] = T[copies[0]]
    Q = (T[copies[:600]] + 1e-3 * rng.standard_normal((600, 129))).astype(np.float32)
    mask = np.ones((600, 2304), np.uint8)
    mask[:, copies[::10]] = 0
    return Q, T, mask
