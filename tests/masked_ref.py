"""NumPy reference for knnMatch under a mask (fm_knn_masked); not a test.

* ``pack`` / ``unpack``: a uint8 / bool [nq, nt] mask <-> the library's bit layout, uint64 [nq, pad128(nt) / 64] words, bit b
  of word w of row i = (query row i, train row 64 w + b); bits at or beyond nt are 0.
* ``knn_u8``: brute force on the integer route -- exact int64 d2, ``np.sqrt`` in float32, order (float32 bits, index).
* ``knn_bin``: the same for binary rows (popcount of the XOR; the distance is the count as float32).
* ``knn_f32``: ``oracle.bf_knn(order=1)`` (the device's fma chain) applied per query row to that row's permitted train rows,
  with the indices mapped back.
* ``knn``: the three by kind ("u8", "f32", "bin").
Every function returns ``(idx int32 [nq, k], dist float32 [nq, k])`` with -1 / +inf where fewer than k rows are permitted.
Nothing here calls the code under test."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import oracle  # noqa: E402


def pad128(n):
    return (n + 127) // 128 * 128


def pack(mask):
    m = np.asarray(mask) != 0
    nq, nt = m.shape
    words = pad128(nt) // 64
    full = np.zeros((nq, words * 64), dtype=np.uint8)
    full[:, :nt] = m
    b = np.packbits(full.reshape(nq, words, 8, 8), axis=3, bitorder="little").reshape(nq, words, 8)
    return np.ascontiguousarray(b).view("<u8").reshape(nq, words)


def unpack(words, nt):
    w = np.ascontiguousarray(words, dtype="<u8")
    nq = w.shape[0]
    bits = np.unpackbits(w.view(np.uint8).reshape(nq, -1), axis=1, bitorder="little")
    return bits[:, :nt].astype(np.uint8)


def _lists(d32, mask, k):
    """Per row the k smallest (float32 bits, index) among the permitted columns of the float32 matrix d32 (>= 0)."""
    nq, nt = d32.shape
    idx = np.full((nq, k), -1, np.int32)
    dist = np.full((nq, k), np.inf, np.float32)
    bits = d32.view(np.uint32).astype(np.int64)
    for i in range(nq):
        cols = np.nonzero(mask[i])[0]
        if cols.size == 0:
            continue
        key = (bits[i, cols] << 32) | cols
        top = cols[np.argsort(key, kind="stable")[:k]]
        idx[i, :top.size] = top
        dist[i, :top.size] = d32[i, top]
    return idx, dist


def knn_u8(Q, T, mask, k):
    q, t = np.asarray(Q, dtype=np.int64), np.asarray(T, dtype=np.int64)
    d2 = (q * q).sum(1)[:, None] + (t * t).sum(1)[None, :] - 2 * (q @ t.T)
    return _lists(np.sqrt(d2.astype(np.float32)), np.asarray(mask) != 0, k)


def knn_bin(Q, T, mask, k):
    q, t = np.asarray(Q, dtype=np.uint8), np.asarray(T, dtype=np.uint8)
    h = np.zeros((q.shape[0], t.shape[0]), np.int64)
    pop = np.array([bin(v).count("1") for v in range(256)], dtype=np.int64)
    for c in range(q.shape[1]):
        h += pop[q[:, c][:, None] ^ t[:, c][None, :]]
    return _lists(h.astype(np.float32), np.asarray(mask) != 0, k)


def knn_f32(Q, T, mask, k):
    Q, T = np.ascontiguousarray(Q, dtype=np.float32), np.ascontiguousarray(T, dtype=np.float32)
    m = np.asarray(mask) != 0
    nq = Q.shape[0]
    idx = np.full((nq, k), -1, np.int32)
    dist = np.full((nq, k), np.inf, np.float32)
    for i in range(nq):
        cols = np.nonzero(m[i])[0]
        if cols.size == 0:
            continue
        ii, dd = oracle.bf_knn(Q[i:i + 1], T[cols], k, order=1, threads=1)
        idx[i] = np.where(ii[0] >= 0, cols[np.maximum(ii[0], 0)], -1)
        dist[i] = dd[0]
    return idx, dist


def knn(kind, Q, T, mask, k):
    return {"u8": knn_u8, "f32": knn_f32, "bin": knn_bin}[kind](Q, T, mask, k)
