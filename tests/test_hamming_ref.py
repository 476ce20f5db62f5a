"""CPU: the NumPy Hamming reference (tests/hamming_ref.py) against a plain Python double loop and hand-made cases, and the
matchutil checks of normType that need no device."""
import numpy as np
import pytest

import hamming_ref as H
from fastmatch_amd import matchutil


def _h(a, b):
    return sum(bin(int(x) ^ int(y)).count("1") for x, y in zip(a, b))


def _loop_knn(Q, T, k):
    out = []
    for q in Q:
        lst = []                                               # OpenCV: strict insertion in ascending train order
        for j, t in enumerate(T):
            d = _h(q, t)
            pos = len(lst)
            while pos > 0 and d < lst[pos - 1][0]:
                pos -= 1
            lst.insert(pos, (d, j))
            del lst[k:]
        out.append(lst + [(np.inf, -1)] * (k - len(lst)))
    return out


def _loop_xcheck(Q, T):
    elect = {}
    for j, t in enumerate(T):
        best = None
        for i, q in enumerate(Q):
            d = _h(q, t)
            if best is None or d < best[0]:
                best = (d, i)
        if best is not None:
            d, i = best
            if i not in elect or d < elect[i][0]:
                elect[i] = (d, j)
    return [elect.get(i, (np.inf, -1)) for i in range(len(Q))]


@pytest.mark.parametrize("width", [1, 8, 16, 31, 32, 61, 64])
@pytest.mark.parametrize("nq,nt", [(0, 3), (3, 0), (1, 1), (2, 5), (7, 3), (17, 15)])
@pytest.mark.parametrize("pool", [0, 4])
def test_reference_equals_the_double_loop(width, nq, nt, pool):
    rng = np.random.default_rng(width * 1000 + nq * 10 + nt)
    if pool:                                                   # few distinct rows: mass ties
        P = rng.integers(0, 256, (pool, width), dtype=np.uint8)
        Q, T = P[rng.integers(0, pool, nq)], P[rng.integers(0, pool, nt)]
    else:
        Q = rng.integers(0, 256, (nq, width), dtype=np.uint8)
        T = rng.integers(0, 256, (nt, width), dtype=np.uint8)
    for k in (1, 2, 5):
        idx, dist = H.knn(Q, T, k)
        ref = _loop_knn(Q, T, k)
        assert idx.tolist() == [[j for _, j in r] for r in ref]
        assert dist.tolist() == [[float(d) for d, _ in r] for r in ref]
    tidx, tdist = H.xcheck(Q, T)
    ref = _loop_xcheck(Q, T)
    assert tidx.tolist() == [j for _, j in ref]
    assert tdist.tolist() == [float(d) for d, _ in ref]


def test_equal_distances_go_to_the_earlier_train_row():
    Q = np.array([[0x00]], np.uint8)
    T = np.array([[0x01], [0x02], [0x04], [0x00], [0x08]], np.uint8)
    idx, dist = H.knn(Q, T, 5)
    assert idx.tolist() == [[3, 0, 1, 2, 4]] and dist.tolist() == [[0, 1, 1, 1, 1]]
    idx, dist = H.knn(np.array([[0x80]], np.uint8), T[:3], 2)
    assert idx.tolist() == [[0, 1]] and dist.tolist() == [[2, 2]]


def test_crosscheck_a_query_elected_by_a_row_it_does_not_prefer():
    # q1's own nearest train row is t0 (h = 1, the earlier of two at 1), but t0 elects q0 (h = 0): q1 gets t1
    Q = np.array([[0x00], [0x01]], np.uint8)
    T = np.array([[0x00], [0x03]], np.uint8)
    assert H.knn(Q, T, 1)[0].tolist() == [[0], [0]]
    tidx, dist = H.xcheck(Q, T)
    assert tidx.tolist() == [0, 1] and dist.tolist() == [0, 1]


def test_crosscheck_a_query_nobody_elects():
    tidx, dist = H.xcheck(np.array([[0x00], [0xFF], [0x0F]], np.uint8), np.array([[0x01], [0x03]], np.uint8))
    assert tidx.tolist() == [0, -1, -1] and dist.tolist()[1:] == [np.inf, np.inf]
    assert dist[0] == 1.0             # both train rows elect q0 (t1 ties q0 and q2 at 2: the lower query index); t0 at 1 wins


def test_ratio_match_rejects_a_zero_second_distance():
    Q = np.array([[0x00], [0x0F], [0xF0]], np.uint8)
    T = np.array([[0x0F], [0x0F], [0x00], [0x01]], np.uint8)
    q, t, d, r = H.ratio_match(Q, T, 0.8)
    # q0: d0 = 0 (t2), d1 = 1 (t3) -> 0 < 0.8 accepted; q1: d0 = d1 = 0 (duplicates) -> 0 / 0 rejected; q2: 4 / 4 rejected
    assert q.tolist() == [0] and t.tolist() == [2] and d.tolist() == [0.0] and r.tolist() == [0.0]


def test_matchutil_refuses_norms_and_dtypes_it_does_not_build():
    a = np.zeros((4, 32), np.uint8)
    for bad in (7, 1, 2, 5, "L2"):
        with pytest.raises(ValueError):
            matchutil.bf_match(a, a, k=1, options={"normType": bad})
    with pytest.raises(ValueError, match="NORM_HAMMING2"):
        matchutil.bf_match(a, a, k=1, options={"normType": 7})
    with pytest.raises(ValueError, match="uint8"):
        matchutil.bf_match(a.astype(np.float32), a, k=2, options={"normType": matchutil.NORM_HAMMING})
    with pytest.raises(ValueError, match="uint8"):
        matchutil.ratio_match_arrays(a, a.astype(np.int16), 0.8, options={"normType": matchutil.NORM_HAMMING})
    with pytest.raises(ValueError, match="radiusMatch"):
        matchutil.bf_radius_match(a, a, 10.0, options={"normType": matchutil.NORM_HAMMING})
    assert (matchutil.NORM_L2, matchutil.NORM_HAMMING) == (4, 6)
