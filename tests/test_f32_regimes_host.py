"""No GPU: every value regime of tests/f32_regimes.py is the edge it claims to be, checked with the oracle alone (the
float32 fma chain, order 1).  A regime that misses its condition gets its constants changed, not its assertion relaxed."""
import numpy as np

import oracle
import f32_regimes as R


def _knn(Q, T, k):
    return oracle.bf_knn(Q, T, k, order=1)


def test_builders_are_deterministic_float32_of_the_stated_shapes():
    for name, (build, _) in R.REGIMES.items():
        Q, T = build()
        Q2, T2 = build()
        dim = 61 if name == "dim61" else R.DIM
        assert Q.dtype == T.dtype == np.float32 and Q.shape == (R.NQ, dim) and T.shape == (R.NT, dim), name
        assert np.array_equal(Q.view(np.uint32), Q2.view(np.uint32)) and np.array_equal(T.view(np.uint32), T2.view(np.uint32)), name


def test_overflow_every_distance_is_inf_and_every_index_minus_one():
    idx, dist = _knn(*R.overflow(), 8)
    assert (idx == -1).all() and np.isposinf(dist).all()


def test_underflow_1e30_every_distance_is_zero():
    Q, T = R.underflow(1e-30)
    assert np.count_nonzero(T) > T.size // 2            # (the rows themselves are not zero)
    idx, dist = _knn(Q, T, R.NT)
    assert (dist == 0).all()
    assert np.array_equal(idx, np.broadcast_to(np.arange(R.NT, dtype=np.int32), idx.shape))   # rows by index


def test_underflow_1e23_distances_are_quantised_into_ties():
    idx, dist = _knn(*R.underflow(1e-23), 8)
    assert np.isfinite(dist).all() and (idx >= 0).all()
    tied = dist[:, 1:] == dist[:, :-1]
    assert tied.mean() >= 0.10, tied.mean()
    assert len(np.unique(dist)) > 1                      # (but not all one value: that is the 1e-30 case)


def test_tiny_squares_are_subnormal_and_distances_distinct():
    Q, T = R.tiny()
    sq = np.abs(Q.astype(np.float64)) ** 2
    assert np.median(sq) < np.finfo(np.float32).tiny     # a typical v * v is a float32 subnormal
    idx, dist = _knn(Q, T, 8)
    assert np.isfinite(dist).all() and (dist > 0).all()
    assert (dist[:, 1:] == dist[:, :-1]).mean() < 0.01


def test_huge_every_top8_distance_is_finite():
    idx, dist = _knn(*R.huge(), 8)
    assert np.isfinite(dist).all() and (idx >= 0).all()


def test_huge_and_overflow_exceed_the_collection_limit_and_the_others_do_not():
    for name, (build, _) in R.REGIMES.items():
        Q, T = build()
        m = max(np.abs(a[np.isfinite(a)]).max() for a in (Q, T))
        assert (m > R.COLL_F32_MAX) == (name in ("huge", "overflow")), (name, m)
    assert 3.0 * float(R.COLL_F32_MAX) < float(R.COLL_PAD_F32)


def test_qt_apart_cases_lie_on_either_side_of_40_binades():
    for binades, usable in ((35, True), (45, False)):
        Q, T = R.qt_apart(binades)
        eq, et = np.frexp(np.abs(Q).max())[1], np.frexp(np.abs(T).max())[1]
        assert (abs(int(eq) - int(et)) <= 40) == usable, (binades, eq, et)
        idx, dist = _knn(Q, T, 8)
        assert np.isfinite(dist).all()


def test_mixed_scale_has_rows_that_flush_in_fp16_beside_rows_that_set_the_scale():
    for a in R.mixed_scale():
        ex = np.frexp(np.abs(a).max())[1]
        scaled = np.ldexp(a.astype(np.float64), 14 - int(ex))            # the fp16 planes' scale (filter_f16.hip)
        flushed = (np.abs(scaled) < 2.0 ** -14).all(axis=1)               # an fp16 subnormal (or zero) in every dimension
        i = np.arange(len(a))
        small, big = (i % 11 == 0) & (i % 7 != 0), (i % 7 == 0) & (i % 11 != 0)
        assert small.sum() >= 20 and big.sum() >= 30
        assert flushed[small].all() and not flushed[~small].any()
        assert (np.abs(scaled[big]).max(axis=1) >= 2.0 ** 11).all()      # within 3 binades of the bank's largest magnitude


def test_nonfinite_rows_trail_as_minus_one_inf():
    Q, T = R.nonfinite()
    idx, dist = _knn(Q, T, R.NT)
    assert (idx[33] == -1).all() and np.isposinf(dist[33]).all()          # the query row with an inf
    others = np.delete(np.arange(R.NQ), 33)
    assert (idx[others, -1] == -1).all() and np.isposinf(dist[others, -1]).all()
    assert (idx[others, :-1] >= 0).all() and np.isfinite(dist[others, :-1]).all()
    assert not (idx == 17).any()                                           # the train row with an inf is never a match


def test_padding_trap_rows_of_1e18_beat_real_rows_for_the_first_half_only():
    Q, images = R.padding_trap()
    assert [im.shape[0] for im in images] == [129, 1, 127]
    S, is_pad = R.stack_with_padding(images)
    assert S.shape[0] == 256 + 128 + 128 and is_pad.sum() == 127 + 127 + 1
    idx, dist = _knn(Q, S, 2)
    assert np.isfinite(dist).all()
    hit = is_pad[idx].any(axis=1)
    h = R.NQ // 2
    assert hit[:h].mean() >= 0.90, hit[:h].mean()
    assert not hit[h:].any()
    # and the first half is beyond the limit a collection accepts, the second half and the images within it
    assert np.abs(Q[:h]).max() > R.COLL_F32_MAX
    assert max(np.abs(Q[h:]).max(), max(np.abs(im).max() for im in images)) <= R.COLL_F32_MAX
