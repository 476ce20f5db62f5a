"""CPU: the reference helper of the grown-bank tests (tests/grown_ref.py) itself -- the append arithmetic against cases
written out by hand, the index remaps, and that the adversarial data really puts a gap row nearer than every real row for
EVERY row of the other bank (float64), so that test_grown_banks_gpu.py cannot pass because its data were harmless."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grown_ref as gr          # noqa: E402


def test_offsets_of_hand_written_appends():
    lay = gr.Layout([1, 31, 32, 33, 0, 100])
    # 1 row at 0; the next append starts at 32 (rows 1 .. 31 are a gap) and ends at 63; 64 .. 95; 96 .. 128; the empty
    # append reports the next tile boundary, 160, and moves nothing; 100 rows at 160 .. 259
    assert lay.first == [0, 32, 64, 96, 160, 160]
    assert lay.n_phys == 260 and lay.n_real == 197
    want_gaps = list(range(1, 32)) + [63] + list(range(129, 160))
    assert lay.gaps.tolist() == want_gaps
    assert lay.phys[:3].tolist() == [0, 32, 33] and lay.phys[-1] == 259
    assert lay.phys[32] == 64 and lay.phys[64] == 96 and lay.phys[96] == 128 and lay.phys[97] == 160


@pytest.mark.parametrize("sizes, first, n_phys, gaps", [
    ([1], [0], 1, []),
    ([31, 1], [0, 32], 33, [31]),
    ([32, 1], [0, 32], 33, []),
    ([33, 1], [0, 64], 65, list(range(33, 64))),
    ([0, 5], [0, 0], 5, []),
    ([5, 0], [0, 32], 5, []),                       # a gap behind the last row is no interior gap
    ([5, 0, 0, 2], [0, 32, 32, 32], 34, list(range(5, 32))),
    ([100, 100], [0, 128], 228, list(range(100, 128))),
    ([], [], 0, []),
])
def test_offsets_small_cases(sizes, first, n_phys, gaps):
    lay = gr.Layout(sizes)
    assert lay.first == first and lay.n_phys == n_phys and lay.gaps.tolist() == gaps
    assert lay.n_real == sum(sizes) == n_phys - len(gaps)


def test_the_patterns_of_the_gpu_tests():
    a, b = gr.Layout(gr.PATTERNS["in_stage"]), gr.Layout(gr.PATTERNS["across"])
    assert a.first == [0, 32, 64, 96, 160, 160, 288, 352] and a.n_phys == 357 and a.n_real == 266
    assert b.first == [0, 160, 192] and b.n_phys == 319 and b.n_real == 257
    # gaps inside a 128-row stage (1 .. 31, 63), across a stage boundary (260 .. 287 runs over 256) ...
    assert {1, 31, 63, 129, 159, 260, 287} <= set(a.gaps.tolist()) and not {0, 32, 128, 259, 288, 356} & set(a.gaps.tolist())
    assert b.gaps.tolist() == list(range(129, 160)) + list(range(161, 192))
    assert max(a.n_phys, b.n_phys) < 700


def test_rows_accept_arrays_and_split_inverts_dense():
    rng = np.random.default_rng(1)
    parts = [rng.integers(0, 256, (n, 7), dtype=np.uint8) for n in (3, 0, 40, 1)]
    lay = gr.Layout(parts)
    assert lay.sizes == [3, 0, 40, 1] and lay.first == [0, 32, 32, 96]
    dense = lay.dense(parts)
    assert dense.shape == (44, 7)
    back = lay.split(dense)
    assert [p.shape[0] for p in back] == lay.sizes and all(np.array_equal(x, y) for x, y in zip(parts, back))


def test_index_remaps_round_trip():
    lay = gr.Layout(gr.PATTERNS["in_stage"])
    real = np.arange(lay.n_real, dtype=np.int32)
    phys = lay.to_phys(real)
    assert phys.dtype == np.int32 and np.array_equal(phys, lay.phys) and (np.diff(phys) > 0).all()      # monotone: orders survive
    assert np.array_equal(lay.to_real(phys), real)
    assert not np.isin(phys, lay.gaps).any()
    mixed = np.array([[0, -1], [lay.n_real - 1, 5]], dtype=np.int32)
    assert lay.to_phys(mixed).tolist() == [[0, -1], [356, 36]]
    assert lay.to_real(np.array([-1, 0, 1, 32, 63, 356])).tolist() == [-1, 0, -2, 1, -2, 265]
    # LISTS and ROWS, train side and query side
    idx = np.array([[3, -1]] * 4, dtype=np.int32)
    dist = np.ones((4, 2), np.float32)
    assert lay.lists_train((idx, dist))[0].tolist() == [[34, -1]] * 4
    rows = (np.array([0, 2], np.int32), np.array([1, 40], np.int32), np.zeros(2, np.float32))
    assert lay.rows_train(rows)[1].tolist() == [32, 72] and lay.rows_train(rows)[0] is rows[0]
    per_phys = np.arange(lay.n_phys)
    assert np.array_equal(lay.lists_query((per_phys,))[0], lay.phys)
    got = lay.rows_query((np.array([0, 1, 32, 63, 64], np.int32), np.array([9, 8, 7, 6, 5], np.int32)))
    assert got[0].tolist() == [0, 1, 32] and got[1].tolist() == [9, 7, 5]


@pytest.mark.parametrize("kind", ["u8", "f32"])
@pytest.mark.parametrize("pattern", sorted(gr.PATTERNS))
@pytest.mark.parametrize("dim", [128, 61])
def test_adversarial_data_put_a_gap_row_nearest_for_every_row(kind, pattern, dim):
    lay, G, O = gr.dataset(kind, pattern, dim, "adv")
    assert G.shape == (lay.n_real, dim) and O.shape == (gr.N_OTHER, dim)
    assert G.dtype == O.dtype == (np.uint8 if kind == "u8" else np.float32)
    assert gr.gap_is_nearest(kind, G, O).all()
    # the same by hand for one row, in float64, against what a gap row holds inside the bank (uint8: every byte 128, which
    # the bank stores as 0 after its shift by 128; float32: zeros)
    o = O[17].astype(np.float64)
    fill = 128.0 if kind == "u8" else 0.0
    assert ((o - fill) ** 2).sum() < ((G.astype(np.float64) - o[None, :]) ** 2).sum(axis=1).min()
    # the values are what the issue names: all 256 byte values / a unit normal
    if kind == "u8":
        assert G.min() == 0 and G.max() == 255 and O.min() == 0 and O.max() == 255
    else:
        assert abs(float(G.mean())) < 0.05 and abs(float(G.std()) - 1.0) < 0.05


@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_siftlike_data_keep_gap_rows_far_and_have_matches(kind):
    lay, G, O = gr.dataset(kind, "in_stage", 128, "sift")
    assert not gr.gap_is_nearest(kind, G, O).any()
    t, _ = gr.ref_xcheck1(O, G)
    assert (t >= 0).sum() > 30                                  # planted pairs: the cross-check has something to find


def test_rescan_data_tie_inside_the_filter_margin_with_the_gap_row_nearest():
    """The data of the per-row rescan test: what makes the fp16 filter flag a row (many candidates within its margin of the
    best) and what makes a scan that scores gap rows wrong (the zero row nearer than every real row), in float64."""
    lay, G, O, small = gr.rescan_dataset()
    assert lay.n_phys == 220 and lay.n_real == 157 and len(lay.gaps) == 63 and len(small) == gr.RESCAN_SMALL
    assert O.shape == (gr.RESCAN_OTHER, 128) and gr.RESCAN_OTHER <= 256 and lay.n_phys <= 256       # rescans, not a whole-call redo
    assert gr.gap_is_nearest("f32", G, O).all()
    d2 = gr.d2_f64(O, G)
    nm_max = float((G.astype(np.float64) ** 2).sum(1).max())
    margin = (1.1 / 1024.0) * ((O.astype(np.float64) ** 2).sum(1) + nm_max)                          # filter_f16.hip's M, per row
    near = d2[:, small]
    assert ((near.max(axis=1) - near.min(axis=1)) < 0.05 * margin).all()                              # a hundred candidates, one margin
    rest = np.delete(d2, small, axis=1)
    assert (rest.min(axis=1) > near.max(axis=1) + 10.0 * margin).all()                                # the full rows: far outside it
    # the tiny rows among themselves (fm_self_dist): for most of them (the nearest of 99 siblings has a tail) the zero row is
    # nearer than every sibling -- any one such row fails a scan that scores gap rows --, and the siblings are within the margin
    S = G[small].astype(np.float64)
    dd = gr.d2_f64(S, S) + np.diag(np.full(len(small), np.inf))
    assert ((S * S).sum(1) < dd.min(axis=1)).mean() > 0.8
    assert (dd[np.isfinite(dd)].max() < 0.05 * (1.1 / 1024.0) * nm_max)


def test_reference_shapes_on_a_small_case():
    rng = np.random.default_rng(5)
    Q = rng.integers(0, 256, (9, 16), dtype=np.uint8)
    T = rng.integers(0, 256, (12, 16), dtype=np.uint8)
    d = np.sqrt(gr.d2_f64(Q, T).astype(np.float32))
    idx, dist = gr.ref_knn(Q, T, 3)
    assert np.array_equal(idx[:, 0], d.argmin(axis=1)) and np.array_equal(dist[:, 0], d.min(axis=1))
    q, t, dd = gr.ref_radius(Q, T, np.float32(np.median(d)))
    assert len(q) == (d < np.float32(np.median(d))).sum() and (np.diff(q) >= 0).all()
    assert np.array_equal(dd, d[q, t])
    off = np.concatenate([[0], np.cumsum(np.bincount(q, minlength=9))])
    assert np.array_equal(gr.radius_rows((off, t, dd))[0], q)
    qa, ta, da, ra = gr.ref_knn2_ratio(Q, T, 0.9)
    assert np.array_equal(ta, idx[qa, 0]) and (ra < 0.9).all()
    for sym in (False, True):
        qm = gr.ref_mutual_ratio(Q, T, 0.95, sym)[0]
        assert set(qm.tolist()) <= set(gr.ref_knn2_ratio(Q, T, 0.95)[0].tolist())
