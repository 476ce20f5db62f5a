"""CPU: the preconditions of tests/test_hamming_widths_gpu.py.  The data of tests/hamming_width_ref.py must make every 16-byte
K step and every row's last real byte load-bearing -- the GPU tests rely on it to notice a skipped K step, a stale byte behind
the row's width or a row offset scaled by the wrong row size -- and the stacked references must be the per-image ones."""
import numpy as np
import pytest

import hamming_ref as H
import hamming_width_ref as W
import masked_ref


def test_the_width_lists_cover_every_k_step_count():
    assert sorted({W.ksteps(w) for w in W.WIDTHS}) == [1, 2, 3, 4]
    assert sorted({W.ksteps(w) for w in W.COLL_WIDTHS}) == [1, 3, 4]      # (KS = 2 is the 32 bytes of the older collection tests)
    assert all(1 <= w <= 64 for w in W.WIDTHS + W.COLL_WIDTHS) and set(W.COLL_WIDTHS) <= set(W.WIDTHS)
    for ks in (2, 3, 4):                                     # one byte into the step, and the step's full width
        assert 16 * (ks - 1) + 1 in W.WIDTHS and 16 * ks in W.WIDTHS
    assert 1 in W.WIDTHS and 16 in W.WIDTHS
    # the shapes: two output chunks with a partial second one, three splits of three stages with a partial last stage
    assert W.NQ > 256 and W.NQ % 256 != 0
    assert W.sweep_splits(W.NQ, W.NT) == (3, 3) and W.NT % 128 != 0 and W.sweep_splits(W.NT, W.NQ)[0] == 1
    assert 0 in W.IMAGE_SIZES and 1 in W.IMAGE_SIZES and 128 in W.IMAGE_SIZES and any(n > 512 for n in W.IMAGE_SIZES)
    assert any(n % 128 not in (0, 1) for n in W.IMAGE_SIZES)


@pytest.mark.parametrize("width", sorted(set(W.WIDTHS + W.COLL_WIDTHS)))
def test_the_family_is_what_its_description_says(width):
    ks = W.ksteps(width)
    base = W.family(width, 24 * 40, 0)                       # f = 0 rows show the pool
    A = W.family(width, 400, 3)
    pool = {r.tobytes() for r in base[[i for i in range(len(base)) if (i // ks) % 4 == 0]]}
    assert len(pool) <= 24
    for i, row in enumerate(A):
        f = W.FLIPS[(i // ks) % 4]
        lo, hi = W.segment(width, i % ks)
        diffs = [np.unpackbits(row ^ np.frombuffer(b, np.uint8)) for b in pool]
        if width > 1:                                        # (one-byte base rows lie closer to each other than 5 bits)
            assert min(int(d.sum()) for d in diffs) == f
        best = [d for d in diffs if int(d.sum()) == f][0]    # exactly f bits from a base row ...
        where = np.nonzero(best)[0] // 8
        assert ((where >= lo) & (where < hi)).all()          # ... all inside segment i % KS ...
        assert (where == hi - 1).all()                       # ... in its last real byte (f < 8)
    assert np.array_equal(W.family(width, 400, 3), A)        # deterministic; another seed gives other rows
    assert not np.array_equal(W.family(width, 400, 4), A)


@pytest.mark.parametrize("width", sorted(set(W.WIDTHS + W.COLL_WIDTHS)))
def test_every_segment_and_the_last_byte_are_load_bearing(width):
    Q, T = W.pair(width)
    assert Q.shape == (W.NQ, width) and T.shape == (W.NT, width)
    idx, dist = H.knn(Q, T, 2)
    xt, _ = H.xcheck(Q, T)
    assert (dist[:, 0] == dist[:, 1]).sum() >= 50            # ties between the first two neighbours: the index decides
    assert len(H.ratio_match(Q, T, W.TAU)[0]) >= 10          # the ratio test accepts some rows ...
    assert len(H.ratio_match(Q, T, W.TAU)[0]) <= W.NQ - 10   # ... and rejects some
    assert 10 <= (xt >= 0).sum() <= W.NQ - 10                # the same for the cross-check
    for s in range(W.ksteps(width)):
        Qz, Tz = W.zero_segment(Q, width, s), W.zero_segment(T, width, s)
        zi, _ = H.knn(Qz, Tz, 2)
        changed = int((zi != idx).any(axis=1).sum())
        assert changed >= 30, (width, s, changed)            # a kernel blind to segment s cannot return idx
        zx, _ = H.xcheck(Qz, Tz)
        assert int((zx != xt).sum()) >= 10, (width, s)
        # one side alone: a step dropped from only the query or only the train bank
        for a, b in ((Qz, T), (Q, Tz)):
            assert int((H.knn(a, b, 2)[0] != idx).any(axis=1).sum()) >= 30, (width, s)
    Ql, Tl = W.zero_last_byte(Q, width), W.zero_last_byte(T, width)
    assert int((H.knn(Ql, Tl, 2)[0] != idx).any(axis=1).sum()) >= 30, width
    assert int((H.knn(Q, Tl, 2)[0] != idx).any(axis=1).sum()) >= 30, width
    # a foreign byte behind the row (0xFF in one bank, as a pitched source leaves it) would show as well
    if width < 64:
        Qw = np.concatenate([Q, np.full((W.NQ, 1), 0xFF, np.uint8)], axis=1)
        Tw = np.concatenate([T, np.zeros((W.NT, 1), np.uint8)], axis=1)
        assert not np.array_equal(H.knn(Qw, Tw, 2)[1], dist)


@pytest.mark.parametrize("width", W.COLL_WIDTHS)
def test_the_stacked_references_are_the_per_image_ones(width):
    Q, images = W.gallery(width)
    assert [im.shape[0] for im in images] == W.IMAGE_SIZES and all(im.shape[1] == width for im in images)
    for k in (1, 2, 3, 8):
        a, b = W.stacked_knn(Q, images, k), W.merged_knn(Q, images, k)
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), (width, k)
    # the ratio test on the stacked lists, the votes of both modes
    accepted, votes0, votes1 = W.stacked_ratio(Q, images, W.TAU)
    img, loc, dist = W.merged_knn(Q, images, 2)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(img[:, 1] >= 0, dist[:, 0].astype(np.float64) / dist[:, 1].astype(np.float64), np.nan)
        s = np.nonzero(r < W.TAU)[0]
    assert len(s) >= 5 and np.array_equal(accepted[0], s) and np.array_equal(accepted[1], img[s, 0])
    assert np.array_equal(accepted[2], loc[s, 0]) and np.array_equal(accepted[3], dist[s, 0]) and np.array_equal(accepted[4], r[s])
    assert votes0.sum() == len(s) and votes0[1] == 0 and votes1[1] == 0 and votes1[2] == 0      # (an image of one row has no ratio)
    for i, im in enumerate(images):
        ei, ed = H.knn(Q, im, 2)
        with np.errstate(divide="ignore", invalid="ignore"):
            assert votes1[i] == int((np.where(ei[:, 1] >= 0, ed[:, 0].astype(np.float64) / ed[:, 1], np.nan) < W.TAU).sum())
    assert votes1.sum() > 0
    # the masked form with every pair permitted is the unmasked one; with image 4 forbidden nothing comes from image 4
    ones = [np.ones((W.NQ, n), np.uint8) for n in W.IMAGE_SIZES]
    assert all(np.array_equal(x, y) for x, y in zip(W.stacked_knn_masked(Q, images, ones, 3), W.stacked_knn(Q, images, 3)))
    ones[4][:] = 0
    mi, ml, md = W.stacked_knn_masked(Q, images, ones, 3)
    rest = images[:4] + [images[4][:0]] + images[5:]
    assert not (mi == 4).any() and all(np.array_equal(x, y) for x, y in zip((mi, ml, md), W.stacked_knn(Q, rest, 3)))
    # the gallery keeps every segment load-bearing inside the single images that have more than a handful of rows
    for i in (0, 3, 4, 5):
        idx = H.knn(Q, images[i], 2)[0]
        for s in range(W.ksteps(width)):
            zi = H.knn(W.zero_segment(Q, width, s), W.zero_segment(images[i], width, s), 2)[0]
            assert int((zi != idx).any(axis=1).sum()) >= 20, (width, i, s)
    assert masked_ref.pad128(W.NT) == 1152
