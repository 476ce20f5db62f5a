"""Shared by test_hamming_widths_host.py and test_hamming_widths_gpu.py: binary rows in which every 16-byte K step and the
last real byte of a row decide the answers, and the stacked-collection forms of the references that exist already.  Nothing
here touches the GPU, and nothing here computes a distance of its own: hamming_ref, masked_ref and hamming_radius_ref do.

The Hamming kernels are compiled once per K-step count KS = ceil(bytes / 16) = 1 .. 4.  ``family(width, n, seed)``:
* every row is one of ``pool`` random base rows of ``width`` bytes (the pool is seeded by the width alone: a query bank and a
  train bank of one width share it), with f = (0, 1, 2, 5)[(i // KS) % 4] bits flipped in row i;
* ALL flipped bits of row i lie in the one 16-byte segment s = i % KS (bytes 16 s .. min(16 s + 15, width - 1)), the bits of
  the segment's last real byte first -- f <= 5 < 8, so they are bits of that byte: for the last segment the row's last byte.
Rows of one base sit at h = 0 .. 10 from each other (masses of ties: the lowest index decides all the time), rows of different
bases at about 4 * width.  Which of the near rows comes first depends on single bits of one segment each, so a kernel that
skips a K step, reads a stale or foreign byte behind ``width``, or scales a row offset by the wrong row size cannot produce
the reference's lists (test_hamming_widths_host.py asserts that as a precondition, per width and segment)."""
import functools

import numpy as np

import hamming_ref
import masked_ref

WIDTHS = [1, 16, 17, 32, 33, 40, 48, 49, 64]            # pair calls: KS = 1, 1, 2, 2, 3, 3, 3, 4, 4
COLL_WIDTHS = [1, 33, 48, 64]                           # collection calls: KS = 1, 3, 3, 4
NQ, NT = 300, 1100                                      # two 256-row output chunks; 9 stages of 128 in 3 splits, the last partial
IMAGE_SIZES = [129, 0, 1, 128, 700, 127]                # partial stages, an empty image, an image that ends on a stage
FLIPS = (0, 1, 2, 5)
TAU = 0.8


def ksteps(width):
    return (width + 15) // 16


def segment(width, s):
    """(first byte, one past the last real byte) of 16-byte segment s."""
    assert 0 <= s < ksteps(width)
    return 16 * s, min(16 * s + 16, width)


def family(width, n, seed, pool=24):
    ks = ksteps(width)
    base = np.random.default_rng(5000 + width).integers(0, 256, (pool, width), dtype=np.uint8)
    rng = np.random.default_rng(7000 + 1000 * seed + width)
    rows = base[rng.integers(0, pool, n)].copy()
    for i in range(n):
        f = FLIPS[(i // ks) % 4]
        lo, hi = segment(width, i % ks)
        last = 8 * (hi - 1) + rng.permutation(8)                       # the last real byte's bits first ...
        rest = 8 * lo + rng.permutation(8 * (hi - 1 - lo))             # ... then the segment's other bits
        bits = np.concatenate([last, rest])[:f]
        np.bitwise_xor.at(rows[i], bits >> 3, (1 << (bits & 7)).astype(np.uint8))
    return rows


def zero_segment(A, width, s):
    lo, hi = segment(width, s)
    out = A.copy()
    out[:, lo:hi] = 0
    return out


def zero_last_byte(A, width):
    out = A.copy()
    out[:, width - 1] = 0
    return out


@functools.lru_cache(maxsize=None)
def pair(width):
    """(Q [300, width], T [1100, width]), read-only."""
    Q, T = family(width, NQ, 1), family(width, NT, 2)
    Q.setflags(write=False)
    T.setflags(write=False)
    return Q, T


@functools.lru_cache(maxsize=None)
def gallery(width):
    """(Q [300, width], the six images), read-only; every image numbers its rows from 0 (its own segment cycle)."""
    images = [family(width, n, 10 + i) for i, n in enumerate(IMAGE_SIZES)]
    for im in images:
        im.setflags(write=False)
    return pair(width)[0], images


def sweep_splits(nq, nt):
    """(splits, stages per split) of plan_hamming for an nq x nt sweep, restated: 256 output rows per workgroup, about 2048
    workgroups, a split of at least 4 whole 128-row stages."""
    chunks, stages = (nq + 255) // 256, (nt + 127) // 128
    ns = max(1, min((2048 + chunks - 1) // chunks, (stages + 3) // 4))
    per = (stages + ns - 1) // ns
    return (stages + per - 1) // per, per


# ---- the stacked forms of the references: a collection answers on the concatenated rows, every hit as (image, row) ---------
def first_rows(images):
    return np.concatenate([[0], np.cumsum([im.shape[0] for im in images])]).astype(np.int64)


def concat(images, width):
    return np.concatenate([im.reshape(-1, width) for im in images]) if images else np.zeros((0, width), np.uint8)


def to_img_row(idx, images):
    fr = first_rows(images)
    img = np.where(idx >= 0, np.searchsorted(fr, idx, side="right") - 1, -1).astype(np.int32)
    return img, np.where(idx >= 0, idx - fr[np.maximum(img, 0)], -1).astype(np.int32)


def stacked_knn(Q, images, k):
    """(img, row inside the image, dist) [nq, k]: hamming_ref.knn on the concatenated rows."""
    idx, dist = hamming_ref.knn(Q, concat(images, Q.shape[1]), k)
    img, loc = to_img_row(idx, images)
    return img, loc, dist


def stacked_knn_masked(Q, images, masks, k):
    """masks[i] = uint8 [nq, rows of image i]: masked_ref.knn_bin on the concatenated rows and masks."""
    dense = np.concatenate([np.asarray(m, np.uint8).reshape(Q.shape[0], -1) for m in masks], axis=1)
    idx, dist = masked_ref.knn_bin(Q, concat(images, Q.shape[1]), dense, k)
    img, loc = to_img_row(idx, images)
    return img, loc, dist


def ratios(idx, dist):
    """float64 d0 / d1 per row of a 2-NN list, NaN without a second neighbour (hamming_ref.ratio_match's rule)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(idx[:, 1] >= 0, dist[:, 0].astype(np.float64) / dist[:, 1].astype(np.float64), np.nan)


def stacked_ratio(Q, images, tau):
    """(qidx, img, row, dist, ratio) of the query rows whose stacked 2-NN list passes the ratio test, and the votes of mode 0
    (per image of the first neighbour) and of mode 1 (the test inside every image separately)."""
    idx, dist = hamming_ref.knn(Q, concat(images, Q.shape[1]), 2)
    r = ratios(idx, dist)
    with np.errstate(invalid="ignore"):
        s = np.nonzero(r < tau)[0]
    img, loc = to_img_row(idx, images)
    accepted = (s.astype(np.int32), img[s, 0], loc[s, 0], dist[s, 0], r[s])
    votes0 = np.bincount(img[s, 0], minlength=len(images)).astype(np.int64)
    votes1 = np.array([len(hamming_ref.ratio_match(Q, im, tau)[0]) for im in images], np.int64)
    return accepted, votes0, votes1


def merged_knn(Q, images, k):
    """stacked_knn put together the other way round, for the host test: hamming_ref.knn image by image, then per query row
    the k smallest (h, image, row) of all the lists."""
    nq = Q.shape[0]
    per = [hamming_ref.knn(Q, im, k) for im in images]
    img = np.full((nq, k), -1, np.int32)
    loc = np.full((nq, k), -1, np.int32)
    dist = np.full((nq, k), np.inf, np.float32)
    for q in range(nq):
        cand = sorted((float(d[q, j]), i, int(ix[q, j])) for i, (ix, d) in enumerate(per) for j in range(k) if ix[q, j] >= 0)[:k]
        for j, (d, i, r) in enumerate(cand):
            img[q, j], loc[q, j], dist[q, j] = i, r, d
    return img, loc, dist
