"""Reference side of the masked radiusMatch tests (test_radius_masked_host.py, test_radius_masked_gpu.py,
test_radius_masked_collection_gpu.py); not a test.

A masked list is the UNMASKED reference list with the forbidden entries removed -- nothing else.  The unmasked lists come from
the reference modules the unmasked calls are tested against: radius_coll_ref.Ref (oracle.bf_knn with k = all rows, cut at
dist < r_i: the cut of test_radius_match_gpu.py) for the integer and the float32 route, hamming_radius_ref.Ref for binary rows,
wide_radius_ref.Ref for wide float rows.  Every data set is 300 query rows x 2100 train rows, which as a collection are the
images SIZES.  The mask patterns live here too.  Nothing here calls the code under test."""
import functools
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (_HERE, os.path.dirname(_HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import hamming_radius_ref as HR     # noqa: E402
import radius_coll_ref as RC        # noqa: E402
import wide_radius_ref as WR        # noqa: E402
import wide_ref                     # noqa: E402
from fastmatch_amd import synth     # noqa: E402

NQ, NT = 300, 2100                  # 300: no multiple of 64, 128 or 256; 2100 = 32 * 64 + 52: a partial last mask word
SIZES = [700, 1, 130, 0, 1269]      # the same train rows as a collection: padding behind four images, an empty image
IMG_ALL, IMG_NONE = 2, 0            # collection masks: image 2 is left all-permitted (None), image 0 all-forbidden
PAIR_SETS = ["i8", "f32", "f32all", "ham8", "ham32", "ham64", "wide129", "wide256"]
COLL_SETS = ["i8", "f32", "ham32"]
PATTERNS = ["random", "band", "ones", "zeros", "walk", "first", "last", "third"]
BAND = 40


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def kind(name):
    return "ham" if name.startswith("ham") else "wide" if name.startswith("wide") else name


@functools.lru_cache(maxsize=None)
def data(name):
    """(Q, T) of a data set, read-only.  f32: the "floaty" rows of test_radius_match_gpu.py.  f32all: the same train rows times
    2^45 -- the banks' fp16 scales lie more than 40 binades apart, so the float32 route has no filter planes for the pair and
    every pair is a candidate (the `all` path of the sweep)."""
    if name in ("i8", "f32", "f32all"):
        Q, T, _ = synth.planted_pair(NQ, NT, seed=23)
        if name != "i8":
            rng = np.random.default_rng(29)
            Q = (Q.astype(np.float32) / 512.0 + rng.random(Q.shape, dtype=np.float32) * 1e-3).astype(np.float32)
            T = (T.astype(np.float32) / 512.0 + rng.random(T.shape, dtype=np.float32) * 1e-3).astype(np.float32)
            if name == "f32all":
                T = (T * np.float32(2.0 ** 45)).astype(np.float32)
    elif name.startswith("ham"):
        Q, T = HR.data(int(name[3:]), NQ, NT)
    else:
        Q, T = wide_ref.clustered(NQ, NT, int(name[4:]), 500 + int(name[4:]))
    Q, T = np.ascontiguousarray(Q), np.ascontiguousarray(T)
    Q.setflags(write=False)
    T.setflags(write=False)
    return Q, T


def images(name):
    return [np.ascontiguousarray(im) for im in np.split(data(name)[1], np.cumsum(SIZES)[:-1])]


@functools.lru_cache(maxsize=None)
def ref(name):
    """The unmasked reference of a data set over the images SIZES (a pair reads the global index, cut(...)[4])."""
    Q = data(name)[0]
    mod = {"ham": HR, "wide": WR}.get(kind(name), RC)
    return mod.Ref(Q, images(name))


def _sorted_dist(name):
    r = ref(name)
    return r.sorted if kind(name) == "ham" else r.dist


def radius(name, k=40):
    """A scalar radius of about k hits per row: the median k-th distance of the reference, nudged up."""
    return np.nextafter(np.float32(np.median(_sorted_dist(name)[:, k])), np.float32(np.inf))


def row_radii(name, seed=3):
    """One ordinary radius per row: just above one of the row's 60 smallest reference distances."""
    rng = np.random.default_rng(seed)
    d = _sorted_dist(name)
    r = d[np.arange(NQ), rng.integers(20, 60, NQ)].astype(np.float32)
    return np.nextafter(r, np.float32(np.inf))


def mixed_radii(name):
    """The reference modules' own mixed arrays: 0, a negative value, NaN and +inf among ordinary radii."""
    mod = {"ham": HR, "wide": WR}.get(kind(name), RC)
    return mod.mixed_radii(ref(name))


def radii(name):
    return [("scalar", radius(name)), ("rows", row_radii(name)), ("mixed", mixed_radii(name))]


@functools.lru_cache(maxsize=None)
def mask(pattern, nq=NQ, nt=NT, seed=0):
    """bool [nq, nt], read-only.  random: density 0.5.  band: BAND consecutive permitted train rows per query row (most mask
    words zero: the skip paths).  walk: (j % 64 == i % 64), every bit position of a word in every lane group.  first / last:
    the single train row 0 / nt - 1.  third: random, every third query row fully forbidden."""
    rng = np.random.default_rng(4000 + seed)
    M = np.zeros((nq, nt), bool)
    if pattern in ("random", "third"):
        M = rng.random((nq, nt)) < 0.5
        if pattern == "third":
            M[0::3] = False
    elif pattern == "band":
        for i in range(nq):
            s = (i * 37) % max(1, nt - BAND)
            M[i, s:s + BAND] = True
    elif pattern == "ones":
        M[:] = True
    elif pattern == "walk":
        M = (np.arange(nt)[None, :] % 64) == (np.arange(nq)[:, None] % 64)
    elif pattern == "first":
        M[:, 0] = True
    elif pattern == "last":
        M[:, nt - 1] = True
    elif pattern != "zeros":
        raise ValueError(pattern)
    M = np.ascontiguousarray(M)
    M.setflags(write=False)
    return M


@functools.lru_cache(maxsize=None)
def coll_mask(pattern):
    """The pattern over the concatenated real rows with image IMG_ALL all-permitted and image IMG_NONE all-forbidden."""
    M = mask(pattern).copy()
    fr = np.concatenate([[0], np.cumsum(SIZES)])
    M[:, fr[IMG_ALL]:fr[IMG_ALL + 1]] = True
    M[:, fr[IMG_NONE]:fr[IMG_NONE + 1]] = False
    M.setflags(write=False)
    return M


def per_image(M):
    """A [nq, total] mask as the per-image list a collection call takes (None: everything permitted)."""
    fr = np.concatenate([[0], np.cumsum(SIZES)])
    return [None if i == IMG_ALL else np.ascontiguousarray(M[:, fr[i]:fr[i + 1]]) for i in range(len(SIZES))]


def filtered(cut, M):
    """cut = Ref.cut(r) = (offsets, img, loc, dist, global idx), flat; M bool [nq, total].  The same lists without the
    entries whose (query row, global train row) M forbids."""
    off, img, loc, dist, glob = cut
    nq = off.shape[0] - 1
    rows = np.repeat(np.arange(nq), np.diff(off))
    keep = M[rows, glob] if rows.size else np.zeros(0, bool)
    cnt = np.bincount(rows[keep], minlength=nq) if rows.size else np.zeros(nq, np.int64)
    noff = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    return noff, img[keep], loc[keep], dist[keep], glob[keep]


def want(name, r, M):
    return filtered(ref(name).cut(r), M)


def same_pair(got, wanted, what=""):
    """got = (offsets, idx, dist) of a bank pair; wanted = filtered(...).  Indices exactly, distances as bit patterns."""
    off, idx, dist = got
    woff, _, _, wdist, wglob = wanted
    assert off.dtype == np.int64 and np.array_equal(off, woff), "%s offsets" % (what,)
    assert idx.shape == dist.shape == (int(woff[-1]),), "%s sizes" % (what,)
    assert np.array_equal(idx, wglob), "%s idx" % (what,)
    assert np.array_equal(bits(dist), bits(wdist)), "%s dist" % (what,)


def same_coll(got, wanted, what=""):
    off, img, idx, dist = got
    woff, wimg, widx, wdist = wanted[:4]
    assert off.dtype == np.int64 and np.array_equal(off, woff), "%s offsets" % (what,)
    assert img.shape == idx.shape == dist.shape == (int(woff[-1]),), "%s sizes" % (what,)
    assert np.array_equal(img, wimg), "%s img" % (what,)
    assert np.array_equal(idx, widx), "%s idx" % (what,)
    assert np.array_equal(bits(dist), bits(wdist)), "%s dist" % (what,)
