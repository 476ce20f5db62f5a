"""Host: Hamming radiusMatch without a GPU.

* fast-match_amd/csrc/ham_radius.h through a stand-alone C++ harness: for every radius of a dense set and every h of [0, W],
  float32(h) < r  <=>  h <= ham_radius_limit(r, W)  <=>  W - 2 h >= ham_radius_dot_min(limit, W) -- the contract's test, the
  integer limit and the threshold the sweep compares its raw dot product with.
* The reference (tests/hamming_radius_ref.py) against a naive double loop on tiny inputs, a tie group and r exactly on an
  integer included.
* matchutil.hamming_radius_match(_arrays): every ValueError is raised before a context is even looked up."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import hamming_radius_ref as HR
from fastmatch_amd import matchutil

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fast-match_amd", "csrc")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)

HARNESS = r"""
#include "ham_radius.h"
#include <stdio.h>
#include <string.h>
#include <stdint.h>
// stdin: lines "<W> <radius bits hex>"; stdout per line: "<limit> <threshold bits hex> <errors>"
int main()
{
    int W; unsigned rb;
    while (scanf("%d %x", &W, &rb) == 2) {
        float r; memcpy(&r, &rb, 4);
        const int H = fm::ham_radius_limit(r, W);
        const float T = fm::ham_radius_dot_min(H, W);
        long errors = (H < -1 || H > W);
        for (int h = 0; h <= W; ++h) {
            const bool in = (float)h < r;
            errors += in != (h <= H);
            errors += in != ((float)(W - 2 * h) >= T);
        }
        unsigned tb; memcpy(&tb, &T, 4);
        printf("%d %08x %ld\n", H, tb, errors);
    }
    return 0;
}
"""

WIDTHS = [8, 136, 256, 512]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if HIPCC is None:
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("ham_radius")
    src = d / "h.cpp"
    src.write_text(HARNESS)
    exe = d / "h"
    subprocess.check_call([HIPCC, "-O2", "-std=c++17", "-x", "c++", "-I", CSRC, str(src), "-o", str(exe)])
    return str(exe)


def _radii(W):
    k = np.arange(0, W + 2, dtype=np.float32)
    inf = np.float32(np.inf)
    special = np.array([-1.0, -0.0, 1e-45, np.nan, np.inf, -np.inf, 1e30], np.float32)     # (1e-45: a denormal)
    return np.concatenate([k, np.nextafter(k, inf), np.nextafter(k, -inf), k + np.float32(0.5), special]).astype(np.float32)


def _run(exe, W, radii):
    inp = "".join("%d %08x\n" % (W, int(b)) for b in radii.view(np.uint32))
    out = subprocess.run([exe], input=inp, capture_output=True, text=True, check=True).stdout.split("\n")
    res = [line.split() for line in out if line.strip()]
    assert len(res) == len(radii)
    return [(int(a), np.array([int(b, 16)], np.uint32).view(np.float32)[0], int(c)) for a, b, c in res]


@pytest.mark.parametrize("W", WIDTHS)
def test_limit_and_threshold_agree_with_the_float_compare(harness, W):
    radii = _radii(W)
    hs = np.arange(0, W + 1, dtype=np.float32)
    for r, (H, T, errors) in zip(radii, _run(harness, W, radii)):
        assert errors == 0, (W, r, H, T)
        with np.errstate(invalid="ignore"):
            inside = hs < r
        want = int(np.nonzero(inside)[0].max()) if inside.any() else -1        # the contract's H_i, from NumPy's float32 compare
        assert H == want, (W, r, H, want)
        assert T == (np.inf if H < 0 else W - 2 * H), (W, r, H, T)


def test_edge_radii_by_name(harness):
    W = 256
    cases = [(-1.0, -1), (-0.0, -1), (0.0, -1), (1e-45, 0), (np.nan, -1), (np.inf, W), (-np.inf, -1), (1e30, W), (0.5, 0),
             (1.0, 0), (50.0, 49), (50.5, 50), (256.0, 255), (256.5, 256), (257.0, 256)]
    radii = np.array([r for r, _ in cases], np.float32)
    for (r, want), (H, T, errors) in zip(cases, _run(harness, W, radii)):
        assert errors == 0 and H == want, (r, H, want)


def _naive(Q, T, radii):
    """The contract as a double loop: (offsets, idx, dist)."""
    off, idx, dist = [0], [], []
    for i in range(len(Q)):
        hits = []
        for j in range(len(T)):
            h = sum(bin(int(a) ^ int(b)).count("1") for a, b in zip(Q[i], T[j]))
            if np.float32(h) < np.float32(radii[i]):
                hits.append((h, j))
        hits.sort()
        idx += [j for _, j in hits]
        dist += [float(h) for h, _ in hits]
        off.append(len(idx))
    return np.array(off, np.int64), np.array(idx, np.int32), np.array(dist, np.float32)


def test_reference_equals_a_naive_double_loop():
    rng = np.random.default_rng(5)
    for nbytes in (1, 3, 8, 17):
        Q = rng.integers(0, 256, (9, nbytes), dtype=np.uint8)
        T = rng.integers(0, 256, (23, nbytes), dtype=np.uint8)
        T[[3, 11, 19]] = Q[2]                        # a tie group at h = 0 for row 2 ...
        T[[4, 20]] = Q[2] ^ np.uint8(1)              # ... and one at h = nbytes
        ref = HR.Ref(Q, T)
        h27 = float(ref.h[2, 7])
        for r in (0.0, 0.5, float(nbytes), float(nbytes) + 0.5, 4.0, h27, np.nextafter(np.float32(h27), np.float32(np.inf)),
                  8.0 * nbytes, np.inf, np.nan, -1.0):
            want = _naive(Q, T, [r] * len(Q))
            HR.same_pair_lists(want, ref.cut(np.float32(r)), "r = %r" % (r,))
        radii = HR.mixed_radii(ref)
        HR.same_pair_lists(_naive(Q, T, radii), ref.cut(radii), "per-row radii")
        # r exactly on an integer excludes that distance; the tie group ascends by index
        off, _, _, dist, gidx = ref.cut(np.float32(nbytes))
        assert (dist < nbytes).all()
        assert list(gidx[off[2]:off[2] + 3]) == [3, 11, 19]


def test_reference_against_images_reports_image_and_row():
    rng = np.random.default_rng(6)
    images = [rng.integers(0, 256, (n, 4), dtype=np.uint8) for n in (5, 0, 3, 1)]
    Q = rng.integers(0, 256, (4, 4), dtype=np.uint8)
    ref = HR.Ref(Q, images)
    flat = HR.Ref(Q, np.concatenate(images))
    off, img, loc, dist, g = ref.cut(np.inf)
    assert np.array_equal(g, flat.cut(np.inf)[4]) and off[-1] == 4 * 9
    first = np.array([0, 5, 5, 8])
    assert np.array_equal(first[img] + loc, g) and set(img.tolist()) == {0, 2, 3}


def test_split_rule_restated():
    assert HR.sweep_splits(300, 2100) == (5, 4)          # 17 stages: 5 splits of at most 4
    assert HR.sweep_splits(300, 1920) == (4, 4)          # the collection layout's 15 stages
    assert HR.sweep_splits(300, 129) == (1, 2)
    assert HR.sweep_splits(300, 1) == (1, 1)
    assert HR.sweep_splits(100000, 100000) == (6, 131)   # 391 query groups, 782 stages


def test_matchutil_refusals_come_before_any_upload(monkeypatch):
    def boom(options):
        raise AssertionError("a refusal reached the device")
    monkeypatch.setattr(matchutil, "_context", boom)
    u8 = np.zeros((5, 32), np.uint8)
    cases = [
        (u8.astype(np.float32), u8, 3.0, {}, "uint8"),
        (u8, u8.astype(np.int8), 3.0, {}, "uint8"),
        (u8, np.zeros((5, 16), np.uint8), 3.0, {}, "bytes"),
        (np.zeros((5, 65), np.uint8), np.zeros((5, 65), np.uint8), 3.0, {}, "1 .. 64"),
        (np.zeros((5, 0), np.uint8), np.zeros((5, 0), np.uint8), 3.0, {}, "1 .. 64"),
        (u8, u8, 3.0, {"mask": np.ones((5, 5), np.uint8)}, "mask"),
        (u8, u8, np.ones(4, np.float32), {}, "radii"),
        (u8, u8, np.ones(6, np.float32), {}, "radii"),
    ]
    for q, t, r, opts, word in cases:
        for fn in (matchutil.hamming_radius_match_arrays, matchutil.hamming_radius_match):
            with pytest.raises(ValueError, match=word):
                fn(q, t, r, options=opts)
    with pytest.raises(AssertionError, match="reached the device"):      # a valid call does go to the context
        matchutil.hamming_radius_match_arrays(u8, u8, 3.0)
