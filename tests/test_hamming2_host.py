"""Host: NORM_HAMMING2 (K11b, csrc/hamming2.hip) without a GPU.

* The tetrahedral encoding: encode(q) . encode(t) == 3 P - 4 h2 for all 256 x 256 byte pairs and for random rows at every
  width 1 .. 64, h2 by OpenCV's cell-count table; the table agrees with popcount((x | x >> 1) & 0x55), the vector-ALU rule;
  an all-zero encoded row (a padding row) gives dot 0, i.e. h2 = 3 P / 4.
* ham2_radius_dot_min (csrc/ham_radius.h) compiled on its own with the host compiler: float32(h2) < r  <=>  h2 <= limit  <=>
  3 P - 4 h2 >= threshold, at r in {0, NaN, a denormal, k, k +- ulp, k + 0.5, P, > P, +inf}.
* The K-step counts of the width table, the exported and bound symbols, the header's pinned sentences and new notes.
* Every Python refusal comes before the library is touched; the three pinned normType-7 refusals still hold."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import hamming2_ref as H2
from fastmatch_amd import _ffi, matchutil

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fast-match_amd", "csrc")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


def _header():
    return open(os.path.join(ROOT, "include", "fastmatch_hip.h")).read()


# ---- the encoding ---------------------------------------------------------------------------------------------------------
def test_identity_for_all_byte_pairs():
    v = np.arange(256, dtype=np.uint8)[:, None]
    e = H2.encode(v).astype(np.int32)
    assert e.shape == (256, 12) and set(np.unique(e)) == {-1, 1}
    dot = e @ e.T
    h2 = H2.distances(v, v)
    assert np.array_equal(dot, 3 * 4 - 4 * h2)
    assert np.array_equal(h2, H2.distances_by_mask(v, v))
    # the four vertices of the issue's table, cell 0 of a byte: 00, 01, 10, 11 (a = the low bit)
    assert [tuple(e[c, :3]) for c in range(4)] == [(-1, -1, 1), (1, -1, -1), (-1, 1, -1), (1, 1, 1)]
    # where NORM_HAMMING and NORM_HAMMING2 disagree: both bits of a cell differ -> 2 bits, 1 cell
    assert H2.distances(np.array([[0b11]], np.uint8), np.array([[0]], np.uint8))[0, 0] == 1


@pytest.mark.parametrize("nbytes", range(1, 65))
def test_identity_at_every_width(nbytes):
    rng = np.random.default_rng(700 + nbytes)
    Q = rng.integers(0, 256, (9, nbytes), dtype=np.uint8)
    T = rng.integers(0, 256, (11, nbytes), dtype=np.uint8)
    T[3] = Q[2]                                         # a duplicate: h2 = 0, dot = 3 P
    T[4] = ~Q[2]                                        # the complement: every cell differs, h2 = P, dot = -P
    P = 4 * nbytes
    h2 = H2.distances(Q, T)
    dot = H2.encode(Q).astype(np.int32) @ H2.encode(T).astype(np.int32).T
    assert np.array_equal(dot, 3 * P - 4 * h2)
    assert h2[2, 3] == 0 and h2[2, 4] == P
    assert np.array_equal(h2, H2.distances_by_mask(Q, T))
    assert np.abs(dot).max() <= 768                     # every partial sum is an integer the f32 accumulator holds exactly
    # a padding row is all zeros in the encoded plane: dot 0, which decodes to 3 P / 4 -- never excluded by value
    assert not (np.zeros((1, 12 * nbytes), np.int32) @ H2.encode(T).astype(np.int32).T).any()


def test_kstep_table():
    ks = [H2.fp4_steps(b) for b in range(1, 65)]
    last = {k: max(b for b in range(1, 65) if H2.fp4_steps(b) == k) for k in range(1, 7)}
    assert last == {1: 10, 2: 21, 3: 32, 4: 42, 5: 53, 6: 64} and min(ks) == 1 and max(ks) == 6
    assert H2.fp4_steps(32) == 3 and H2.fp4_steps(64) == 6          # an ORB row: exactly three steps, no padding
    assert 12 * 32 == 3 * 128 and 12 * 64 == 6 * 128
    src = open(os.path.join(CSRC, "fm_internal.h")).read()
    assert "return (12 * bytes + 127) / 128;" in src


# ---- ham_radius.h -----------------------------------------------------------------------------------------------------------
HARNESS = r"""
#include "ham_radius.h"
#include <stdio.h>
#include <string.h>
// stdin: lines "<P> <radius bits hex>"; stdout per line: "<limit> <threshold bits hex> <errors>"
int main()
{
    int P; unsigned rb;
    while (scanf("%d %x", &P, &rb) == 2) {
        float r; memcpy(&r, &rb, 4);
        const int H = fm::ham_radius_limit(r, P);
        const float T = fm::ham2_radius_dot_min(H, P);
        long errors = (H < -1 || H > P);
        for (int h = 0; h <= P; ++h) {
            const bool in = (float)h < r;
            errors += in != (h <= H);
            errors += in != ((float)(3 * P - 4 * h) >= T);
        }
        unsigned tb; memcpy(&tb, &T, 4);
        printf("%d %08x %ld\n", H, tb, errors);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if HIPCC is None:
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("ham2_radius")
    src = d / "h.cpp"
    src.write_text(HARNESS)
    exe = d / "h"
    subprocess.check_call([HIPCC, "-O2", "-std=c++17", "-x", "c++", "-I", CSRC, str(src), "-o", str(exe)])
    return str(exe)


@pytest.mark.parametrize("P", [4, 40, 128, 256])
def test_radius_threshold_agrees_with_the_float_compare(harness, P):
    k = np.arange(0, P + 2, dtype=np.float32)
    inf = np.float32(np.inf)
    special = np.array([0.0, -0.0, -1.0, np.nan, 1e-45, P, P + 0.5, 1e30, np.inf, -np.inf], np.float32)
    radii = np.concatenate([k, np.nextafter(k, inf), np.nextafter(k, -inf), k + np.float32(0.5), special]).astype(np.float32)
    inp = "".join("%d %08x\n" % (P, int(b)) for b in radii.view(np.uint32))
    out = [l.split() for l in subprocess.run([harness], input=inp, capture_output=True, text=True, check=True).stdout.split("\n") if l.strip()]
    assert len(out) == len(radii)
    for r, (H, tb, errors) in zip(radii, out):
        H, thr = int(H), np.array([int(tb, 16)], np.uint32).view(np.float32)[0]
        assert int(errors) == 0, (P, r)
        if not r > 0:
            assert H == -1 and thr == np.inf, (P, r)
        elif r > P:
            assert H == P and thr == -P, (P, r)                   # every real row; a padding row (dot 0) would pass: index mask
        else:
            assert H == int(np.ceil(r)) - 1 and thr == 3 * P - 4 * H, (P, r)


# ---- the reference against a naive loop ---------------------------------------------------------------------------------------
def test_reference_against_a_naive_loop():
    rng = np.random.default_rng(5)
    Q = rng.integers(0, 256, (7, 3), dtype=np.uint8)
    T = rng.integers(0, 256, (9, 3), dtype=np.uint8)
    T[6] = T[1]                                          # a tie at different indices
    naive = np.array([[sum(1 for byte in range(3) for c in range(4) if ((int(q[byte]) ^ int(t[byte])) >> (2 * c)) & 3) for t in T] for q in Q])
    assert np.array_equal(H2.distances(Q, T), naive)
    idx, dist = H2.knn(Q, T, 3)
    for i in range(7):
        want = sorted((naive[i, j], j) for j in range(9))[:3]
        assert [(int(d), int(j)) for d, j in zip(dist[i], idx[i])] == want
    idx, dist = H2.knn(Q, T[:1], 2)
    assert (idx[:, 1] == -1).all() and np.isinf(dist[:, 1]).all()
    off, ridx, rdist = H2.radius_match(Q, T, 5.0)
    for i in range(7):
        want = sorted((naive[i, j], j) for j in range(9) if naive[i, j] < 5.0)
        assert [(int(d), int(j)) for d, j in zip(rdist[off[i]:off[i + 1]], ridx[off[i]:off[i + 1]])] == want
    q, t, d, r = H2.mutual_ratio(Q, T, 0.95)
    fq, ft, _, _ = H2.ratio_match(Q, T, 0.95)
    assert set(q) <= set(fq)


# ---- the C-ABI and the header -----------------------------------------------------------------------------------------------
def test_symbols_constants_and_header():
    hdr = _header()
    assert _ffi.FM_BANK_BIN2 == 5 and _ffi.FM_DT_BIN2 == 6
    assert re.search(r"#define\s+FM_BANK_BIN2\s+5\b", hdr) and re.search(r"#define\s+FM_DT_BIN2\s+6\b", hdr)
    assert int(re.search(r"#define\s+FM_ABI_VERSION\s+(\d+)", hdr).group(1)) == 12 and _ffi.FM_ABI_VERSION == 12
    for name in ("FM_BANK_BIN2", "FM_DT_BIN2", "fm_bank_create_bin2"):          # the revision comment names the additions
        assert name in hdr.split("#define FM_ABI_VERSION")[0], name
    res, argtypes = _ffi.SYMBOLS["fm_bank_create_bin2"]
    assert res is ctypes.c_int and argtypes == _ffi.SYMBOLS["fm_bank_create_bin"][1]
    lib = _ffi.load_library()
    assert hasattr(lib, "fm_bank_create_bin2") and lib.fm_abi_version() == 12
    assert callable(_ffi.Context.bank_binary2)
    assert matchutil.NORM_HAMMING2 == 7
    # the pinned "Not built" sentences stay, each with its note; the new section documents the contract
    k11 = hdr.split("int  fm_bank_create_bin")[0].split("Not built:")[-1]
    assert "NORM_HAMMING2" in k11 and "NORM_HAMMING2 has since come" in k11
    fast = hdr.split("---- Hamming Fast-Match")[1].split("int fm_hamming_self_dist")[0].split("Not built:")[1]
    assert "NORM_HAMMING2" in fast and "has since come" in fast and "stays out of Fast-Match" in fast
    coll = hdr.split("typedef struct fm_collection fm_collection;")[0]
    assert "NORM_HAMMING2, radius queries per" in coll and "NORM_HAMMING2 has since come for bank pairs" in coll
    sect = hdr.split("---- K11b: NORM_HAMMING2")[1].split("int fm_bank_create_bin2")[0]
    for text in ("3 P - 4 h2", "tetrahedron", "FM_EUNSUPPORTED", "FM_EINVAL", "fm_hamming_radius_match(_dev)", "fm_mutual_ratio",
                 "lowest index wins a tie", "cellSize = 2"):
        assert text in sect, text


# ---- Python: every refusal before the library is touched -------------------------------------------------------------------
def test_python_refusals_come_before_any_upload(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a refusal touched the device")
    monkeypatch.setattr(matchutil, "_context", no_device)
    monkeypatch.setattr(_ffi, "default_context", no_device)
    a = np.zeros((4, 32), np.uint8)
    calls = [lambda x, y, **o: matchutil.hamming2_match(x, y, k=1, **o),
             lambda x, y, **o: matchutil.hamming2_match_arrays(x, y, k=2, **o),
             lambda x, y, **o: matchutil.hamming2_ratio_match_arrays(x, y, 0.8, **o),
             lambda x, y, **o: matchutil.hamming2_mutual_ratio_match_arrays(x, y, 0.8, **o),
             lambda x, y, **o: matchutil.hamming2_radius_match(x, y, 3.0, **o),
             lambda x, y, **o: matchutil.hamming2_radius_match_arrays(x, y, 3.0, **o)]
    for call in calls:
        for bad in (a.astype(np.float32), a.astype(np.int8), np.zeros(32, np.uint8), np.zeros((4, 65), np.uint8), np.zeros((4, 0), np.uint8)):
            with pytest.raises(ValueError):
                call(bad, a)
            with pytest.raises(ValueError):
                call(a, bad)
        with pytest.raises(ValueError, match="per train row"):
            call(a, np.zeros((4, 16), np.uint8))
        with pytest.raises(ValueError, match="mask"):
            call(a, a, options={"mask": np.ones((4, 4), np.uint8)})
    for k in (0, 9):
        with pytest.raises(ValueError):
            matchutil.hamming2_match(a, a, k=k)
    with pytest.raises(ValueError, match="radii"):
        matchutil.hamming2_radius_match_arrays(a, a, np.ones(3, np.float32))
    m = matchutil.BFMatcher_create(matchutil.NORM_HAMMING2, crossCheck=True)
    assert m.normType == 7 and m.crossCheck
    for call, what in ((lambda: m.add([a]), "collection"), (lambda: m.train(), "collection"),
                       (lambda: m.match(a), "collection"), (lambda: m.knnMatch(a, k=2), "collection"), (lambda: m.knnMatch(a, 2), "collection"),
                       (lambda: m.radiusMatch(a, maxDistance=3.0), "collection"), (lambda: m.radiusMatch(a, 3.0), "collection"),
                       (lambda: m.match(a, a, mask=np.ones((4, 4), np.uint8)), "masks"),
                       (lambda: m.knnMatch(a, a, k=1, mask=np.ones((4, 4), np.uint8)), "masks"),
                       (lambda: m.knnMatch(a, k=1, masks=[None]), "masks"),
                       (lambda: m.radiusMatch(a, a, 3.0, mask=np.ones((4, 4), np.uint8)), "masks")):
        with pytest.raises(ValueError, match=what):
            call()
    # cv2's factory gives today's matcher for the two norms it has served so far
    for norm in (matchutil.NORM_L2, matchutil.NORM_HAMMING):
        assert type(matchutil.BFMatcher_create(norm)) is matchutil.BFMatcher
    assert type(matchutil.BFMatcher_create()) is matchutil.BFMatcher


def test_pinned_normtype_7_refusals_still_hold(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a refusal touched the device")
    monkeypatch.setattr(matchutil, "_context", no_device)
    a = np.zeros((4, 32), np.uint8)
    with pytest.raises(ValueError, match="NORM_HAMMING2"):
        matchutil.bf_match(a, a, k=1, options={"normType": 7})
    with pytest.raises(ValueError):
        matchutil.BFMatcher(normType=7)
    with pytest.raises(ValueError, match="normType"):
        matchutil.mutual_ratio_match_arrays(a, a, 0.8, options={"normType": 7})
    with pytest.raises(ValueError, match="NORM_HAMMING2"):
        matchutil.ratio_match_arrays(a, a, 0.8, options={"normType": 7})


def test_torchmatch_signature():
    import inspect
    from fastmatch_amd import torchmatch
    p = inspect.signature(torchmatch.bank).parameters
    assert p["hamming2"].default is False and p["hamming2"].kind is inspect.Parameter.KEYWORD_ONLY
    assert inspect.signature(torchmatch.Collection.add).parameters["hamming2"].default is False
