"""Host: the FP6 filter's code table, error bound and threshold (fast-match_amd/csrc/fp6_filter.h), compiled on its own.

The filter may lose nothing: for an output row c and any streamed row m of a bank, |c.m - c^.m^| <= E_c, and every pair at
d2 <= D* - 1 passes  acc >= T_c / 1024  in the arithmetic of the kernel (accumulator = c^.m^ / 1024 + start value, exact in
float32).  The harness computes all of it with the header's own functions; numpy recomputes the table and the dot products."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fast-match_amd", "csrc")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)

HARNESS = r"""
#include "fp6_filter.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
// "table": 256 lines "<code> <32 x value>".
// "pairs <file>": the file holds uint32 n, uint32 D*, then n x (128 bytes c, 128 bytes m); the streamed bank is ALL the m rows.
// "edge <file>": uint32 n, then n x (uint32 D*, int32 largest |m|^2, int32 largest |m - m^|^2 of the streamed bank), then the
// n row pairs: every pair has its own cut and its own streamed bank; a negative maximum stands for the one over all m rows.
// Per pair one line "<dot> <dot of the images> <E_c, rounded up to an integer> <keeps> <acc steps> <threshold bits>", and
// under "edge" five more: the threshold in steps, E_c as the header returns it, the threshold in steps with the streamed
// bank's maxima replaced by the OUTPUT row's own |c|^2 and |c - c^|^2, the accumulator in steps had the start value
// been rounded up (-ceil(|m|^2 / 32) steps), and the threshold in steps with |c|^2 and |c^|^2 exchanged.
int main(int argc, char** argv)
{
    if (argc > 1 && !strcmp(argv[1], "table")) {
        for (int v = 0; v < 256; ++v) printf("%d %d\n", fm::fp6_code(v), fm::fp6_value32(fm::fp6_code(v)));
        return 0;
    }
    if (argc < 3) return 2;
    const bool edge = !strcmp(argv[1], "edge");
    FILE* f = fopen(argv[2], "rb");
    unsigned n, D = 0;
    if (!f || fread(&n, 4, 1, f) != 1 || (!edge && fread(&D, 4, 1, f) != 1)) return 2;
    int* own = (int*)malloc((size_t)n * 12 + 12);
    if (edge && fread(own, 12, n, f) != n) return 2;
    unsigned char* buf = (unsigned char*)malloc((size_t)n * 256);
    if (fread(buf, 256, n, f) != n) return 2;
    int um = 0, em = 0;
    for (unsigned i = 0; i < n; ++i) {
        const unsigned char* m = buf + 256 * (size_t)i + 128;
        int u = 0, e = 0;
        for (int k = 0; k < 128; ++k) { const int x = fm::fp6_value32(fm::fp6_code(m[k])); u += m[k] * m[k]; e += (m[k] - x) * (m[k] - x); }
        um = u > um ? u : um; em = e > em ? e : em;
    }
    for (unsigned i = 0; i < n; ++i) {
        const unsigned char* c = buf + 256 * (size_t)i;
        const unsigned char* m = c + 128;
        long dot = 0, hdot = 0;
        int cu = 0, ch = 0, ce = 0, mu = 0;
        for (int k = 0; k < 128; ++k) {
            const int xc = fm::fp6_value32(fm::fp6_code(c[k])), xm = fm::fp6_value32(fm::fp6_code(m[k]));
            dot += c[k] * m[k]; hdot += xc * xm;
            cu += c[k] * c[k]; ch += xc * xc; ce += (c[k] - xc) * (c[k] - xc); mu += m[k] * m[k];
        }
        // the kernel's accumulator: products of the e2m3 values (multiples of 1/64) on the start value, in float32
        float acc = fm::fp6_acc_init(mu);
        for (int k = 0; k < 128; ++k)
            acc += (float)fm::fp6_value32(fm::fp6_code(c[k])) * (1.0f / 32.0f) * ((float)fm::fp6_value32(fm::fp6_code(m[k])) * (1.0f / 32.0f));
        const unsigned d = edge ? (unsigned)own[3 * i] : D;
        const int u1 = edge && own[3 * i + 1] >= 0 ? own[3 * i + 1] : um, e1 = edge && own[3 * i + 2] >= 0 ? own[3 * i + 2] : em;
        const float thr = fm::fp6_threshold_acc(fm::fp6_threshold(cu, ch, ce, u1, e1, d));
        unsigned tb;
        memcpy(&tb, &thr, 4);
        printf("%ld %ld %.0f %d %.0f %u", dot, hdot, ceil(fm::fp6_error_bound(ch, ce, u1, e1)), acc >= thr ? 1 : 0, (double)acc * 64.0, tb);
        if (edge) {
            const float swapped = fm::fp6_threshold_acc(fm::fp6_threshold(cu, ch, ce, cu, ce, d));
            const float columns = fm::fp6_threshold_acc(fm::fp6_threshold(ch, cu, ce, u1, e1, d));
            printf(" %.17g %.17g %.17g %.0f %.17g", (double)thr * 64.0, fm::fp6_error_bound(ch, ce, u1, e1), (double)swapped * 64.0,
                   (double)acc * 64.0 + (double)(mu >> 5) - (double)((mu + 31) >> 5), (double)columns * 64.0);
        }
        printf("\n");
    }
    return 0;
}
"""

GRID = np.array(list(range(0, 64, 4)) + list(range(64, 128, 8)) + list(range(128, 256, 16)), np.int64)     # 32 x the e2m3 magnitudes


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if HIPCC is None:
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("fp6")
    src = d / "h.cpp"
    src.write_text(HARNESS)
    exe = d / "h"
    subprocess.check_call([HIPCC, "-O2", "-std=c++17", "-x", "c++", "-I", CSRC, str(src), "-o", str(exe)])
    return str(exe)


def _table(exe):
    out = subprocess.run([exe, "table"], capture_output=True, text=True, check=True).stdout.split()
    t = np.array(out, np.int64).reshape(256, 2)
    return t[:, 0], t[:, 1]


def test_code_table(harness):
    """All 256 codes: the nearest grid value (numpy), the code <-> value map of e2m3, and the round-trip error per range."""
    code, val = _table(harness)
    assert len(GRID) == 32 and GRID[-1] == 240
    v = np.arange(256)
    want = GRID[np.argmin(np.abs(GRID[None, :] - v[:, None]), axis=1)]          # (the lower value of two equally near)
    assert np.array_equal(val, want)
    # e2m3: exponent bits 4:3 (bias 1), mantissa bits 2:0, subnormals at exponent 0
    e, m = code >> 3, code & 7
    dec = np.where(e == 0, m / 8.0, (1 + m / 8.0) * 2.0 ** (e - 1))
    assert np.array_equal(dec * 32, val) and code.min() == 0 and code.max() == 31
    err = np.abs(val - v)
    assert err[:63].max() <= 2 and err[63:125].max() <= 4 and err[125:241].max() <= 8 and err[241:].max() <= 15
    assert np.array_equal(val[241:], np.full(15, 240))


def _run_pairs(exe, tmp_path, C, M, D):
    n = len(C)
    blob = np.empty((n, 256), np.uint8)
    blob[:, :128], blob[:, 128:] = C, M
    path = tmp_path / "pairs.bin"
    with open(path, "wb") as f:
        f.write(np.array([n, D], np.uint32).tobytes())
        f.write(blob.tobytes())
    out = subprocess.run([exe, "pairs", str(path)], capture_output=True, text=True, check=True).stdout.split()
    return np.array(out, np.float64).reshape(n, 6)


def _adversarial():
    rows = [np.full(128, 255), np.zeros(128), np.arange(128) % 15 + 241]
    rows += [np.full(128, b) for b in (62, 66, 126, 130)]
    for k in (0, 31, 32, 127):
        for b in (255, 1, 62):
            r = np.zeros(128)
            r[k] = b
            rows.append(r)
    rows = np.array(rows, np.uint8)
    i, j = np.meshgrid(np.arange(len(rows)), np.arange(len(rows)))
    return rows[i.ravel()], rows[j.ravel()]


@pytest.mark.parametrize("D", [315 * 315, 1, 2_000_000, 0xfffffffe])
def test_error_bound_and_threshold(harness, tmp_path, D):
    """200 random row pairs (SIFT-like, uniform, and near copies at distances around the cut) plus every pair of the
    adversarial rows: the dot-product error stays within E_c, the float32 accumulator is the exact number of steps, and no
    pair at d2 <= D* - 1 fails the threshold."""
    from fastmatch_amd import synth
    rng = np.random.default_rng(5)
    Q, T, _ = synth.planted_pair(70, 70, seed=9, p=0.5, sigma=6.0)
    U = rng.integers(0, 256, (60, 128)).astype(np.uint8)
    near = np.clip(Q.astype(np.int64) + rng.integers(-30, 31, Q.shape), 0, 255).astype(np.uint8)
    C = np.concatenate([Q, U, Q])
    M = np.concatenate([T, U[::-1], near])
    assert len(C) == 200
    aC, aM = _adversarial()
    C, M = np.concatenate([C, aC]), np.concatenate([M, aM])
    res = _run_pairs(harness, tmp_path, C, M, D)
    c, m = C.astype(np.int64), M.astype(np.int64)
    dot = (c * m).sum(1)
    code, val = _table(harness)
    hdot = (val[C] * val[M]).sum(1)
    assert np.array_equal(res[:, 0], dot) and np.array_equal(res[:, 1], hdot)
    assert (np.abs(dot - hdot) <= res[:, 2]).all()
    # accumulator: hdot / 1024 - floor(|m|^2 / 32) / 64 in steps of 1/64, exact
    steps = hdot // 16 - (m * m).sum(1) // 32
    assert (hdot % 16 == 0).all() and np.array_equal(res[:, 4], steps) and np.abs(steps).max() < 1 << 24
    d2 = ((c - m) ** 2).sum(1)
    must = d2 <= D - 1
    assert must.any() or D == 1
    assert (res[must, 3] == 1).all(), (D, d2[must & (res[:, 3] == 0)])


def _run_edge(exe, tmp_path, C, M, D, um=None, em=None):
    """Every pair against its own cut D[i]; the streamed bank's maxima per pair (um[i], em[i]), or those of all M rows."""
    n = len(C)
    own = np.full((n, 3), -1, np.int64)
    own[:, 0] = D
    if um is not None:
        own[:, 1], own[:, 2] = um, em
    blob = np.empty((n, 256), np.uint8)
    blob[:, :128], blob[:, 128:] = C, M
    path = tmp_path / "edge.bin"
    with open(path, "wb") as f:
        f.write(np.array([n], np.uint32).tobytes())
        f.write(own.astype(np.int32).view(np.uint32).tobytes())
        f.write(blob.tobytes())
    out = subprocess.run([exe, "edge", str(path)], capture_output=True, text=True, check=True).stdout.split()
    return np.array(out, np.float64).reshape(n, 11)


# bytes halfway between two grid values (the table rounds them down), and 241 .. 255, which clamp to 240
HALFWAY = list(range(2, 64, 4)) + list(range(68, 128, 8)) + list(range(136, 240, 16)) + list(range(241, 256))
# (c, m) of the six constant pairs measured first, and whether the threshold with the OUTPUT row's maxima still keeps them
TABLE = [(136, 152, False), (136, 168, False), (200, 232, False), (136, 255, False), (36, 255, False), (255, 36, True)]


def _own_bank(exe, tmp_path, C, M):
    """The pairs, each against D* = d2 + 1 with m alone as the streamed bank: (result rows, d2)."""
    C, M = np.asarray(C, np.uint8), np.asarray(M, np.uint8)
    _, val = _table(exe)
    c, m = C.astype(np.int64), M.astype(np.int64)
    d2 = ((c - m) ** 2).sum(1)
    return _run_edge(exe, tmp_path, C, M, d2 + 1, (m * m).sum(1), ((m - val[M]) ** 2).sum(1)), d2


def test_constant_rows_on_the_threshold(harness, tmp_path):
    """Cauchy-Schwarz is an equality for constant rows: (c - c^) || m and c^ || (m - m^), and with bytes that round DOWN both
    terms of c.m - c^.m^ are positive, so the dot product loses exactly E_c.  Every constant row of a halfway byte (4k + 2
    below 64, 8k + 4 below 128, 16k + 8 below 240) or of a clamped one (241 .. 255), and 36 of the first table, against every
    other one, each pair at its own cut D* = d2 + 1 with m alone as the streamed bank: 2 162 pairs.
    - every pair is kept, |c.m - c^.m^| <= E_c and E_c - |c.m - c^.m^| < 1 unit;
    - 0 <= acc - threshold <= 2 steps of 1/64.  The slack is E_c's safety terms (2^-20 E_c + 2^-10 < 1.5 units, E_c < 2^20),
      the floor of T_c (< 1 unit), the float32 rounding of T_c / 1024 (< 1 unit: T_c / 1024 < 4096, half an ulp is 2^-13) and
      the floor of the start value (< 16 units; 0 here, |m|^2 = 128 b^2 is a multiple of 32): under 20 units = 1.25 steps.
      MEASURED: 1/16 step (one unit) for every one of the pairs;
    - sharpness: the threshold recomputed with the maxima of the OUTPUT row (|c|^2, |c - c^|^2) in place of the streamed
      bank's -- what a prologue reading the wrong bank's max6 would compute -- is higher for 1 129 of the pairs, and every one
      of those FAILS it (E_c is a multiple of 128 here, so a higher threshold is at least 8 steps higher).  Of the first table's
      six pairs that loses all but 255 against 36, where the swap loosens the threshold."""
    rows = sorted(set(HALFWAY + [36]))
    assert len(HALFWAY) == 46
    C = np.array([np.full(128, a) for a in rows for b in rows if a != b], np.uint8)
    M = np.array([np.full(128, b) for a in rows for b in rows if a != b], np.uint8)
    res, d2 = _own_bank(harness, tmp_path, C, M)
    c, m = C.astype(np.int64), M.astype(np.int64)
    _, val = _table(harness)
    dot, hdot = (c * m).sum(1), (val[C] * val[M]).sum(1)
    assert np.array_equal(res[:, 0], dot) and np.array_equal(res[:, 1], hdot)
    assert (res[:, 3] == 1).all()
    lost = dot - hdot
    assert (lost >= 0).all() and (lost <= res[:, 7]).all() and (res[:, 7] - lost < 1).all()
    assert np.array_equal(res[:, 4], hdot // 16 - (m * m).sum(1) // 32) and ((m * m).sum(1) % 32 == 0).all()
    gap = res[:, 4] - res[:, 6]
    print("gap in steps: min %r max %r" % (gap.min(), gap.max()))
    assert (gap >= 0).all() and (gap <= 2).all()
    higher = res[:, 8] > res[:, 6]
    print("%d of %d pairs have a higher threshold under the output row's maxima" % (higher.sum(), len(higher)))
    assert higher.sum() > len(higher) // 3 and (res[higher, 4] < res[higher, 8]).all()
    for a, b, survives in TABLE:
        i = np.nonzero((C[:, 0] == a) & (M[:, 0] == b))[0][0]
        assert (res[i, 4] >= res[i, 8]) == survives and higher[i] == (not survives), (a, b)
    assert d2[(C[:, 0] == 136) & (M[:, 0] == 152)][0] == 32768 and d2[(C[:, 0] == 36) & (M[:, 0] == 255)][0] == 6139008


# (c byte, m byte, {index: byte} edits of m): one per value range of m, |m|^2 no multiple of 32
OFF32 = [(2, 6, {5: 4, 77: 5}), (68, 76, {5: 75}), (2, 152, {5: 150}), (36, 255, {5: 254})]


@pytest.mark.parametrize("a,b,edit", OFF32)
def test_start_value_rounds_down(harness, tmp_path, a, b, edit):
    """A constant row's |m|^2 = 128 b^2 is a multiple of 32, where floor and ceil of |m|^2 / 32 agree.  One or two bytes of m
    moved make it none, at the price of a little slack in Cauchy-Schwarz.  A short search over one- and two-byte edits by up
    to 3 found in every value range of m a pair that stays within ONE step of its threshold, so the start value rounded up,
    -ceil(|m|^2 / 32) steps, loses it: this pins the rounding direction of fp6_acc_init.  MEASURED gaps, in steps:
      c = 2,  m = 6 with m[5] = 4, m[77] = 5      2/16   (|m|^2 mod 32 = 1)
      c = 68, m = 76 with m[5] = 75              13/16   (9)
      c = 2,  m = 152 with m[5] = 150             3/16   (4)
      c = 36, m = 255 with m[5] = 254             3/16   (3)
    (The edit named first, m = 152 with one byte at 151 against c = 136, measures 17/16 steps: kept either way.)"""
    m = np.full(128, b)
    for k, v in edit.items():
        m[k] = v
    assert (m.astype(np.int64) ** 2).sum() % 32 != 0
    res, _ = _own_bank(harness, tmp_path, [np.full(128, a)], [m])
    gap, up = res[0, 4] - res[0, 6], res[0, 9] - res[0, 6]
    print("gap %r steps; with the start value rounded up %r" % (gap, up))
    assert res[0, 3] == 1 and 0 <= gap < 1
    assert res[0, 9] == res[0, 4] - 1 and up < 0


def test_a_row_that_rounds_up_pins_the_stat6_columns(harness, tmp_path):
    """For a row whose bytes round DOWN, |c|^2 >= |c^|^2 >= |c - c^|^2 and every permutation of the three stat6 columns
    LOWERS the threshold: |c|^2 / 2 only shrinks, and sqrt(a) max||m|| + sqrt(b) max||m - m^|| is least with the smaller of
    a, b against the larger maximum.  The constant families above cannot see such a mix-up.  A row that rounds UP has
    |c^|^2 > |c|^2: 233 (image 240) against 36 (a grid value: no error on the streamed side) at D* = d2 + 1 clears its
    threshold by 2 (c^ - c) m = 64 512 units, and |c^|^2 in the place of |c|^2 raises the threshold by
    (|c^|^2 - |c|^2) / 2 = 211 904 units: the pair must be kept, and must fail that threshold.  MEASURED: 4 032 steps above the
    true threshold, 9 212 steps below the other one."""
    res, d2 = _own_bank(harness, tmp_path, [np.full(128, 233)], [np.full(128, 36)])
    assert d2[0] == 128 * 197 ** 2 and res[0, 3] == 1
    gap, other = res[0, 4] - res[0, 6], res[0, 4] - res[0, 10]
    print("gap %r steps; against the threshold with |c|^2 and |c^|^2 exchanged %r" % (gap, other))
    assert 0 <= gap <= (2 * 7 * 36 * 128) / 16 + 2 and other < 0
