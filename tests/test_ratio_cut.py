"""Host: the ratio test's distance cut (fast-match_amd/csrc/ratio_cut.h, ratio_cut_d2) against a brute-force scan.

D* must be the smallest integer d2 from which on every d2 fails  (double)sqrtf((float)d2) / sd_max < tau  -- the arithmetic
of xcheck_finalize_kernel -- or "no cut" (0xffffffff) where the header promises none.  A small C++ harness compiles the
header on its own and checks, per (sd_max, tau), every d2 of [0, 2^24 + 2^20) plus a window around D*."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fast-match_amd", "csrc")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)

HARNESS = r"""
#include "ratio_cut.h"
#include <stdio.h>
#include <string.h>
// stdin: lines "<sd_max bits hex> <tau bits hex>"; stdout per line: "<D*> <errors>"
static bool fails(uint32_t d2, double sd, double tau) { return !((double)sqrtf((float)d2) / sd < tau); }
int main()
{
    unsigned long long sb, tb;
    while (scanf("%llx %llx", &sb, &tb) == 2) {
        double sd, tau;
        memcpy(&sd, &sb, 8); memcpy(&tau, &tb, 8);
        const uint32_t D = fm::ratio_cut_d2(sd, tau);
        long errors = 0;
        if (D != fm::kNoRatioCut) {
            // exhaustive below 2^24 + 2^20 (past the float32 image's first rounding step), then around D*
            const uint64_t lim = (1ull << 24) + (1ull << 20);
            for (uint64_t d = 0; d < lim; ++d) errors += fails((uint32_t)d, sd, tau) != (d >= D);
            for (int64_t k = -4096; k <= 4096; ++k) {
                const int64_t d = (int64_t)D + k;
                if (d >= 0 && d <= 0xffffffffll) errors += fails((uint32_t)d, sd, tau) != (d >= (int64_t)D);
            }
            errors += !fails(0xffffffffu, sd, tau);
        } else {
            // "no cut": either it was promised (NaN tau, sd_max NaN / inf / sign bit) or nothing below 2^32 - 1 fails
            const bool promised = tau != tau || sd != sd || signbit(sd) || isinf(sd);
            if (!promised) errors += fails(0xfffffffeu, sd, tau);
        }
        printf("%u %ld\n", D, errors);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if HIPCC is None:
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("ratio_cut")
    src = d / "h.cpp"
    src.write_text(HARNESS)
    exe = d / "h"
    subprocess.check_call([HIPCC, "-O2", "-std=c++17", "-x", "c++", "-I", CSRC, str(src), "-o", str(exe)])
    return str(exe)


def _bits(x):
    return "%016x" % int(np.array([x], np.float64).view(np.uint64)[0])


def _run(exe, cases):
    inp = "".join("%s %s\n" % (_bits(s), _bits(t)) for s, t in cases)
    out = subprocess.run([exe], input=inp, capture_output=True, text=True, check=True).stdout.split("\n")
    res = [tuple(int(v) for v in line.split()) for line in out if line.strip()]
    assert len(res) == len(cases)
    return res


NOCUT = 0xffffffff


def _f32root(d2):
    return float(np.sqrt(np.float32(d2)))


def test_edge_values(harness):
    nan, inf = float("nan"), float("inf")
    cases = [
        (411.0, nan), (nan, 0.7), (inf, 0.7), (-inf, 0.7), (-1.0, 0.7), (-0.0, 0.7), (nan, nan),
        (0.0, 0.7), (0.0, 0.0), (0.0, inf), (0.0, -1.0),
        (411.0, 0.0), (411.0, -0.0), (411.0, -3.0), (411.0, -inf), (411.0, inf),
        (5e-324, 0.7), (2.2250738585072014e-308, 1e300), (1e300, 1e-300), (1.7976931348623157e308, 0.7),
    ]
    res = _run(harness, cases)
    for (s, t), (D, err) in zip(cases, res):
        assert err == 0, (s, t, D)
    expect = {0: NOCUT, 1: NOCUT, 2: NOCUT, 3: NOCUT, 4: NOCUT, 5: NOCUT, 6: NOCUT, 7: 0, 8: 0, 9: 0, 10: 0,
              11: 0, 12: 0, 13: 0, 14: 0, 15: NOCUT}
    for i, want in expect.items():
        assert res[i][0] == want, (cases[i], res[i])


def test_bench_like_values(harness):
    """The flagship's numbers (self distances 400-450, tau 0.7) and a spread of both around them."""
    rng = np.random.default_rng(11)
    cases = [(450.0, 0.7), (411.0, 0.7), (438.0, 0.7), (1.0, 0.7), (3.0, 1.0), (2047.0, 1.0), (100.0, 5.0)]
    cases += [(float(s), float(t)) for s, t in zip(rng.uniform(1, 3000, 40), rng.uniform(0.05, 2.0, 40))]
    for (s, t), (D, err) in zip(cases, _run(harness, cases)):
        assert err == 0 and D != NOCUT, (s, t, D)
    D = _run(harness, [(450.0, 0.7)])[0][0]
    assert _f32root(D - 1) / 450.0 < 0.7 <= _f32root(D) / 450.0


def test_tau_on_a_root(harness):
    """tau exactly equal to a root / sd_max: that d2 fails (strict <), the one below passes."""
    cases = []
    for d2 in [1, 2, 99_225, 175_000, 1_000_000, 4_197_199, 4_197_200, 4_197_201, 8_323_200, 16_777_216, 16_777_217]:
        for sd in [1.0, 411.0, 2048.0, 3.5]:
            cases.append((sd, _f32root(d2) / sd))
    for (s, t), (D, err) in zip(cases, _run(harness, cases)):
        assert err == 0 and D != NOCUT, (s, t, D)
        assert _f32root(D) / s >= t and (D == 0 or _f32root(D - 1) / s < t)


def test_float32_root_tie_range(harness):
    """Cuts inside the range where neighbouring d2 share a float32 root (d2 >= 4 197 200) and past 2^24, where the
    float32 image of d2 itself rounds: D* is the first member of its root class."""
    cases = []
    for d2 in [4_197_200, 4_197_201, 4_200_000, 6_000_001, 8_323_200, 16_777_215, 16_777_216, 16_777_219, 33_554_435,
               1 << 31, 0xfffffff0]:
        for sd in [1.0, 1000.0, 4096.0]:
            r = _f32root(d2) / sd
            cases += [(sd, r), (sd, np.nextafter(r, 0.0)), (sd, np.nextafter(r, np.inf))]
    for (s, t), (D, err) in zip(cases, _run(harness, cases)):
        assert err == 0, (s, t, D)
