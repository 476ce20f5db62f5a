"""Host: the FP6 sweep's screen threshold (fp6_screen_threshold, fast-match_amd/csrc/fp6_filter.h), compiled on its own.

filter6_kernel's accumulators start at zero; a block is screened against  thr_s = thr - smax  (smax: the largest accumulator
start of the streamed stage) and only a block that passes reads its rows' starts and repeats the test exactly.  The screen
may lose nothing, so thr_s has to be rounded DOWN: here it is checked against exact rational arithmetic for thresholds over
the whole value range (negative ones, kF6Never) and every kind of smax (0, step multiples down to the lowest start there
is, kFp6PadInit), and "exact test passes => screen passes" is run on accumulators that sit on and next to the threshold.
The device computes the same value with the hardware's round-down subtraction (the helper's other branch), which the GPU
tests reach; what is pinned here is the value both must produce."""
import os
import shutil
import subprocess
from fractions import Fraction

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
// "consts": the bits of kF6Never and kFp6PadInit.  "<file>": uint32 n, then n x (float thr, float smax); per pair one line
// with the bits of fp6_screen_threshold(thr, smax).
int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    if (!strcmp(argv[1], "consts")) {
        const float a = fm::kF6Never, b = fm::kFp6PadInit;
        unsigned ab, bb;
        memcpy(&ab, &a, 4); memcpy(&bb, &b, 4);
        printf("%u %u\n", ab, bb);
        return 0;
    }
    FILE* f = fopen(argv[1], "rb");
    unsigned n;
    if (!f || fread(&n, 4, 1, f) != 1) return 2;
    float* v = (float*)malloc((size_t)n * 8 + 8);
    if (fread(v, 8, n, f) != n) return 2;
    for (unsigned i = 0; i < n; ++i) {
        const float t = fm::fp6_screen_threshold(v[2 * i], v[2 * i + 1]);
        unsigned tb;
        memcpy(&tb, &t, 4);
        printf("%u\n", tb);
    }
    return 0;
}
"""

STEP = 1.0 / 64.0
ACC_MAX = 460800          # steps: 128 products of at most 3600
START_MIN = -260100       # steps: -floor(128 x 255^2 / 32)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if HIPCC is None:
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("fp6s")
    src = d / "h.cpp"
    src.write_text(HARNESS)
    exe = d / "h"
    subprocess.check_call([HIPCC, "-O2", "-std=c++17", "-x", "c++", "-I", CSRC, str(src), "-o", str(exe)])
    return str(exe)


@pytest.fixture(scope="module")
def consts(harness):
    out = subprocess.run([harness, "consts"], capture_output=True, text=True, check=True).stdout.split()
    never, pad = np.array(out, np.uint32).view(np.float32)
    assert never == np.float32(3.0e38) and pad == np.float32(-3.4e38)
    return never, pad


def _screen(exe, tmp_path, thr, smax):
    thr, smax = np.asarray(thr, np.float32), np.asarray(smax, np.float32)
    blob = np.stack([thr, smax], axis=1).astype(np.float32)
    path = tmp_path / "pairs.bin"
    with open(path, "wb") as f:
        f.write(np.array([len(blob)], np.uint32).tobytes())
        f.write(blob.tobytes())
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, check=True).stdout.split()
    return np.array(out, np.uint32).view(np.float32)


def _thresholds(rng, never):
    """Thresholds as fp6_threshold_acc can return them (|T_c| / 1024 below 2^22, any fraction) and beyond: zeros, the
    smallest and largest magnitudes, values whose difference with a step multiple is not a float32, kF6Never."""
    t = [0.0, -0.0, 1e-45, -1e-45, 1e-38, -1e-38, 2.0 ** -30, -2.0 ** -30, 1.0 / 3.0, -1.0 / 3.0, 48.4140625, -48.4140625,
         4064.0625, -4064.0625, 4064.06256103515625, 7200.0, -2097152.0, 2097151.75, -4194303.5, 4194303.5, 16777216.0,
         -16777216.0, 3.0e30, -3.0e30, float(never)]
    t += list(rng.uniform(-100.0, 100.0, 40)) + list(rng.uniform(-4.2e6, 4.2e6, 40))
    t += list((rng.integers(-ACC_MAX, ACC_MAX, 40) + rng.uniform(-0.5, 0.5, 40)) * STEP)
    bits = rng.integers(0, 1 << 32, 200, dtype=np.uint64).astype(np.uint32).view(np.float32)       # any finite float32
    t += list(bits[np.isfinite(bits) & (np.abs(bits) < 3.0e38)])
    return np.array(t, np.float32)


def _smaxes(rng, pad):
    s = [0.0, -STEP, -2 * STEP, -127.984375, -3753.21875, START_MIN * STEP, float(pad)]
    s += list(rng.integers(START_MIN, 1, 40) * STEP)
    return np.array(s, np.float32)


def test_rounded_down_and_never_nan(harness, consts, tmp_path):
    """Every threshold against every smax: thr_s is a number, finite unless thr - smax lies below every finite float32 (it
    cannot here), thr_s <= thr - smax in exact arithmetic, and the next float32 up is above the difference (the LARGEST such
    value: the screen is as sharp as the format allows) unless the difference is beyond the largest finite float32.  The
    round-to-nearest difference breaks the first property on these very cases, so they do see the rounding direction."""
    never, pad = consts
    rng = np.random.default_rng(11)
    T, S = _thresholds(rng, never), _smaxes(rng, pad)
    thr, smax = np.repeat(T, len(S)), np.tile(S, len(T))
    got = _screen(harness, tmp_path, thr, smax)
    assert not np.isnan(got).any() and np.isfinite(got).all()
    fmax = float(np.finfo(np.float32).max)
    nearest_too_high = 0
    for t, s, g in zip(thr.tolist(), smax.tolist(), got.tolist()):
        exact = Fraction(t) - Fraction(s)
        assert Fraction(g) <= exact, (t, s, g)
        with np.errstate(over="ignore"):
            up = float(np.nextafter(np.float32(g), np.float32(np.inf)))
            near = np.float32(t) - np.float32(s)
        assert g == fmax and exact >= Fraction(fmax) or Fraction(up) > exact, (t, s, g)
        nearest_too_high += bool(np.isinf(near) or Fraction(float(near)) > exact)
    print("%d of %d pairs: the round-to-nearest difference is above thr - smax" % (nearest_too_high, len(thr)))
    assert nearest_too_high > len(thr) // 20
    # kF6Never against a stage of padding rows: the one sum beyond the format -- it stays the largest finite float32
    assert _screen(harness, tmp_path, [never], [pad])[0] == np.float32(fmax)
    # an output row beyond the bank is never reached by an accumulator, whatever the stage
    assert (_screen(harness, tmp_path, np.full(len(S), never), S) > np.float32(ACC_MAX * STEP)).all()


def test_exact_test_passes_implies_screen_passes(harness, consts, tmp_path):
    """Accumulators are step multiples 0 .. 460 800 steps, starts step multiples -260 100 .. 0 steps with start <= smax (or
    kFp6PadInit: a padding row, which nothing keeps).  For random accumulators and for the adversarial ones -- the smallest
    step multiple with acc + start >= thr, its two neighbours, for the row that attains smax and for rows below it -- a
    lane that passes  acc + start >= thr  (exact: float64 holds the sum) passes  acc >= thr_s."""
    never, pad = consts
    rng = np.random.default_rng(12)
    n = 4000
    smax_steps = np.concatenate([rng.integers(START_MIN, 1, n - 200), np.zeros(100, np.int64), np.full(100, START_MIN)])
    below = np.where(rng.random(n) < 0.5, 0, rng.integers(0, 3000, n))           # the row's start: smax or below it
    start_steps = np.maximum(smax_steps - below, START_MIN)
    thr = np.concatenate([rng.uniform(-100.0, 100.0, n // 2), rng.uniform(-4200.0, 7300.0, n - n // 2)]).astype(np.float32)
    thr[::97] = np.float32(0.0)
    thr[1::97] = (rng.integers(-6400, 6400, len(thr[1::97])) * STEP).astype(np.float32)        # thresholds ON a step
    thr_s = _screen(harness, tmp_path, thr, (smax_steps * STEP).astype(np.float32))
    # the smallest accumulator (in steps) that passes the exact test, clamped to what an accumulator can be
    first = np.ceil(thr.astype(np.float64) * 64.0).astype(np.int64) - start_steps
    checked = passed = 0
    for d in (-1, 0, 1, 2, 64, None):
        acc_steps = np.clip(first + d, 0, ACC_MAX) if d is not None else rng.integers(0, ACC_MAX + 1, n)
        acc = (acc_steps * STEP).astype(np.float32)
        assert np.array_equal(acc.astype(np.float64) * 64.0, acc_steps)                        # exact in float32
        exact_pass = (acc_steps + start_steps) * STEP >= thr.astype(np.float64)
        screen_pass = acc >= thr_s
        assert not (exact_pass & ~screen_pass).any(), d
        checked += n
        passed += int(exact_pass.sum())
    assert passed > checked // 4 and passed < checked
    # padding rows: acc + kFp6PadInit is below every threshold a real output row has, screen or no screen
    assert (np.float32(ACC_MAX * STEP) + pad < thr).all()
    # a stage of padding rows only: thr_s is beyond every accumulator
    assert (_screen(harness, tmp_path, thr, np.full(n, pad)) > np.float32(ACC_MAX * STEP)).all()
