"""Host: the FP6 filter's split rule (fast-match_amd/csrc/fp6_plan.h), compiled on its own.

One stage count L per workgroup for a whole launch, minimising  ceil(sum_i chunks_i * ceil(stages_i / L) / R) * (L + P)  over
8 <= L <= the largest stage count, ties to the larger L; pair i then gets K1's normalisation of ceil(stages_i / L) splits.
The harness prints what the header chooses; Python recomputes the minimum by trying every L."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fast-match_amd", "csrc")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)

HARNESS = r"""
#include "fp6_plan.h"
#include <stdio.h>
#include <stdlib.h>
// "rule R P chunks stages [chunks stages ...]": one line "<L> <workgroups at L> <rounds at L>", then per pair
// "<nsplit> <stages per split>".
// "forced stages n": "<nsplit> <stages per split>" of a forced count.
int main(int argc, char** argv)
{
    if (argc == 4 && argv[1][0] == 'f') {
        int ns, per;
        fm::fp6_plan_split_forced(atoi(argv[2]), atoi(argv[3]), &ns, &per);
        printf("%d %d\n", ns, per);
        return 0;
    }
    if (argc < 6 || (argc - 4) % 2) return 2;
    const int R = atoi(argv[2]);
    const double P = atof(argv[3]);
    const int n = (argc - 4) / 2;
    fm::Fp6PlanPair* p = (fm::Fp6PlanPair*)malloc(sizeof(fm::Fp6PlanPair) * n);
    for (int i = 0; i < n; ++i) p[i] = fm::Fp6PlanPair{atoi(argv[4 + 2 * i]), atoi(argv[5 + 2 * i])};
    const int L = fm::fp6_plan_stages(p, n, R, P);
    printf("%d %lld %lld\n", L, (long long)fm::fp6_plan_workgroups(p, n, L), (long long)fm::fp6_plan_rounds(p, n, R, L));
    for (int i = 0; i < n; ++i) {
        int ns, per;
        fm::fp6_plan_split(p[i].stages, L, &ns, &per);
        printf("%d %d\n", ns, per);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or HIPCC
    if cxx is None:
        pytest.skip("no host compiler")
    d = tmp_path_factory.mktemp("fp6_plan")
    src, exe = d / "plan.cpp", d / "plan"
    src.write_text(HARNESS)
    cmd = [cxx, "-O1", "-std=c++17", "-I", CSRC, str(src), "-o", str(exe)]
    if cxx == HIPCC:
        cmd[1:1] = ["-x", "c++"]
    subprocess.check_call(cmd)
    return str(exe)


def _ceil(a, b):
    return -(-a // b)


def _rule(exe, pairs, R=256, P=1.5):
    args = [exe, "rule", str(R), repr(P)] + [str(v) for pr in pairs for v in pr]
    lines = subprocess.check_output(args, text=True).split("\n")
    L, wg, rounds = (int(v) for v in lines[0].split())
    return L, wg, rounds, [tuple(int(v) for v in ln.split()) for ln in lines[1:1 + len(pairs)]]


def _brute(pairs, R=256, P=1.5):
    """(L, cost) of the minimum over every L, the larger L on ties.  Costs are multiples of 1/2 far below 2^53: exact."""
    best = None
    for L in range(8, max(8, max(s for _, s in pairs)) + 1):
        wg = sum(c * _ceil(s, L) for c, s in pairs)
        cost = _ceil(wg, R) * (L + P)
        if best is None or cost <= best[1]:
            best = (L, cost)
    return best


def _check_cover(pairs, L, splits):
    for (_, stages), (ns, per) in zip(pairs, splits):
        if L is not None:           # the rule's normalisation of ceil(stages / L) splits
            n0 = _ceil(stages, L)
            assert per == _ceil(stages, n0) and ns == _ceil(stages, per), (stages, L, ns, per)
            if stages < 8:
                assert ns == 1
        # split f sweeps stages [f per, min((f + 1) per, stages)): every stage once, no split empty
        seen = [0] * stages
        for f in range(ns):
            lo, hi = f * per, min((f + 1) * per, stages)
            assert lo < hi
            for st in range(lo, hi):
                seen[st] += 1
        assert seen == [1] * stages


def test_bench_batch(harness):
    """12 pairs of 100 000 x 100 000 rows: 98 filter chunks, 782 stages each.  5 splits of 157 stages in 23 rounds of 256
    workgroups (3 645.5 stage-times; K1's 13 splits of 61 are 60 rounds, 3 750)."""
    pairs = [(98, 782)] * 12
    L, wg, rounds, splits = _rule(harness, pairs)
    assert (L, wg, rounds) == (157, 12 * 98 * 5, 23)
    assert splits == [(5, 157)] * 12
    assert _brute(pairs) == (157, 23 * 158.5)
    _check_cover(pairs, L, splits)


CASES = {
    "one_pair": [(98, 782)],
    "64_small": [(13, 98)] * 64,
    "mixed": [(98, 782), (13, 98), (1, 9), (2, 9), (40, 313), (7, 1000), (1, 3), (3, 8)],
    "three_stages": [(1, 3)],
    "below_and_above_8": [(5, 7), (5, 17)],
    "large": [(1000, 20000), (3, 12345)],
}


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("R,P", [(256, 1.5), (304, 1.5), (7, 0.5)])
def test_minimum_matches_brute_force(harness, name, R, P):
    pairs = CASES[name]
    L, wg, rounds, splits = _rule(harness, pairs, R, P)
    bl, bcost = _brute(pairs, R, P)
    assert wg == sum(c * _ceil(s, L) for c, s in pairs) and rounds == _ceil(wg, R)
    assert rounds * (L + P) == bcost, (L, bl)
    assert L == bl
    assert 8 <= L <= max(8, max(s for _, s in pairs))
    _check_cover(pairs, L, splits)
    # the launch's grid is sum of chunks x splits: at most the workgroups at L, and an int
    grid = sum(c * ns for (c, _), (ns, _) in zip(pairs, splits))
    assert grid <= wg < 2 ** 31


def test_totals_stay_below_2_31(harness):
    """16 pairs at the largest sizes an int holds: 2^21 chunks x 2^24 stages.  At L = 8 the sum is 2^49; the rule's own choice
    must come out as a number a grid can carry, and nothing may wrap on the way."""
    pairs = [(1 << 21, 1 << 24)] * 16
    L, wg, rounds, splits = _rule(harness, pairs)
    assert wg == sum(c * _ceil(s, L) for c, s in pairs)
    assert rounds == _ceil(wg, 256)
    assert wg < 2 ** 31
    _check_cover([(1, 1 << 12)], 100, [(41, 100)])          # (the cover check itself, on a case with a short last split)


@pytest.mark.parametrize("stages,force", [(9, 1), (9, 2), (9, 3), (9, 4), (9, 5), (9, 9), (9, 12), (782, 5), (782, 13), (12, 3), (3, 2)])
def test_forced_count_is_k1s(harness, stages, force):
    ns, per = (int(v) for v in subprocess.check_output([harness, "forced", str(stages), str(force)], text=True).split())
    f = min(force, stages)
    assert per == _ceil(stages, f) and ns == _ceil(stages, per)
    _check_cover([(1, stages)], None, [(ns, per)])
