"""Host: the match graph's chunker (fast-match_amd/csrc/pairs_plan.h), compiled on its own.

Consecutive pairs share a chunk until the next pair would take it over the byte budget, over 2^31 - 1 workgroups, merge blocks
or join blocks, over 2^24 slots or over 2^30 - 1 wide rows; a chunk holds at least one pair; a single pair over the workgroup
or the wide-row limit is refused with its index.  The harness prints the header's chunks; Python restates the greedy rule and
checks the chunks' properties from prefix sums.  The same harness built with -fsanitize=address,undefined must print the same
and report nothing."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fast-match_amd", "csrc")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)

GRID, SLOTS, WROWS = 2 ** 31 - 1, 2 ** 24, 2 ** 30 - 1
FIELDS = ("part", "bound", "fix", "wg", "mblocks", "jblocks", "ra", "rb", "wrows")

HARNESS = r"""
#include "pairs_plan.h"
#include <stdio.h>
#include <stdlib.h>
// <file> <budget> <ndir>.  The file: one run per line, "<repeat> part bound fix wg mblocks jblocks ra rb wrows".
// Prints "refused <pair> <status>", or per chunk "p0 p1 nslots wg mblocks jblocks entries lists wrows part bound fix work".
int main(int argc, char** argv)
{
    if (argc != 4) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    std::vector<fm::PairsCost> run;
    std::vector<size_t> reps;
    size_t n = 0;
    long long rep;
    unsigned long long v[9];
    while (fscanf(f, "%lld %llu %llu %llu %llu %llu %llu %llu %llu %llu", &rep, v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6, v + 7, v + 8) == 10) {
        fm::PairsCost c;
        c.part = (size_t)v[0]; c.bound = (size_t)v[1]; c.fix = (size_t)v[2];
        c.wg = (int64_t)v[3]; c.mblocks = (int64_t)v[4]; c.jblocks = (int64_t)v[5];
        c.ra = (int64_t)v[6]; c.rb = (int64_t)v[7]; c.wrows = (int64_t)v[8];
        run.push_back(c); reps.push_back((size_t)rep); n += (size_t)rep;
    }
    fclose(f);
    std::vector<fm::PairsCost> cost;
    cost.reserve(n);
    for (size_t i = 0; i < run.size(); ++i) cost.insert(cost.end(), reps[i], run[i]);
    std::vector<fm::PairsSpan> out;
    int64_t bad = -1;
    const fm::PairsPlanStatus st = fm::pairs_plan(cost.data(), (int64_t)cost.size(), (size_t)strtoull(argv[2], nullptr, 10), atoi(argv[3]), &out, &bad);
    if (st != fm::kPairsPlanOk) { printf("refused %lld %d\n", (long long)bad, (int)st); return 0; }
    for (const fm::PairsSpan& s : out)
        printf("%lld %lld %d %lld %lld %lld %lld %lld %lld %llu %llu %llu %.17g\n", (long long)s.p0, (long long)s.p1, s.nslots, (long long)s.wg,
               (long long)s.mblocks, (long long)s.jblocks, (long long)s.entries, (long long)s.lists, (long long)s.wrows,
               (unsigned long long)s.part, (unsigned long long)s.bound, (unsigned long long)s.fix, s.work);
    return 0;
}
"""


def _compile(d, name, extra):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or HIPCC
    if cxx is None:
        pytest.skip("no host compiler")
    src, exe = d / (name + ".cpp"), d / name
    src.write_text(HARNESS)
    cmd = [cxx, "-O1", "-std=c++17"] + extra + ["-I", CSRC, str(src), "-o", str(exe)]
    if cxx == HIPCC:
        cmd[1:1] = ["-x", "c++"]
    subprocess.check_call(cmd)
    return str(exe)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("pairs_plan"), "plan", [])


@pytest.fixture(scope="module")
def harness_san(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("pairs_plan_san"), "plan_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def pair(ra, rb, part=0, bound=0, fix=0, wg=0, mblocks=None, jblocks=None, wrows=0):
    """One pair's cost as the routes fill it in: all zero when a side is empty."""
    if ra == 0 or rb == 0:
        return dict.fromkeys(FIELDS, 0)
    return dict(part=part, bound=bound, fix=fix, wg=wg, mblocks=-(-ra // 256) - (-rb // 256) if mblocks is None else mblocks,
                jblocks=-(-ra // 256) if jblocks is None else jblocks, ra=ra, rb=rb, wrows=wrows)


def _run(exe, tmp_path, runs, budget, ndir=2):
    """runs: [(repeat, cost)].  The harness's output: ("refused", pair, status) or the list of chunk tuples."""
    f = tmp_path / "costs.txt"
    f.write_text("".join("%d %s\n" % (rep, " ".join(str(c[k]) for k in FIELDS)) for rep, c in runs))
    out = subprocess.check_output([exe, str(f), str(budget), str(ndir)], text=True, stderr=subprocess.STDOUT)
    lines = out.split("\n")
    if lines[0].startswith("refused"):
        _, p, st = lines[0].split()
        return ("refused", int(p), int(st))
    return [tuple(float(v) if i == 12 else int(v) for i, v in enumerate(ln.split())) for ln in lines if ln]


def _bytes(c):
    live = c["ra"] > 0 and c["rb"] > 0
    return c["part"] + c["bound"] + c["fix"] + (c["ra"] + c["rb"]) * 16 + c["ra"] * 17 + c["jblocks"] * 12 if live else 0


def _greedy(costs, budget, ndir):
    """The rule, restated: chunks as (p0, p1, nslots, wg, mblocks, jblocks, entries, lists, wrows, part, bound, fix)."""
    chunks, z = [], dict(p0=0, used=0, nslots=0, wg=0, mblocks=0, jblocks=0, entries=0, lists=0, wrows=0, part=0, bound=0, fix=0)
    ch = dict(z)

    def close(p1):
        chunks.append((ch["p0"], p1) + tuple(ch[k] for k in ("nslots", "wg", "mblocks", "jblocks", "entries", "lists", "wrows", "part", "bound", "fix")))
    for p, c in enumerate(costs):
        need = _bytes(c)
        if ch["p0"] < p and (ch["used"] + need > budget or ch["wg"] + c["wg"] > GRID or ch["jblocks"] + c["jblocks"] > GRID or
                             ch["mblocks"] + c["mblocks"] > GRID or ch["nslots"] + 2 > SLOTS or ch["wrows"] + c["wrows"] > WROWS):
            close(p)
            ch = dict(z, p0=p)
        if c["wg"] > GRID:
            return ("refused", p, 1)
        if c["wrows"] > WROWS:
            return ("refused", p, 2)
        ch["used"] += need
        if c["ra"] > 0 and c["rb"] > 0:
            ch["nslots"] += ndir
            ch["entries"] += 0 if ndir == 1 else c["ra"]
            ch["lists"] += c["ra"] if ndir == 1 else c["ra"] + c["rb"]
            for k in ("wg", "mblocks", "jblocks", "wrows", "part", "bound", "fix"):
                ch[k] += c[k]
    close(len(costs))
    return chunks


def _check_properties(runs, budget, ndir, chunks):
    """What must hold of any correct chunking, from prefix sums (exact: every sum is far below 2^63)."""
    reps = np.array([r for r, _ in runs], dtype=np.int64)
    col = {k: np.repeat(np.array([c[k] for _, c in runs], dtype=np.int64), reps) for k in FIELDS}
    n = int(reps.sum())
    live = (col["ra"] > 0) & (col["rb"] > 0)
    for k in FIELDS:                    # (a pair with an empty side contributes nothing)
        assert not col[k][~live].any()
    col["bytes"] = np.where(live, col["part"] + col["bound"] + col["fix"] + (col["ra"] + col["rb"]) * 16 + col["ra"] * 17 + col["jblocks"] * 12, 0)
    col["nslots"] = np.where(live, ndir, 0)
    col["entries"] = np.where(live, 0 if ndir == 1 else col["ra"], 0)
    col["lists"] = np.where(live, col["ra"] if ndir == 1 else col["ra"] + col["rb"], 0)
    pre = {k: np.concatenate(([0], np.cumsum(v))) for k, v in col.items()}

    def total(k, p0, p1):
        return int(pre[k][p1] - pre[k][p0])
    # consecutive, non-empty, a partition of [0, n)
    assert chunks[0][0] == 0 and chunks[-1][1] == n
    for a, b in zip(chunks, chunks[1:]):
        assert a[1] == b[0]
    for ch in chunks:
        p0, p1 = ch[0], ch[1]
        assert p0 < p1
        # the sums are the sums of the chunk's pairs
        names = ("nslots", "wg", "mblocks", "jblocks", "entries", "lists", "wrows", "part", "bound", "fix")
        assert tuple(ch[2:12]) == tuple(total(k, p0, p1) for k in names), (p0, p1)
        work = float(ndir) * float(np.sum(col["ra"][p0:p1].astype(np.float64) * col["rb"][p0:p1].astype(np.float64) * live[p0:p1]))
        assert abs(ch[12] - work) <= 1e-9 * max(work, 1.0)
        # over the budget only alone; never over an integer limit
        assert total("bytes", p0, p1) <= budget or p1 - p0 == 1
        assert ch[3] <= GRID and ch[4] <= GRID and ch[5] <= GRID and ch[2] <= SLOTS and ch[8] <= WROWS
        # the greedy maximum: the pair behind the chunk would have broken the budget or a limit
        if p1 < n:
            assert (total("bytes", p0, p1 + 1) > budget or ch[3] + col["wg"][p1] > GRID or ch[5] + col["jblocks"][p1] > GRID or
                    ch[4] + col["mblocks"][p1] > GRID or ch[2] + 2 > SLOTS or ch[8] + col["wrows"][p1] > WROWS), (p0, p1)


def _expand(runs):
    return [c for rep, c in runs for _ in range(rep)]


def _random_runs(rng, n, route):
    runs = []
    for _ in range(n):
        ra, rb = (int(rng.integers(0, 3000)) if rng.random() > 0.1 else 0 for _ in range(2))
        if route == "i8":
            c = pair(ra, rb, part=256 * int(rng.integers(1, 400)), bound=256 * int(rng.integers(0, 40)), fix=256 * int(rng.integers(0, 50)),
                     wg=int(rng.integers(2, 60)))
        elif route == "wide":
            pr = -(-ra // 128) * 128 + -(-rb // 128) * 128
            c = pair(ra, rb, part=pr * 16, bound=pr * 4, fix=(ra + rb) * 256 * 12, wg=pr // 128, wrows=pr)
        else:
            c = pair(ra, rb)
        runs.append((1, c))
    return runs


@pytest.mark.parametrize("route", ["i8", "wide", "pairwise"])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_costs_follow_the_greedy_rule(harness, tmp_path, route, seed):
    rng = np.random.default_rng(seed)
    runs = _random_runs(rng, 300, route)
    one = max(_bytes(c) for _, c in runs)
    for budget in (1, one // 2, one, 3 * one + 17, 40 * one, 1 << 40):
        got = _run(harness, tmp_path, runs, budget)
        assert [c[:12] for c in got] == _greedy(_expand(runs), budget, 2)
        _check_properties(runs, budget, 2, got)


def test_forward_lists_alone_have_no_entries(harness, tmp_path):
    """ndir = 1 (fm_collection_wide_knn2_each): one slot per live pair, lists of rows(a), no per-row entries, no join blocks."""
    rng = np.random.default_rng(5)
    runs = []
    for _ in range(200):
        ra, rb = 700, int(rng.integers(0, 2000)) if rng.random() > 0.2 else 0
        runs.append((1, pair(ra, rb, part=768 * 16, bound=768 * 4, fix=ra * 256 * 12, wg=6, mblocks=3, jblocks=0, wrows=768)))
    for budget in (1, 5_000_000, 1 << 40):
        got = _run(harness, tmp_path, runs, budget, 1)
        assert [c[:12] for c in got] == _greedy(_expand(runs), budget, 1)
        _check_properties(runs, budget, 1, got)
        assert all(c[6] == 0 and c[5] == 0 for c in got)


def test_pairs_with_an_empty_side(harness, tmp_path):
    """They cost nothing and own no slot; behind a chunk that is over the budget on its own they start the next one, as
    every pair does, and a chunk of empty pairs alone is served (no slots, no blocks)."""
    live, dead = pair(1000, 900, part=4096, wg=8), pair(0, 900)
    runs = [(3, dead), (1, live), (2, dead), (2, live), (1, dead)]
    one = _bytes(live)
    for budget in (one - 1, one, 2 * one, 1 << 30):
        got = _run(harness, tmp_path, runs, budget)
        assert [c[:12] for c in got] == _greedy(_expand(runs), budget, 2)
        _check_properties(runs, budget, 2, got)
    got = _run(harness, tmp_path, [(5, dead)], 1 << 30)
    assert [c[:12] for c in got] == [(0, 5) + (0,) * 10]
    # one byte short: the pair alone is over the budget, the empty pairs in front of it stay in a chunk without slots
    got = _run(harness, tmp_path, runs, one - 1)
    assert got[0][:3] == (0, 3, 0) and got[1][:3] == (3, 4, 2)


def test_budget_equal_to_the_sum_and_one_byte_short(harness, tmp_path):
    c = pair(500, 400, part=8192, bound=512, fix=2304, wg=4)
    runs = [(7, c)]
    total = 7 * _bytes(c)
    got = _run(harness, tmp_path, runs, total)
    assert [(g[0], g[1]) for g in got] == [(0, 7)]
    got = _run(harness, tmp_path, runs, total - 1)
    assert [(g[0], g[1]) for g in got] == [(0, 6), (6, 7)]
    _check_properties(runs, total - 1, 2, got)


def test_workgroup_limit_reached_exactly(harness, tmp_path):
    """2^31 - 1 workgroups fit one chunk; one more closes it; a single pair of 2^31 is refused with its index."""
    half, rest = pair(10, 10, wg=2 ** 30), pair(10, 10, wg=2 ** 30 - 1)
    got = _run(harness, tmp_path, [(1, half), (1, rest), (1, pair(10, 10, wg=1))], 1 << 40)
    assert [(g[0], g[1], g[3]) for g in got] == [(0, 2, GRID), (2, 3, 1)]
    got = _run(harness, tmp_path, [(2, half)], 1 << 40)
    assert [(g[0], g[1]) for g in got] == [(0, 1), (1, 2)]
    runs = [(1, half), (1, pair(0, 5)), (1, pair(10, 10, wg=2 ** 31))]
    assert _run(harness, tmp_path, runs, 1 << 40) == ("refused", 2, 1) == _greedy(_expand(runs), 1 << 40, 2)
    # the same limit on the merge's and the join's blocks
    for k in ("mblocks", "jblocks"):
        runs = [(1, pair(10, 10, **{k: 2 ** 30})), (1, pair(10, 10, **{k: 2 ** 30 - 1})), (1, pair(10, 10, **{k: 1}))]
        got = _run(harness, tmp_path, runs, 1 << 40)
        assert [(g[0], g[1]) for g in got] == [(0, 2), (2, 3)]
        _check_properties(runs, 1 << 40, 2, got)


def test_slot_count_crosses_2_24(harness, harness_san, tmp_path):
    """2^23 - 1 pairs leave the chunk at 2^24 - 2 slots: the next pair's two slots reach the limit exactly and stay, the one
    after it would cross it."""
    c = pair(1, 1)                      # two slots, two merge blocks, one join block, one entry, two list entries

    def span(p0, p1):
        m = p1 - p0
        return (p0, p1, 2 * m, 0, 2 * m, m, m, 2 * m, 0, 0, 0, 0, 2.0 * m)
    for exe in (harness, harness_san):
        assert _run(exe, tmp_path, [(2 ** 23 + 2, c)], 1 << 62) == [span(0, 2 ** 23), span(2 ** 23, 2 ** 23 + 2)]
    assert _run(harness, tmp_path, [(2 ** 23 - 1, c)], 1 << 62) == [span(0, 2 ** 23 - 1)]
    assert span(0, 2 ** 23 - 1)[2] == SLOTS - 2 and span(0, 2 ** 23)[2] == SLOTS


def test_wide_rows_at_the_limit(harness, tmp_path):
    """2^30 - 1 rows of a wide chunk's output-row space fit, one more closes the chunk; a single pair of 2^30 is refused."""
    a, b = pair(10, 10, wrows=2 ** 29), pair(10, 10, wrows=2 ** 29 - 1)
    runs = [(1, a), (1, b), (1, pair(10, 10, wrows=1)), (1, a), (1, a)]
    got = _run(harness, tmp_path, runs, 1 << 40)
    assert [(g[0], g[1], g[8]) for g in got] == [(0, 2, WROWS), (2, 4, 2 ** 29 + 1), (4, 5, 2 ** 29)]
    _check_properties(runs, 1 << 40, 2, got)
    runs = [(1, a), (1, pair(10, 10, wrows=2 ** 30))]
    assert _run(harness, tmp_path, runs, 1 << 40) == ("refused", 1, 2) == _greedy(_expand(runs), 1 << 40, 2)
    # over both limits: the workgroups are named first
    assert _run(harness, tmp_path, [(1, pair(10, 10, wg=2 ** 31, wrows=2 ** 30))], 1 << 40) == ("refused", 0, 1)


def test_same_chunks_under_the_sanitizers(harness, harness_san, tmp_path):
    """Every input shape above once more through the -fsanitize=address,undefined build: the same lines, no report (a report
    ends the harness with a non-zero status)."""
    rng = np.random.default_rng(11)
    cases = [(_random_runs(rng, 200, r), b, 2) for r in ("i8", "wide", "pairwise") for b in (1, 100_000, 10_000_000, 1 << 40)]
    cases.append(([(3, pair(0, 9)), (1, pair(1000, 900, part=4096, wg=8)), (2, pair(7, 0))], 100, 2))
    cases.append(([(1, pair(10, 10, wg=2 ** 30)), (1, pair(10, 10, wg=2 ** 30 - 1)), (1, pair(10, 10, wg=1))], 1 << 40, 2))
    cases.append(([(1, pair(10, 10, wg=2 ** 31))], 1 << 40, 2))
    cases.append(([(1, pair(10, 10, wrows=2 ** 29)), (1, pair(10, 10, wrows=2 ** 29 - 1)), (1, pair(10, 10, wrows=2 ** 30))], 1 << 40, 1))
    c = pair(500, 400, part=8192, bound=512, fix=2304, wg=4)
    cases.append(([(7, c)], 7 * _bytes(c), 2))
    cases.append(([(7, c)], 7 * _bytes(c) - 1, 2))
    for runs, budget, ndir in cases:
        assert _run(harness_san, tmp_path, runs, budget, ndir) == _run(harness, tmp_path, runs, budget, ndir)
