"""CPU (hipcc cross-compiles): the registers, scratch and LDS of the product's kernels, as far as the project's own text
states them, read from the amdhsa.kernels metadata of the units compiled with the product's flags.

* filter6_kernel (K12): no scratch, no spills, the static LDS of the source's static_assert.
* "No scratch, no spills"  for every instantiation of K11's sweep and self-distance kernels, K13's masked
  sweep, K8's filter, and K12's rescoring and preparation kernels.
* The row-reduce kernels (K1 / K2) that do spill are accepted as they are today: not more than the table below.
* Registers are held to the occupancy step, not to a number: for a kernel with __launch_bounds__(T, B) the unified
  VGPR + AGPR allocation (granule 8 of a 512-entry file per SIMD lane) must leave room for B workgroups of T threads on
  a CU.  The compiler itself takes B for waves per SIMD, which is less for every workgroup of more than 256 threads, so
  most of these kernels do not meet the workgroup reading today ("Kernel resources under test"): those are
  held to today's register count instead, and all of them to the compiler's reading.

The tables are today's build; a change that moves a kernel past them must edit them on purpose."""
import re

import pytest

import isa_read as R

pytestmark = pytest.mark.skipif(not R.have_hipcc(), reason="no hipcc")

# The build the tables were taken from (the values are ceilings whichever compiler runs the test).
RECORDED_WITH = "AMD clang version 22.0.0git (https://github.com/RadeonOpenCompute/llvm-project roc-7.2.0 26014 7b800a19466229b8479a78de19143dc33c3ab9b5)"

NO_SCRATCH = [("filter6", "filter6_kernel", 1), ("filter6", "rescore6_kernel", 1), ("filter6", "prep6_kernel", 1),
              ("hamming", "ham_sweep_kernel", 8), ("hamming", "ham_self_kernel", 4),       # "in any of the eight / four"
              ("masked", "masked_i8_kernel", 2), ("filter_f16", "filter_kernel", 7)]

# rowreduce.hip, kernels with scratch today: (.vgpr_spill_count, .private_segment_fixed_size in bytes per lane).  The 4 /
# 20 of the <4, 2, ...> forms is the top-2 body DESIGN.md describes; the 16-wave forms of 8 blocks per wave are the
# fallback shapes of banks too small to fill the chip.  Every kernel of the unit that is not listed has neither.
ACCEPTED_SCRATCH = {
    "_ZN2fm22rowreduce_guard_kernelENS_7RRBatchEPKj": (2, 12),
    "_ZN2fm22rowreduce_batch_kernelILi4ELi2ELi8ELi3ELi1ELb0EEEvNS_7RRBatchE": (4, 20),
    "_ZN2fm22rowreduce_table_kernelILi4ELi2ELi8ELi3ELi1EEEvPKNS_8RRParamsEPKii": (4, 20),
    "_ZN2fm16rowreduce_kernelILi4ELi1ELb1ELi4ELi2ELi0ELb1EEEvNS_8RRParamsE": (1, 8),
    "_ZN2fm16rowreduce_kernelILi6ELi1ELb1ELi8ELi3ELi1ELb0EEEvNS_8RRParamsE": (18, 76),
    "_ZN2fm16rowreduce_kernelILi6ELi1ELb1ELi8ELi3ELi0ELb0EEEvNS_8RRParamsE": (18, 76),
    "_ZN2fm16rowreduce_kernelILi6ELi1ELb1ELi8ELi2ELi0ELb0EEEvNS_8RRParamsE": (4, 20),
    "_ZN2fm16rowreduce_kernelILi6ELi1ELb0ELi8ELi2ELi0ELb0EEEvNS_8RRParamsE": (6, 28),
    "_ZN2fm16rowreduce_kernelILi6ELi1ELb1ELi4ELi2ELi0ELb0EEEvNS_8RRParamsE": (13, 56),
    "_ZN2fm16rowreduce_kernelILi6ELi1ELb0ELi4ELi2ELi0ELb0EEEvNS_8RRParamsE": (16, 68),
    "_ZN2fm16rowreduce_kernelILi8ELi1ELb1ELi16ELi2ELi0ELb0EEEvNS_8RRParamsE": (402, 560),
    "_ZN2fm16rowreduce_kernelILi8ELi1ELb0ELi16ELi2ELi0ELb0EEEvNS_8RRParamsE": (409, 568),
    "_ZN2fm16rowreduce_kernelILi6ELi2ELb1ELi8ELi3ELi1ELb0EEEvNS_8RRParamsE": (33, 136),
    "_ZN2fm16rowreduce_kernelILi6ELi2ELb1ELi8ELi3ELi0ELb0EEEvNS_8RRParamsE": (33, 136),
    "_ZN2fm16rowreduce_kernelILi6ELi2ELb1ELi8ELi2ELi0ELb0EEEvNS_8RRParamsE": (47, 120),
    "_ZN2fm16rowreduce_kernelILi6ELi2ELb0ELi8ELi2ELi0ELb0EEEvNS_8RRParamsE": (48, 124),
    "_ZN2fm16rowreduce_kernelILi6ELi2ELb1ELi4ELi2ELi0ELb0EEEvNS_8RRParamsE": (50, 148),
    "_ZN2fm16rowreduce_kernelILi6ELi2ELb0ELi4ELi2ELi0ELb0EEEvNS_8RRParamsE": (69, 160),
    "_ZN2fm16rowreduce_kernelILi8ELi2ELb1ELi16ELi2ELi0ELb0EEEvNS_8RRParamsE": (668, 752),
    "_ZN2fm16rowreduce_kernelILi8ELi2ELb0ELi16ELi2ELi0ELb0EEEvNS_8RRParamsE": (697, 760),
    "_ZN2fm16rowreduce_kernelILi8ELi2ELb1ELi8ELi3ELi1ELb0EEEvNS_8RRParamsE": (12, 52),
    "_ZN2fm16rowreduce_kernelILi8ELi2ELb1ELi8ELi3ELi0ELb0EEEvNS_8RRParamsE": (8, 36),
    "_ZN2fm16rowreduce_kernelILi4ELi2ELb1ELi16ELi2ELi0ELb0EEEvNS_8RRParamsE": (4, 20),
    "_ZN2fm16rowreduce_kernelILi4ELi2ELb0ELi16ELi2ELi0ELb0EEEvNS_8RRParamsE": (4, 20),
    "_ZN2fm16rowreduce_kernelILi4ELi2ELb1ELi8ELi3ELi1ELb0EEEvNS_8RRParamsE": (4, 20),
    "_ZN2fm16rowreduce_kernelILi4ELi2ELb1ELi8ELi3ELi0ELb0EEEvNS_8RRParamsE": (4, 20),
    "_ZN2fm16rowreduce_kernelILi4ELi2ELb0ELi8ELi2ELi0ELb0EEEvNS_8RRParamsE": (6, 28),
    "_ZN2fm16rowreduce_kernelILi4ELi2ELb1ELi4ELi2ELi0ELb0EEEvNS_8RRParamsE": (12, 52),
    "_ZN2fm16rowreduce_kernelILi4ELi2ELb0ELi4ELi2ELi0ELb0EEEvNS_8RRParamsE": (13, 56),
}

# Kernels whose allocation does not leave room for B workgroups of T threads per CU today: .vgpr_count, as a ceiling.
VGPRS_TODAY = {                                                                   # (T, B): what B workgroups would allow
    "_ZN2fm14filter6_kernelENS_7F6BatchE": 172,                                   # (512, 2): 128
    "_ZN2fm13filter_kernelILi4ELi1ELi8ELb1ELb0EEEvNS_7FParamsE": 204,             # (512, 2): 128
    "_ZN2fm13filter_kernelILi4ELi1ELi8ELb0ELb0EEEvNS_7FParamsE": 198,             # (512, 2): 128
    "_ZN2fm13filter_kernelILi4ELi2ELi8ELb0ELb0EEEvNS_7FParamsE": 205,             # (512, 2): 128
    "_ZN2fm13filter_kernelILi4ELi1ELi8ELb1ELb1EEEvNS_7FParamsE": 233,             # (512, 2): 128
    "_ZN2fm16rowreduce_kernelILi4ELi1ELb1ELi8ELi3ELi1ELb1EEEvNS_8RRParamsE": 128,  # (512, 4): 64
    "_ZN2fm16rowreduce_kernelILi4ELi1ELb1ELi8ELi3ELi0ELb1EEEvNS_8RRParamsE": 128,  # (512, 4): 64
    "_ZN2fm16rowreduce_kernelILi4ELi1ELb1ELi8ELi2ELi0ELb1EEEvNS_8RRParamsE": 124,  # (512, 4): 64
    "_ZN2fm16rowreduce_kernelILi4ELi1ELb0ELi8ELi2ELi0ELb1EEEvNS_8RRParamsE": 122,  # (512, 4): 64
    "_ZN2fm16rowreduce_kernelILi6ELi1ELb1ELi8ELi3ELi1ELb0EEEvNS_8RRParamsE": 168,  # (512, 3): 80
    "_ZN2fm16rowreduce_kernelILi6ELi1ELb1ELi8ELi3ELi0ELb0EEEvNS_8RRParamsE": 168,  # (512, 3): 80
    "_ZN2fm16rowreduce_kernelILi6ELi1ELb1ELi8ELi2ELi0ELb0EEEvNS_8RRParamsE": 168,  # (512, 3): 80
    "_ZN2fm16rowreduce_kernelILi6ELi1ELb0ELi8ELi2ELi0ELb0EEEvNS_8RRParamsE": 168,  # (512, 3): 80
    "_ZN2fm16rowreduce_kernelILi8ELi1ELb1ELi16ELi2ELi0ELb0EEEvNS_8RRParamsE": 128,  # (1024, 2): 64
    "_ZN2fm16rowreduce_kernelILi8ELi1ELb0ELi16ELi2ELi0ELb0EEEvNS_8RRParamsE": 128,  # (1024, 2): 64
    "_ZN2fm16rowreduce_kernelILi8ELi1ELb1ELi8ELi3ELi1ELb0EEEvNS_8RRParamsE": 228,  # (512, 2): 128
    "_ZN2fm16rowreduce_kernelILi8ELi1ELb1ELi8ELi3ELi0ELb0EEEvNS_8RRParamsE": 220,  # (512, 2): 128
    "_ZN2fm16rowreduce_kernelILi8ELi1ELb1ELi8ELi2ELi0ELb0EEEvNS_8RRParamsE": 206,  # (512, 2): 128
    "_ZN2fm16rowreduce_kernelILi8ELi1ELb0ELi8ELi2ELi0ELb0EEEvNS_8RRParamsE": 206,  # (512, 2): 128
    "_ZN2fm16rowreduce_kernelILi4ELi1ELb1ELi16ELi2ELi0ELb0EEEvNS_8RRParamsE": 116,  # (1024, 4): 64
    "_ZN2fm16rowreduce_kernelILi4ELi1ELb0ELi16ELi2ELi0ELb0EEEvNS_8RRParamsE": 116,  # (1024, 4): 64
    "_ZN2fm16rowreduce_kernelILi4ELi1ELb1ELi8ELi3ELi1ELb0EEEvNS_8RRParamsE": 126,  # (512, 4): 64
    "_ZN2fm16rowreduce_kernelILi4ELi1ELb1ELi8ELi3ELi0ELb0EEEvNS_8RRParamsE": 126,  # (512, 4): 64
    "_ZN2fm16rowreduce_kernelILi4ELi1ELb1ELi8ELi2ELi0ELb0EEEvNS_8RRParamsE": 120,  # (512, 4): 64
    "_ZN2fm16rowreduce_kernelILi4ELi1ELb0ELi8ELi2ELi0ELb0EEEvNS_8RRParamsE": 123,  # (512, 4): 64
    "_ZN2fm16rowreduce_kernelILi6ELi2ELb1ELi8ELi3ELi1ELb0EEEvNS_8RRParamsE": 168,  # (512, 3): 80
    "_ZN2fm16rowreduce_kernelILi6ELi2ELb1ELi8ELi3ELi0ELb0EEEvNS_8RRParamsE": 168,  # (512, 3): 80
    "_ZN2fm16rowreduce_kernelILi6ELi2ELb1ELi8ELi2ELi0ELb0EEEvNS_8RRParamsE": 168,  # (512, 3): 80
    "_ZN2fm16rowreduce_kernelILi6ELi2ELb0ELi8ELi2ELi0ELb0EEEvNS_8RRParamsE": 168,  # (512, 3): 80
    "_ZN2fm16rowreduce_kernelILi8ELi2ELb1ELi16ELi2ELi0ELb0EEEvNS_8RRParamsE": 128,  # (1024, 2): 64
    "_ZN2fm16rowreduce_kernelILi8ELi2ELb0ELi16ELi2ELi0ELb0EEEvNS_8RRParamsE": 128,  # (1024, 2): 64
    "_ZN2fm16rowreduce_kernelILi8ELi2ELb1ELi8ELi3ELi1ELb0EEEvNS_8RRParamsE": 256,  # (512, 2): 128
    "_ZN2fm16rowreduce_kernelILi8ELi2ELb1ELi8ELi3ELi0ELb0EEEvNS_8RRParamsE": 256,  # (512, 2): 128
    "_ZN2fm16rowreduce_kernelILi8ELi2ELb1ELi8ELi2ELi0ELb0EEEvNS_8RRParamsE": 246,  # (512, 2): 128
    "_ZN2fm16rowreduce_kernelILi8ELi2ELb0ELi8ELi2ELi0ELb0EEEvNS_8RRParamsE": 244,  # (512, 2): 128
    "_ZN2fm16rowreduce_kernelILi4ELi2ELb1ELi16ELi2ELi0ELb0EEEvNS_8RRParamsE": 127,  # (1024, 4): 64
    "_ZN2fm16rowreduce_kernelILi4ELi2ELb0ELi16ELi2ELi0ELb0EEEvNS_8RRParamsE": 127,  # (1024, 4): 64
    "_ZN2fm16rowreduce_kernelILi4ELi2ELb1ELi8ELi3ELi1ELb0EEEvNS_8RRParamsE": 128,  # (512, 4): 64
    "_ZN2fm16rowreduce_kernelILi4ELi2ELb1ELi8ELi3ELi0ELb0EEEvNS_8RRParamsE": 128,  # (512, 4): 64
    "_ZN2fm16rowreduce_kernelILi4ELi2ELb1ELi8ELi2ELi0ELb0EEEvNS_8RRParamsE": 126,  # (512, 4): 64
    "_ZN2fm16rowreduce_kernelILi4ELi2ELb0ELi8ELi2ELi0ELb0EEEvNS_8RRParamsE": 128,  # (512, 4): 64
    "_ZN2fm22rowreduce_batch_kernelILi4ELi1ELi8ELi3ELi1ELb1EEEvNS_7RRBatchE": 128,  # (512, 4): 64
    "_ZN2fm22rowreduce_batch_kernelILi4ELi1ELi8ELi3ELi1ELb0EEEvNS_7RRBatchE": 126,  # (512, 4): 64
    "_ZN2fm22rowreduce_batch_kernelILi4ELi2ELi8ELi3ELi1ELb0EEEvNS_7RRBatchE": 128,  # (512, 4): 64
    "_ZN2fm22rowreduce_guard_kernelENS_7RRBatchEPKj": 127,                         # (512, 4): 64
    "_ZN2fm20rowreduce_tri_kernelILi1EEEvNS_8RRParamsE": 114,                      # (512, 4): 64
    "_ZN2fm26rowreduce_tri_batch_kernelILi1EEEvNS_7RRBatchE": 114,                 # (512, 4): 64
    "_ZN2fm22rowreduce_table_kernelILi4ELi2ELi8ELi3ELi1EEEvPKNS_8RRParamsEPKii": 128,  # (512, 4): 64
}


@pytest.fixture(scope="module")
def meta(tmp_path_factory):
    cache = {}

    def get(unit):
        if unit not in cache:
            cache[unit] = R.metadata(R.isa(unit, tmp_path_factory))
        return cache[unit]
    return get


def instances(md, base):
    return {n: m for n, m in md.items() if re.match(r"_ZN2fm\d+%s(I|E)" % base, n)}


def test_filter6_kernel_is_what_the_source_states(meta):
    (m,) = instances(meta("filter6"), "filter6_kernel").values()
    lds = int(re.search(r"static_assert\(kF6LdsBytes == (\d+)", R.source("filter6")).group(1))
    assert m["private_segment_fixed_size"] == 0
    assert m["vgpr_spill_count"] == 0
    assert m["group_segment_fixed_size"] == lds


@pytest.mark.parametrize("unit,base,count", NO_SCRATCH, ids=[b for _, b, _ in NO_SCRATCH])
def test_no_scratch_no_spills(meta, unit, base, count):
    found = instances(meta(unit), base)
    assert len(found) == count, sorted(found)
    for name, m in found.items():
        assert (m["vgpr_spill_count"], m["private_segment_fixed_size"]) == (0, 0), (name, m)


def test_row_reduce_scratch_is_not_more_than_today(meta):
    md = meta("rowreduce")
    assert set(ACCEPTED_SCRATCH) <= set(md), sorted(set(ACCEPTED_SCRATCH) - set(md))
    for name, m in md.items():
        spills, scratch = ACCEPTED_SCRATCH.get(name, (0, 0))
        assert m["vgpr_spill_count"] <= spills and m["private_segment_fixed_size"] <= scratch, \
            "%s: %d spilled, %d B of scratch; accepted %d, %d (recorded with %s)" % (
                name, m["vgpr_spill_count"], m["private_segment_fixed_size"], spills, scratch, RECORDED_WITH)
    # the top-2 body's 20 bytes, also in the table kernel
    (tab,) = instances(md, "rowreduce_table_kernel").values()
    assert tab["private_segment_fixed_size"] <= 20


# ---- registers against the launch bounds

def vgpr_limit(waves_per_simd):
    """Largest allocation (a multiple of the granule 8) with that many waves resident on a SIMD's 512 registers per lane."""
    return 512 // min(max(waves_per_simd, 1), 8) // 8 * 8


def allocation(m):
    return (m["vgpr_count"] + 7) // 8 * 8                    # (.vgpr_count is the unified count: the AGPRs are in it)


def _top_level(e, chars):
    """Positions of the characters of `chars` in e that stand outside every pair of parentheses."""
    depth, out = 0, []
    for i, ch in enumerate(e):
        depth += (ch == "(") - (ch == ")")
        if ch in chars and depth == 0:
            out.append(i)
    return out


def c_int(expr, env):
    """Value of a C integer expression of literals, names in env, parentheses, arithmetic, comparisons and ?: ."""
    e = expr.strip()
    marks = _top_level(e, "?:")
    if marks:                                                # a ? b : c, right-associative: the ':' that closes the first '?'
        q, open_ = marks[0], 0
        for i in marks[1:]:
            open_ += 1 if e[i] == "?" else -1
            if open_ < 0:
                return c_int(e[q + 1:i], env) if c_int(e[:q], env) else c_int(e[i + 1:], env)
        raise ValueError(expr)
    flat, at = "", 0
    while "(" in e[at:]:                                     # parenthesised groups by their values
        a = e.index("(", at)
        b = a + _top_level(e[a:], ")")[0]                    # (the one that closes it)
        flat += e[at:a] + str(c_int(e[a + 1:b], env))
        at = b + 1
    flat += e[at:]
    return int(eval(flat.replace("/", "//"), {"__builtins__": {}}, dict(env)))


def launch_bounds(unit):
    """{kernel base name: (template parameter names, T expression, B expression)} of the two-argument bounds of a unit."""
    src = R.source(unit)
    out = {}
    for m in re.finditer(r"(?:template <([^>]*)>[^\n]*\n)?__global__ __launch_bounds__\((.*)\)\n(?:static )?void (\w+)\(", src):
        args = m.group(2)
        commas = _top_level(args, ",")
        if not commas:
            continue
        params = [p.split("=")[0].split()[-1] for p in m.group(1).split(",")] if m.group(1) else []
        out[m.group(3)] = (params, args[:commas[0]], args[commas[0] + 1:])
    return out


def bounded_kernels(unit, md):
    """[(name, metadata, T, B)] of the unit's kernels with __launch_bounds__(T, B), the expressions evaluated with the
    instantiation's template arguments (read from the mangled name) and the unit's integer constants."""
    consts = {n: int(v) for n, v in re.findall(r"\b(k[A-Z]\w*) = (\d+)\s*[,;]", R.source(unit))}
    out = []
    for base, (params, t_expr, b_expr) in launch_bounds(unit).items():
        for name, m in instances(md, base).items():
            targs = re.match(r"_ZN2fm\d+%s(?:I((?:L[ib]\d+E)+)E)?" % base, name).group(1) or ""
            env = dict(consts, **dict(zip(params, (int(x) for x in re.findall(r"L[ib](\d+)E", targs)))))
            t, b = c_int(t_expr, env), c_int(b_expr, env)
            assert t == m["max_flat_workgroup_size"], (name, t_expr, t, m)
            out.append((name, m, t, b))
    return out


def test_c_int_reads_the_bounds_expressions():
    assert c_int("64 * NW", {"NW": 8}) == 512
    assert [c_int("(NC >= 8 ? 2 : (NC >= 6 ? 3 : 4))", {"NC": n}) for n in (4, 6, 8)] == [4, 3, 2]
    assert c_int("16 / kN", {"kN": 8}) == 2
    assert [vgpr_limit(w) for w in range(1, 9)] == [512, 256, 168, 128, 96, 80, 72, 64]


@pytest.mark.parametrize("unit,expected", [("filter6", 1), ("filter_f16", 7), ("rowreduce", 57)])
def test_registers_stay_within_the_launch_bounds(meta, unit, expected):
    md = meta(unit)
    kernels = bounded_kernels(unit, md)
    assert len(kernels) == expected, [k[0] for k in kernels]
    for name, m, t, b in kernels:
        waves = (t + 63) // 64
        # the compiler's reading, which it enforces by spilling: B waves per SIMD, and at least one workgroup
        assert allocation(m) <= vgpr_limit(max(b, (waves + 3) // 4)), (name, m["vgpr_count"], t, b)
        # B workgroups of T threads on the CU's four SIMDs
        limit = vgpr_limit((b * waves + 3) // 4)
        if name in VGPRS_TODAY:
            assert m["vgpr_count"] <= VGPRS_TODAY[name], \
                "%s: %d VGPRs, %d when recorded (%d would allow %d workgroups of %d threads per CU)" % (
                    name, m["vgpr_count"], VGPRS_TODAY[name], limit, b, t)
        else:
            assert allocation(m) <= limit, "%s: %d VGPRs allocate %d, but %d workgroups of %d threads per CU need <= %d" % (
                name, m["vgpr_count"], allocation(m), b, t, limit)
    assert not set(n for n in VGPRS_TODAY if n in md) - set(k[0] for k in kernels)
