"""CPU (hipcc cross-compiles): the schedule of filter6_kernel's stage loop (K12, filter6.hip; DESIGN.md section 4 K12,
"Rotated epilogue"), read off its gfx950 ISA as the product's flags give it.

The loop multiplies a unit in two halves of four matrix instructions and places the max trees and compares of the blocks
tested in a half BETWEEN that half's instructions, where a wave's own vector instructions issue beside its matrix
instruction in flight.  That placement is the scheduler's (sched_group_barrier), so it is held here:

1. every basic block of the loop that holds matrix instructions holds exactly four;
2. between consecutive matrix instructions of a block stand at least 3 and at most 7 vector instructions;
3. no v_max / v_max3 reads an accumulator (a destination register of a matrix instruction) in a block of the loop that
   holds no matrix instruction: no tree was left behind a half.  The hit path, which takes the maximum of acc + start, is
   no such tree: a register the block itself has rewritten (the sum, formed in place) is not an accumulator any more.  The
   drain's tree stands behind the loop;
4. no s_setprio stands inside the loop.

The loop is told by its back edge: the branch behind the last hand-over (s_barrier) to a label in front of the first.  The
checks are functions over isa_read.Kernel; the second half of the file runs them on hand-written snippets, one good and
one broken per rule, without a compiler."""
import re

import pytest

import isa_read as R

needs_hipcc = pytest.mark.skipif(not R.have_hipcc(), reason="no hipcc")
_MFMA = "v_mfma"


def loop_range(k):
    """(first line, last line) of the stage loop: from the target label of the back edge to the back edge."""
    bars = [i for i, l in k.insns if l == "s_barrier"]
    if not bars:
        raise R.IsaError("%s: no s_barrier" % k.name)
    for i, l in k.insns:
        if i > bars[-1] and l.startswith(R._BRANCH):
            t = k.label_line.get(l.split()[1])
            if t is not None and t < bars[0]:
                return t, i
    raise R.IsaError("%s: no branch behind the last s_barrier to a label in front of the first" % k.name)


def basic_blocks(k, lo, hi):
    """The basic blocks of lines lo .. hi: lists of (line, text), cut at labels and behind branches."""
    labels = set(k.label_line.values())
    out, cur = [], []
    text = dict(k.insns)
    for i in range(lo, hi + 1):
        if i in labels and cur:
            out.append(cur)
            cur = []
        l = text.get(i)
        if l is None:
            continue
        cur.append((i, l))
        if l.startswith(R._BRANCH):
            out.append(cur)
            cur = []
    if cur:
        out.append(cur)
    return out


def _is_valu(l):
    return l.startswith("v_") and not l.startswith(_MFMA)


def check_four_per_block(k):
    """Rule 1.  Returns the number of blocks with matrix instructions."""
    n = 0
    for b in basic_blocks(k, *loop_range(k)):
        m = [i for i, l in b if l.startswith(_MFMA)]
        if m and len(m) != 4:
            raise R.IsaError("%s: the basic block at line %d holds %d matrix instructions, a half has 4" % (k.name, b[0][0], len(m)))
        n += 1 if m else 0
    if n == 0:
        raise R.IsaError("%s: no matrix instruction in the loop" % k.name)
    return n


def check_gaps(k, least=3, most=7):
    """Rule 2.  Returns the (smallest, largest) gap."""
    gaps = []
    for b in basic_blocks(k, *loop_range(k)):
        at = [n for n, (_, l) in enumerate(b) if l.startswith(_MFMA)]
        for a, z in zip(at, at[1:]):
            g = sum(1 for _, l in b[a + 1:z] if _is_valu(l))
            if not least <= g <= most:
                raise R.IsaError("%s: %d vector instructions between the matrix instructions at lines %d and %d, not %d .. %d"
                                 % (k.name, g, b[a][0], b[z][0], least, most))
            gaps.append(g)
    if not gaps:
        raise R.IsaError("%s: no two matrix instructions in one block of the loop" % k.name)
    return min(gaps), max(gaps)


def check_no_tree_behind(k):
    """Rule 3.  Returns the number of accumulator registers."""
    acc = set()
    for _, l in k.insns:
        if l.startswith(_MFMA):
            acc |= R._regs(R.operands(l).split(",")[0])
    for b in basic_blocks(k, *loop_range(k)):
        if any(l.startswith(_MFMA) for _, l in b):
            continue
        rewritten = set()                                # (the hit path forms acc + start in place: no accumulator any more)
        for i, l in b:
            if l.startswith(("v_max3_f32", "v_max_f32")):
                hit = sorted(R._regs(R.operands(l).split(",", 1)[1]) & acc - rewritten)
                if hit:
                    raise R.IsaError("%s: `%s` (line %d) reads the accumulator v%d in a block without matrix instructions"
                                     % (k.name, l, i, hit[0]))
            if l.startswith(("v_", "ds_read")) and "," in l:
                rewritten |= R._regs(R.operands(l).split(",")[0])
    return len(acc)


def check_no_setprio(k):
    """Rule 4."""
    lo, hi = loop_range(k)
    bad = [(i, l) for i, l in k.between(lo, hi) if l.startswith("s_setprio")]
    if bad:
        raise R.IsaError("%s: `%s` (line %d) inside the stage loop" % (k.name, bad[0][1], bad[0][0]))
    return True


# ---------------------------------------------------------------------------------------------------------------------
# the product

@pytest.fixture(scope="module")
def k(tmp_path_factory):
    return R.kernel(R.isa("filter6", tmp_path_factory), "filter6_kernel")


@needs_hipcc
def test_loop_is_found(k):
    lo, hi = loop_range(k)
    bars = [i for i, l in k.insns if l == "s_barrier"]
    assert len(bars) == 3 and lo < bars[0] and bars[-1] < hi


@needs_hipcc
def test_every_half_is_a_block_of_four(k):
    units = int(re.search(r"constexpr int kF6Units = kStageRows / kTileRows;\s*// 32-row units per stage: (\d+)", R.source("filter6")).group(1))
    # three stage bodies, `units` multiplies each, two halves a multiply
    assert check_four_per_block(k) == 3 * units * 2


@needs_hipcc
def test_trees_stand_between_the_matrix_instructions(k):
    lo, hi = check_gaps(k)
    assert 3 <= lo <= hi <= 7


@needs_hipcc
def test_no_tree_behind_a_half(k):
    assert check_no_tree_behind(k) >= 64


@needs_hipcc
def test_no_priority_flip_in_the_loop(k):
    assert check_no_setprio(k)


# ---------------------------------------------------------------------------------------------------------------------
# the checks themselves, on hand-written code

def _tree(regs, dst):
    return "\n".join("\tv_max3_f32 v%d, v%d, v%d, v%d" % (dst + n, r, r + 1, r + 2) for n, r in enumerate(regs))


def _half(acc_dst, a, tree_from, n_between=(4, 4, 4), label=None):
    """Four matrix instructions on v[acc_dst ..] and v[acc_dst + 16 ..] with n_between[g] v_max3 on v[tree_from ..] between."""
    out = [label + ":"] if label else []
    for g in range(4):
        d = acc_dst + 16 * (g & 1)
        c = "0" if g < 2 else "v[%d:%d]" % (d, d + 15)
        out.append("\tv_mfma_f32_32x32x64_f8f6f4 v[%d:%d], v[%d:%d], v[200:205], %s cbsz:2 blgp:2" % (d, d + 15, a, a + 5, c))
        if g < 3:
            out.append(_tree([tree_from + 3 * n for n in range(n_between[g])], 190))
    out.append("\tv_cmp_ge_f32_e32 vcc, v190, v180")
    out.append("\ts_cmp_eq_u64 vcc, 0")
    return "\n".join(o for o in out if o)


def _sample(half1, half2, between="", hit=""):
    return """
_ZN2fm6sampleEv:                        ; @_ZN2fm6sampleEv
; %%bb.0:
	s_load_dwordx4 s[4:7], s[0:1], 0x0
.LBB0_1:                                ; =>This Inner Loop Header: Depth=1
	;;#ASMSTART
	s_waitcnt vmcnt(2)
	;;#ASMEND
	;;#ASMSTART
	s_waitcnt lgkmcnt(0)
	s_barrier
	;;#ASMEND
	s_waitcnt lgkmcnt(0)
%s
	s_cbranch_scc1 .LBB0_3
; %%bb.2:
%s
.LBB0_3:
%s
%s
	s_cbranch_scc1 .LBB0_5
; %%bb.4:
	v_add_f32_e32 v191, v0, v170
.LBB0_5:
	s_add_i32 s7, s7, 1
	s_cmp_lt_i32 s7, s6
	s_cbranch_scc1 .LBB0_1
; %%bb.6:
	v_max3_f32 v190, v32, v33, v34
	s_endpgm
.Lfunc_end0:
""" % (half1, hit or "\tv_add_f32_e32 v191, v32, v170", between, half2)


def _k(text):
    return R.kernel(text, "sample")


GOOD = _sample(_half(0, 210, 32), _half(32, 210, 0))


def test_good_sample_passes_every_check():
    k = _k(GOOD)
    lo, hi = loop_range(k)
    assert k.lines[lo].startswith(".LBB0_1") and k.lines[hi].startswith("s_cbranch_scc1 .LBB0_1")
    assert check_four_per_block(k) == 2
    assert check_gaps(k) == (4, 4)
    assert check_no_tree_behind(k) == 64          # (the tree behind the loop, the drain's, is outside the range)
    assert check_no_setprio(k)


def test_a_burst_of_eight_is_rejected():
    # the two halves in one block: the shape of a loop that multiplies a whole unit and tests it behind
    both = _half(0, 210, 32) + "\n" + _half(32, 210, 0)
    with pytest.raises(R.IsaError, match="holds 8 matrix instructions"):
        check_four_per_block(_k(_sample(both, _half(32, 216, 0))))


def test_a_bare_pair_and_a_crowded_gap_are_rejected():
    with pytest.raises(R.IsaError, match="2 vector instructions between"):
        check_gaps(_k(_sample(_half(0, 210, 32, (4, 2, 4)), _half(32, 210, 0))))
    with pytest.raises(R.IsaError, match="8 vector instructions between"):
        check_gaps(_k(_sample(_half(0, 210, 32), _half(32, 210, 0, (4, 4, 8)))))
    assert check_gaps(_k(_sample(_half(0, 210, 32, (3, 7, 5)), _half(32, 210, 0)))) == (3, 7)


def test_a_tree_left_behind_a_half_is_rejected():
    # a block of its own between the halves (behind a label: the hit path's join) that reduces accumulators 32 ..
    left = "\tv_max3_f32 v190, v32, v33, v34\n\ts_cmp_eq_u64 vcc, 0\n\ts_cbranch_scc1 .LBB0_7\n.LBB0_7:"
    with pytest.raises(R.IsaError, match="reads the accumulator v32 in a block without matrix instructions"):
        check_no_tree_behind(_k(_sample(_half(0, 210, 32), _half(32, 210, 0), between=left)))
    # the hit path's maximum over acc + start reads sums, not accumulators
    hit = "\tv_add_f32_e32 v32, v32, v170\n\tv_add_f32_e32 v192, v33, v171\n\tv_max3_f32 v190, v32, v191, v192"
    assert check_no_tree_behind(_k(_sample(_half(0, 210, 32), _half(32, 210, 0), hit=hit))) == 64


def test_a_priority_flip_in_the_loop_is_rejected():
    with pytest.raises(R.IsaError, match="s_setprio 2"):
        check_no_setprio(_k(_sample("\ts_setprio 2\n" + _half(0, 210, 32), _half(32, 210, 0))))
    # in front of the loop (the static form) it is outside the range
    assert check_no_setprio(_k(GOOD.replace(".LBB0_1:   ", "\ts_setprio 1\n.LBB0_1:   ", 1)))
