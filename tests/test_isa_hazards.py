"""CPU (hipcc cross-compiles): the three-buffer row-reduce kernels load their shared bounds with an
inline-asm global_load whose completion the COMPILER does not track (rowreduce.hip, load_bound_untracked:
its own wait would also drain the newest LDS-DMA).  The hand-written s_waitcnt vmcnt(k) at the next stage
hand-over covers the load only if nothing touches the destination VGPR in between -- a copy, a spill or a
re-allocation inserted by a future compiler would read or clobber a value that has not landed.  This test
reads the generated ISA and checks exactly that, for every kernel that uses the construct."""
import re

import pytest

from isa_read import _regs, have_hipcc, isa as _isa, kernels as _kernels


@pytest.mark.skipif(not have_hipcc(), reason="no hipcc")
@pytest.mark.parametrize("unit", ["rowreduce", "filter_f16"])
def test_lds_dma_through_inline_asm_sets_m0_itself(unit, tmp_path_factory):
    """The LDS-DMA helpers written as inline asm (rowreduce.hip lds_dma_16 / lds_dma_4, filter_f16.hip f_lds_dma_16) load M0
    inside the asm statement.  M0 is a reserved register to the compiler -- it is not accepted in a clobber list (ADVICE
    r05) -- so the compiler does not know the statement changes it.  That is safe exactly as long as (a) every such
    instruction has its own s_mov_b32 m0 in front of it in the SAME statement and (b) no kernel that uses the asm form also
    holds a compiler-generated user of M0 (the builtin's global_load_lds, whose M0 set-up the compiler may hoist or reuse
    across our statements).  This reads the generated ISA and checks both, kernel by kernel."""
    text = _isa(unit, tmp_path_factory)
    asm_kernels = 0
    for k in _kernels(text, first_exit=True):
        name = k.name
        block_of = {i: b for b in k.blocks for i, _ in b.insns}
        asm_form, compiler_form = 0, 0
        for i, l in k.insns:
            in_asm = i in k.in_asm
            block = [t for j, t in block_of[i].insns if j <= i] if in_asm else []     # the statement up to this instruction
            if l.startswith("global_load_lds_dword"):
                if in_asm:
                    asm_form += 1
                    assert len(block) >= 3 and block[-3].startswith("s_mov_b32 m0,") and block[-2].startswith("s_nop"), (name, block)
                else:
                    compiler_form += 1
            elif not in_asm and re.search(r"\bm0\b", l) and asm_form + compiler_form >= 0 and not l.startswith("s_mov_b32 m0"):
                # any other reader of M0 the compiler emitted (s_movrel, ds_gws, sendmsg ...) next to the asm form
                compiler_form += 1 if "global_load_lds" not in l else 0
        if asm_form:
            asm_kernels += 1
            assert compiler_form == 0, "%s mixes the inline-asm LDS-DMA with %d compiler-generated users of M0" % (name, compiler_form)
    assert asm_kernels >= 3


@pytest.mark.skipif(not have_hipcc(), reason="no hipcc")
def test_untracked_bound_loads_are_not_touched_before_their_wait(tmp_path_factory):
    text = _isa("rowreduce", tmp_path_factory)
    checked = 0
    for k in _kernels(text, first_exit=True):
        name = k.name
        if "sc1" not in k.text:
            continue
        lines, insns = k.lines, k.insns
        # (only the inline-asm loads: the compiler tracks its own relaxed atomic loads, which look the same)
        loads = [(n, i, l) for n, (i, l) in enumerate(insns)
                 if re.match(r"global_load_dword v\d+, .*\bsc1\b", l) and i > 0 and "ASMSTART" in lines[i - 1]]
        if not loads:
            continue
        # the hand-over waits are the explicit ones: inside an ASMSTART / ASMEND pair
        waits = [n for n, (i, l) in enumerate(insns) if l.startswith("s_waitcnt vmcnt(") and i > 0 and "ASMSTART" in lines[i - 1]]
        assert waits, name
        # loop: the label in front of the first hand-over wait, and the last branch back to it
        label_line = k.label_line
        first_wait_line = insns[waits[0]][0]
        header = max((i, name_) for name_, i in label_line.items() if i < first_wait_line)[1]
        back = [n for n, (i, l) in enumerate(insns) if l.startswith(("s_cbranch", "s_branch")) and l.split()[-1] == header]
        assert back, (name, header)
        loop_end = back[-1]
        loop_start = next(m for m, (i, _) in enumerate(insns) if i > label_line[header])
        is_bound_load = re.compile(r"global_load_dword v\d+, .*\bsc1\b")
        for n, i, l in loads:
            dst = int(re.match(r"global_load_dword v(\d+),", l).group(1))
            nxt = [w for w in waits if w > n]
            window = insns[n + 1:nxt[0]] if nxt else insns[n + 1:loop_end + 1] + insns[loop_start:waits[0]]
            skip_to = None
            for line_no, other in window:
                if skip_to is not None:                     # behind an unconditional branch: not on this path
                    if line_no < skip_to:
                        continue
                    skip_to = None
                if other.startswith("s_branch "):           # (forward jump over the other arm of an if / else)
                    target = label_line.get(other.split()[1])
                    if target is not None and target > line_no:
                        skip_to = target
                    continue
                if is_bound_load.match(other):
                    continue
                ops = other.split(None, 1)[1] if " " in other else ""
                if ("v%d" % dst) not in ops and "v[" not in ops:
                    continue
                assert dst not in _regs(ops), "%s: v%d (an in-flight bound) is touched by `%s` before its wait" % (name, dst, other)
            checked += 1
    assert checked >= 8          # the top-1 kernels with three stage buffers (4 loads per stage body)
