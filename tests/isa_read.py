"""A small reader of gfx950 device ISA, shared by the tests that check what only the generated code can show
(test_isa_hazards.py, test_isa_filter6.py, test_kernel_resources.py; test_isa_read.py tests the checks themselves on
hand-written snippets, without a compiler).

Part 1 is text handling: compile a unit of fast-match_amd/csrc with the product's flags (once per session), split the text
into kernels, list instructions with their line numbers, find the inline-asm (ASMSTART / ASMEND) blocks, read the
per-kernel metadata of the amdhsa.kernels note.

Part 2 are checks over one kernel's text for code that is right only as long as the compiler leaves hand-written
synchronisation alone: loads the compiler does not track (inline-asm global_load with "=v" outputs, waited for with a
hand-counted s_waitcnt and handed to the compiler by an empty asm statement behind it), counted waits against the number
of LDS-DMA per stage, raw barriers, the drain behind a flush.  Every check raises IsaError (an AssertionError) whose
message names the register or the immediate.

Vector memory instructions are told by the mnemonic prefixes in VMEM_PREFIXES and by nothing else."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fast-match_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
VMEM_PREFIXES = ("global_", "flat_", "scratch_", "buffer_")


class IsaError(AssertionError):
    pass


def have_hipcc():
    return os.path.exists(HIPCC)


def _regs(operand_text):
    """VGPR numbers mentioned in an operand string: v12, v[34:37]."""
    out = set()
    for a, b in re.findall(r"\bv\[(\d+):(\d+)\]", operand_text):
        out.update(range(int(a), int(b) + 1))
    out.update(int(x) for x in re.findall(r"\bv(\d+)\b", operand_text))
    return out


def operands(insn):
    return insn.split(None, 1)[1] if " " in insn else ""


def source(unit):
    return open(os.path.join(CSRC, unit + ".hip")).read()


def product_flags(unit):
    """What the Makefile compiles csrc/<unit>.hip with, as far as it shapes device code: the -O and -std of CXXFLAGS and
    the unit's own FLAGS_<unit>."""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    cxx = re.search(r"^CXXFLAGS\s*=\s*(.*)$", mk, re.M).group(1).split()
    flags = [f for f in cxx if re.match(r"-O\w$|-std=", f)]
    assert len(flags) == 2, cxx
    own = re.search(r"^FLAGS_%s\s*=\s*(.*)$" % re.escape(unit), mk, re.M)
    return flags + (own.group(1).split() if own else [])


_ASM = {}


def isa(unit, tmp_path_factory):
    """Device ISA of csrc/<unit>.hip (compiled once per test session, whichever test file asks first)."""
    if unit not in _ASM:
        asm = str(tmp_path_factory.mktemp("isa") / (unit + ".s"))
        subprocess.check_call([HIPCC] + product_flags(unit) + ["--offload-arch=gfx950", "-S", "--cuda-device-only",
                               os.path.join(CSRC, unit + ".hip"), "-o", asm], stderr=subprocess.DEVNULL)
        _ASM[unit] = open(asm).read()
    return _ASM[unit]


class Block(object):
    """One ASMSTART / ASMEND pair: the line numbers of the two markers and the instructions between them."""
    def __init__(self, start):
        self.start, self.end, self.insns = start, None, []

    def texts(self):
        return [l for _, l in self.insns]

    def vmcnt(self):
        """The immediate, if the block is nothing but one `s_waitcnt vmcnt(N)`."""
        t = self.texts()
        m = re.match(r"s_waitcnt vmcnt\((\d+)\)$", t[0]) if len(t) == 1 else None
        return int(m.group(1)) if m else None


class Kernel(object):
    """One kernel of a unit's ISA text.  `lines` are the stripped lines of its code (up to .Lfunc_end, or, with first_exit,
    up to the first s_endpgm as the older checks read it), `insns` the (line number, text) of its instructions -- no
    labels, directives or comments --, `blocks` its inline-asm statements, `in_asm` the line numbers inside one."""
    def __init__(self, name, text, first_exit=False):
        self.name, self.text = name, text
        body = text.split("s_endpgm")[0] if first_exit else re.split(r"\n\.Lfunc_end\d+:", text)[0]
        self.lines = [l.strip() for l in body.splitlines()]
        self.insns, self.blocks, self.in_asm, self.label_line = [], [], set(), {}
        cur = None
        for i, l in enumerate(self.lines):
            if "ASMSTART" in l:
                cur = Block(i)
                continue
            if "ASMEND" in l:
                if cur is not None:
                    cur.end = i
                    self.blocks.append(cur)
                cur = None
                continue
            m = re.match(r"(\.LBB\d+_\d+):", l)              # ".LBB0_39:      ; in Loop: Header=..."
            if m:
                self.label_line[m.group(1)] = i
            if not l or l.startswith((";", ".", "//")):
                continue
            self.insns.append((i, l))
            if cur is not None:
                cur.insns.append((i, l))
                self.in_asm.add(i)
        if cur is not None:                                  # (cut off by first_exit)
            cur.end = len(self.lines)
            self.blocks.append(cur)

    def between(self, lo, hi):
        """Instructions on lines lo < i < hi."""
        return [(i, l) for i, l in self.insns if lo < i < hi]


def kernels(text, first_exit=False):
    """The fm:: kernels of a unit's ISA text, split at their `_ZN2fm...:` labels."""
    out = []
    for k in re.split(r"\n(?=_ZN2fm\w+:)", text):
        name = k.split(":", 1)[0]
        if name.startswith("_ZN2fm"):
            out.append(Kernel(name, k, first_exit))
    return out


def kernel(text, substring):
    found = [k for k in kernels(text) if substring in k.name]
    assert len(found) == 1, (substring, [k.name for k in found])
    return found[0]


_META_KEYS = ("vgpr_count", "agpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
              "group_segment_fixed_size", "max_flat_workgroup_size")


def metadata(text):
    """{kernel name: {key: int}} from the amdhsa.kernels note of a unit's ISA text, for the keys in _META_KEYS."""
    note = text.split("amdhsa.kernels:", 1)[1]
    out, cur = {}, None
    for l in note.splitlines():
        if re.match(r"  - \.", l):
            cur = {}
        m = re.match(r"  [ -] \.(\w+):\s+(\S+)\s*$", l)       # (the kernel's own keys: those of its arguments sit deeper)
        if not m or cur is None:
            continue
        if m.group(1) == "name":
            out[m.group(2)] = cur
        elif m.group(1) in _META_KEYS:
            cur[m.group(1)] = int(m.group(2))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# Part 2: checks

_LOAD = re.compile(r"global_load_dwordx[24] (v\[\d+:\d+\]),")
_DMA = "global_load_lds_dwordx4"
_BRANCH = ("s_cbranch", "s_branch")


def _is_vmem(insn):
    return insn.startswith(VMEM_PREFIXES)


def untracked_window(k):
    """(loads, waits, hand_back) of a kernel's prologue.  loads: [(line, text, destination registers)] of the inline-asm
    global_load_dwordx4 / x2 in front of the first LDS-DMA; hand_back: the first EMPTY asm block behind them and in
    front of the first s_barrier -- the "+v" statement that gives the registers to the compiler --; waits: the asm blocks
    that are one `s_waitcnt vmcnt(N)` between the last load and the hand-back."""
    dma = [i for i, l in k.insns if l.startswith(_DMA)]
    if not dma:
        raise IsaError("%s: no %s" % (k.name, _DMA))
    loads = []
    for b in k.blocks:
        if b.start > dma[0]:
            break
        for i, l in b.insns:
            m = _LOAD.match(l)
            if m:
                loads.append((i, l, _regs(m.group(1))))
    if not loads:
        raise IsaError("%s: no inline-asm operand load in front of the first %s" % (k.name, _DMA))
    last = loads[-1][0]
    barriers = [i for i, l in k.insns if l == "s_barrier"]
    limit = barriers[0] if barriers else len(k.lines)
    empty = [b for b in k.blocks if last < b.start < limit and not b.insns]
    if not empty:
        raise IsaError("%s: no hand-back block (an empty asm statement) between the operand loads and the first s_barrier"
                       % k.name)
    hand_back = empty[0]
    waits = [b for b in k.blocks if last < b.start < hand_back.start and b.vmcnt() is not None]
    if not waits:
        raise IsaError("%s: the hand-back block at line %d has no inline-asm s_waitcnt vmcnt in front of it" % (k.name, hand_back.start))
    return loads, waits, hand_back


def check_untracked_loads(k, expected=None):
    """From each untracked load to the hand-back, in program order over every branch arm, nothing but the asm loads
    themselves names a destination register of an earlier asm load, reading or writing; no scratch_ instruction stands
    there at all; and no branch leaves the range, so that program order is all there is.  Returns the number of loads."""
    loads, _, hand_back = untracked_window(k)
    if expected is not None and len(loads) != expected:
        raise IsaError("%s: %d inline-asm operand loads, the source's constants give %d" % (k.name, len(loads), expected))
    first = loads[0][0]
    dest_at = {i: d for i, _, d in loads}
    in_flight = {}                                           # register -> the load that writes it
    for i, l in k.insns:
        if i < first or i >= hand_back.start:
            continue
        named = _regs(operands(l))
        if i in dest_at:
            named -= dest_at[i]                              # (its own destination; the address may be an older register)
        hit = sorted(r for r in named if r in in_flight)
        if l.startswith("scratch_"):
            raise IsaError("%s: `%s` (line %d) between the untracked loads and their wait%s"
                           % (k.name, l, i, ": it spills v%d, which is in flight" % hit[0] if hit else ""))
        if hit:
            raise IsaError("%s: v%d (destination of `%s`, in flight) is named by `%s` (line %d) before the wait"
                           % (k.name, hit[0], in_flight[hit[0]], l, i))
        if i in dest_at:
            for r in dest_at[i]:
                in_flight[r] = l
        if l.startswith(_BRANCH):
            t = k.label_line.get(l.split()[1])
            if t is None or not first < t < hand_back.start:
                raise IsaError("%s: `%s` (line %d) leaves the range between the untracked loads and the hand-back" % (k.name, l, i))
    return len(loads)


def dma_per_stage(k):
    """D: the LDS-DMA instructions one wave issues for a stage, counted in the code.  A run of them inside one basic
    block is a stage body if the branch in front of the block tests a scalar condition, and the one extra instruction of
    the last wave if it tests EXEC.  Every body must have the same count, every extra must be one."""
    runs, cur, masked = [], 0, False
    last_branch = ""
    labels = set(k.label_line.values())
    text = dict(k.insns)
    for i in range(len(k.lines)):
        l = text.get(i, "")
        if i in labels or l.startswith(_BRANCH):             # a basic block ends
            if cur:
                runs.append((cur, masked))
            cur, last_branch = 0, l                          # (behind a label: a join, no mask known)
            continue
        if l.startswith(_DMA):
            if cur == 0:
                masked = last_branch.startswith(("s_cbranch_execz", "s_cbranch_execnz"))
            cur += 1
    if cur:
        runs.append((cur, masked))
    bodies = sorted(set(n for n, m in runs if not m))
    extras = sorted(set(n for n, m in runs if m))
    if len(bodies) != 1:
        raise IsaError("%s: stage bodies of %s LDS-DMA per wave: no single count" % (k.name, bodies))
    if extras not in ([], [1]):
        raise IsaError("%s: %s LDS-DMA under an EXEC mask, expected one per stage" % (k.name, extras))
    return bodies[0]


def check_prologue_waits(k, d):
    """The inline-asm waits between the untracked loads and the hand-back are exactly vmcnt(0), vmcnt(2 D) and
    vmcnt(2 (D + 1)): no stage, two stages of an ordinary wave, two stages of the last wave."""
    _, waits, _ = untracked_window(k)
    have = sorted(set(b.vmcnt() for b in waits))
    want = sorted({0, 2 * d, 2 * (d + 1)})
    if have != want:
        raise IsaError("%s: prologue waits vmcnt%s, but %d LDS-DMA per wave and stage (counted) need vmcnt%s"
                       % (k.name, tuple(have), d, tuple(want)))
    return have


def check_hand_overs(k, d):
    """Every s_barrier stands in one asm block with `s_waitcnt lgkmcnt(0)` directly in front of it, and the nearest
    inline-asm vmcnt wait in front of it is vmcnt(0), vmcnt(D) or vmcnt(D + 1).  Returns (hand-overs, compiler-emitted
    `s_waitcnt vmcnt(0)` between the first and the last of them: [(line, text)])."""
    bars = [i for i, l in k.insns if l == "s_barrier"]
    if not bars:
        raise IsaError("%s: no s_barrier" % k.name)
    block_of = {i: b for b in k.blocks for i, _ in b.insns}
    for i in bars:
        b = block_of.get(i)
        t = b.texts() if b else []
        n = [j for j, _ in b.insns].index(i) if b else 0
        if b is None or n == 0 or t[n - 1] != "s_waitcnt lgkmcnt(0)":
            raise IsaError("%s: s_barrier at line %d without `s_waitcnt lgkmcnt(0)` directly in front of it in its asm "
                           "statement (%s)" % (k.name, i, "; ".join(t) if b else "compiler-emitted"))
        before = [w.vmcnt() for w in k.blocks if w.end < b.start and w.vmcnt() is not None]
        if not before:
            raise IsaError("%s: s_barrier at line %d has no inline-asm vmcnt wait in front of it" % (k.name, i))
        if before[-1] not in (0, d, d + 1):
            raise IsaError("%s: vmcnt(%d) in front of the s_barrier at line %d, but %d LDS-DMA per wave and stage (counted) "
                           "allow vmcnt(0), vmcnt(%d), vmcnt(%d)" % (k.name, before[-1], i, d, d, d + 1))
    drains = [(i, l) for i, l in k.between(bars[0], bars[-1])
              if i not in k.in_asm and l.startswith("s_waitcnt") and re.search(r"\bvmcnt\(0\)", l)]
    return len(bars), drains


def flush_regions(k):
    """[(first line, last line)]: from a global_atomic (a flush reserves its records with one) to the next inline-asm
    `s_waitcnt vmcnt(0)`, the flush's own drain.  A wait of the compiler's inside costs nothing the drain does not."""
    ends = [b.start for b in k.blocks if b.vmcnt() == 0]
    out = []
    for i, l in k.insns:
        if l.startswith("global_atomic") and not (out and out[-1][0] < i <= out[-1][1]):
            e = [x for x in ends if x > i]
            if e:
                out.append((i, e[0]))
    return out


def check_flush(k):
    """Every record store -- a global_store whose data registers were last written by a ds_read (the wave's hit list) --
    is followed in program order by an inline-asm `s_waitcnt vmcnt(0)` before the next s_barrier.  Returns their number."""
    stores = []
    writer = {}                                              # register -> mnemonic that wrote it last (program order)
    for i, l in k.insns:
        op = l.split()[0]
        ops = [o.strip() for o in operands(l).split(",")]
        if op.startswith("global_store"):
            if len(ops) >= 2 and any(writer.get(r, "").startswith("ds_read") for r in _regs(ops[1])):
                stores.append((i, l))
        elif op.startswith(("s_", "ds_write")) or (_is_vmem(op) and "_store" in op) or ("_atomic" in op and " sc0" not in l):
            continue                                         # (no vector destination)
        elif ops:
            for r in _regs(ops[0]):
                writer[r] = op
    if not stores:
        raise IsaError("%s: no record store (a global_store fed from a ds_read)" % k.name)
    waits = [b for b in k.blocks if b.vmcnt() is not None]
    for i, l in stores:
        # the next hand-written wait must be the flush's drain, reached whatever the lanes do: no branch between the
        # store and it may jump past it (the vmcnt(0) of a hand-over stands under a condition and is no substitute)
        w = next((b for b in waits if b.start > i), None)
        why = None
        if w is None:
            why = "no inline-asm vmcnt wait behind it"
        elif w.vmcnt() != 0:
            why = "the next inline-asm wait is vmcnt(%d)" % w.vmcnt()
        else:
            for j, o in k.between(i, w.start):
                if o == "s_barrier":
                    why = "an s_barrier (line %d) comes first" % j
                elif o.startswith(_BRANCH) and not i < k.label_line.get(o.split()[1], -1) < w.start:
                    why = "`%s` (line %d) can pass the vmcnt(0) at line %d" % (o, j, w.start + 1)
                if why:
                    break
        if why:
            raise IsaError("%s: record store `%s` (line %d) is not drained by an inline-asm `s_waitcnt vmcnt(0)`: %s"
                           % (k.name, l, i, why))
    return len(stores)


def check_no_asm_lds_dma(k):
    """All LDS-DMA of the kernel is the builtin's, whose M0 the compiler manages.  Returns their number."""
    bad = [l for i, l in k.insns if l.startswith("global_load_lds") and i in k.in_asm]
    if bad:
        raise IsaError("%s: inline-asm LDS-DMA `%s` beside the builtin's: M0 is the compiler's here" % (k.name, bad[0]))
    return sum(1 for _, l in k.insns if l.startswith("global_load_lds"))
