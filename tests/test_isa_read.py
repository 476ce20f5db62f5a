"""CPU, no compiler: the checks of isa_read.py on hand-written ISA.  GOOD has the shape of filter6_kernel's code -- three
untracked operand loads, two stages of LDS-DMA (D = 2 per wave, one more under an EXEC mask), the three counted waits
of the prologue, the hand-back, two raw hand-overs and a flush between them -- and passes every check.  Each broken
variant differs from it in one place and must be rejected with a message that names the register or the immediate:
this is the evidence that test_isa_filter6.py would fail if the kernel were subtly wrong."""
import pytest

import isa_read as R

GOOD = """
_ZN2fm6sampleEv:                        ; @_ZN2fm6sampleEv
; %bb.0:
	s_load_dwordx4 s[4:7], s[0:1], 0x0
	v_lshlrev_b32_e32 v1, 4, v0
	v_mov_b32_e32 v3, 0
	v_add_u32_e32 v2, s4, v1
	;;#ASMSTART
	global_load_dwordx4 v[10:13], v[2:3], off
	;;#ASMEND
	;;#ASMSTART
	global_load_dwordx2 v[14:15], v[2:3], off offset:16
	;;#ASMEND
	v_add_u32_e32 v2, s5, v1
	;;#ASMSTART
	global_load_dwordx4 v[2:5], v[2:3], off
	;;#ASMEND
	s_cmp_lt_i32 s6, 1
	s_cbranch_scc1 .LBB0_3
; %bb.1:
	s_mov_b32 m0, s8
	v_add_u32_e32 v20, s9, v1
	global_load_lds_dwordx4 v20, s[0:1]
	global_load_lds_dwordx4 v20, s[0:1] offset:1024
	s_and_saveexec_b64 s[2:3], vcc
	s_cbranch_execz .LBB0_2
; %bb.12:
	global_load_lds_dwordx4 v21, s[8:9]
.LBB0_2:
	s_or_b64 exec, exec, s[2:3]
.LBB0_3:
	s_cmp_gt_i32 s6, 1
	s_cbranch_scc1 .LBB0_4
; %bb.13:
	;;#ASMSTART
	s_waitcnt vmcnt(0)
	;;#ASMEND
	s_branch .LBB0_8
.LBB0_4:
	global_load_lds_dwordx4 v20, s[10:11]
	global_load_lds_dwordx4 v20, s[10:11] offset:1024
	s_and_saveexec_b64 s[2:3], s[12:13]
	s_cbranch_execz .LBB0_5
; %bb.14:
	;;#ASMSTART
	s_waitcnt vmcnt(4)
	;;#ASMEND
.LBB0_5:
	s_andn2_saveexec_b64 s[2:3], s[2:3]
	s_cbranch_execz .LBB0_7
; %bb.6:
	global_load_lds_dwordx4 v21, s[8:9]
	;;#ASMSTART
	s_waitcnt vmcnt(6)
	;;#ASMEND
.LBB0_7:
	s_or_b64 exec, exec, s[2:3]
.LBB0_8:
	;;#ASMSTART
	;;#ASMEND
	v_cvt_f32_i32_e32 v6, v2
	v_and_b32_e32 v7, 63, v10
.LBB0_9:                                ; =>This Inner Loop Header: Depth=1
	s_cmp_lt_i32 s7, s6
	s_cbranch_scc1 .LBB0_10
; %bb.15:
	;;#ASMSTART
	s_waitcnt vmcnt(0)
	;;#ASMEND
	s_branch .LBB0_13
.LBB0_10:
	s_and_saveexec_b64 s[2:3], s[12:13]
	s_cbranch_execz .LBB0_11
; %bb.16:
	;;#ASMSTART
	s_waitcnt vmcnt(2)
	;;#ASMEND
.LBB0_11:
	s_andn2_saveexec_b64 s[2:3], s[2:3]
	s_cbranch_execz .LBB0_12
; %bb.17:
	;;#ASMSTART
	s_waitcnt vmcnt(3)
	;;#ASMEND
.LBB0_12:
	s_or_b64 exec, exec, s[2:3]
.LBB0_13:
	;;#ASMSTART
	s_waitcnt lgkmcnt(0)
	s_barrier
	;;#ASMEND
	s_cbranch_vccnz .LBB0_15
; %bb.18:
	global_load_lds_dwordx4 v[22:23], off
	global_load_lds_dwordx4 v[22:23], off offset:1024
	s_and_saveexec_b64 s[2:3], s[14:15]
	s_cbranch_execz .LBB0_14
; %bb.19:
	global_load_lds_dwordx4 v[24:25], off
.LBB0_14:
	s_or_b64 exec, exec, s[2:3]
.LBB0_15:
	ds_read_b128 v[30:33], v8
	s_waitcnt lgkmcnt(0)
	v_mfma_f32_32x32x64_f8f6f4 v[40:55], v[30:35], v[10:15], 0 cbsz:2 blgp:2
	s_cmpk_lt_u32 s20, 0x81
	s_cbranch_scc1 .LBB0_17
; %bb.20:
	v_mov_b32_e32 v61, s20
	global_atomic_add v61, v60, v61, s[16:17] sc0
	s_waitcnt vmcnt(0)
	v_readfirstlane_b32 s21, v61
	s_waitcnt vmcnt(0)
	ds_read_b64 v[62:63], v9 offset:53248
	v_lshl_add_u64 v[64:65], v[56:57], 3, s[18:19]
	s_waitcnt lgkmcnt(0)
	global_store_dwordx2 v[64:65], v[62:63], off
	;;#ASMSTART
	s_waitcnt vmcnt(0)
	;;#ASMEND
	s_mov_b32 s20, 0
.LBB0_17:
	;;#ASMSTART
	ds_write_b64 v58, v[66:67]
	;;#ASMEND
	;;#ASMSTART
	s_waitcnt vmcnt(2)
	;;#ASMEND
	;;#ASMSTART
	s_waitcnt lgkmcnt(0)
	s_barrier
	;;#ASMEND
	s_add_i32 s7, s7, 2
	s_cmp_lt_i32 s7, s6
	s_cbranch_scc1 .LBB0_9
; %bb.21:
	s_endpgm
.Lfunc_end0:
	.size	_ZN2fm6sampleEv, .Lfunc_end0-_ZN2fm6sampleEv
amdhsa.kernels:
  - .agpr_count:     0
    .args:
      - .address_space:  global
        .name:           p
        .offset:         0
    .group_segment_fixed_size: 61440
    .max_flat_workgroup_size: 512
    .name:           _ZN2fm6sampleEv
    .private_segment_fixed_size: 0
    .vgpr_count:     68
    .vgpr_spill_count: 0
"""

HAND_BACK = "\t;;#ASMSTART\n\t;;#ASMEND\n\tv_cvt_f32_i32_e32 v6, v2\n"
FIRST_DMA = "\ts_mov_b32 m0, s8\n"
DRAIN = "\tglobal_store_dwordx2 v[64:65], v[62:63], off\n\t;;#ASMSTART\n\ts_waitcnt vmcnt(0)\n\t;;#ASMEND\n"
RAW = "\t;;#ASMSTART\n\ts_waitcnt lgkmcnt(0)\n\ts_barrier\n\t;;#ASMEND\n\ts_cbranch_vccnz .LBB0_15\n"


def sample(text=GOOD):
    return R.kernel(text, "sample")


def broken(old, new):
    assert GOOD.count(old) == 1, old
    return sample(GOOD.replace(old, new))


def test_good_snippet_passes_every_check():
    k = sample()
    assert R.check_untracked_loads(k, expected=3) == 3
    d = R.dma_per_stage(k)
    assert d == 2
    assert R.check_prologue_waits(k, d) == [0, 4, 6]
    n, drains = R.check_hand_overs(k, d)
    assert n == 2
    # (the two waits of the compiler's inside the flush: they are listed, and they lie in its region)
    flushes = R.flush_regions(k)
    assert len(flushes) == 1 and len(drains) == 2 and all(flushes[0][0] < i < flushes[0][1] for i, _ in drains)
    assert R.check_flush(k) == 1
    assert R.check_no_asm_lds_dma(k) == 9


def test_reader_splits_blocks_and_reads_metadata():
    k = sample()
    assert [b.vmcnt() for b in k.blocks if b.vmcnt() is not None] == [0, 4, 6, 0, 2, 3, 0, 2]
    assert sum(1 for b in k.blocks if not b.insns) == 1
    assert R._regs("v[2:5], v7, s[8:9], off") == {2, 3, 4, 5, 7}
    assert R.metadata(GOOD) == {"_ZN2fm6sampleEv": {"agpr_count": 0, "group_segment_fixed_size": 61440, "max_flat_workgroup_size": 512,
                                                   "private_segment_fixed_size": 0, "vgpr_count": 68, "vgpr_spill_count": 0}}


def test_read_of_a_loaded_register_before_the_wait_is_rejected():
    k = broken(FIRST_DMA, FIRST_DMA + "\tv_mov_b32_e32 v30, v12\n")
    with pytest.raises(R.IsaError, match=r"v12 \(destination of `global_load_dwordx4 v\[10:13\].*named by `v_mov_b32_e32 v30, v12`"):
        R.check_untracked_loads(k)


def test_spill_of_a_loaded_register_before_the_wait_is_rejected():
    k = broken(FIRST_DMA, FIRST_DMA + "\tscratch_store_dword off, v14, s32 offset:4\n")
    with pytest.raises(R.IsaError, match=r"`scratch_store_dword off, v14, s32 offset:4`.*spills v14"):
        R.check_untracked_loads(k)


def test_any_scratch_access_before_the_wait_is_rejected():
    k = broken(FIRST_DMA, FIRST_DMA + "\tscratch_load_dword v70, off, s32 offset:8\n")
    with pytest.raises(R.IsaError, match=r"`scratch_load_dword v70, off, s32 offset:8`"):
        R.check_untracked_loads(k)


def test_overwrite_of_a_loaded_register_before_the_wait_is_rejected():
    k = broken(FIRST_DMA, FIRST_DMA + "\tv_mov_b32_e32 v3, 0\n")
    with pytest.raises(R.IsaError, match=r"v3 \(destination of `global_load_dwordx4 v\[2:5\].*named by `v_mov_b32_e32 v3, 0`"):
        R.check_untracked_loads(k)


def test_use_in_one_branch_arm_is_rejected():
    # (behind the unconditional branch of the vmcnt(0) arm: a linear scan is stricter than the control flow, on purpose)
    k = broken("\ts_waitcnt vmcnt(4)\n", "\ts_waitcnt vmcnt(4)\n\t;;#ASMEND\n\tv_add_u32_e32 v15, 1, v15\n\t;;#ASMSTART\n\ts_nop 0\n")
    with pytest.raises(R.IsaError, match=r"v15 \(destination of `global_load_dwordx2 v\[14:15\]"):
        R.check_untracked_loads(k)


def test_missing_hand_back_is_rejected():
    k = broken(HAND_BACK, "\tv_cvt_f32_i32_e32 v6, v2\n")
    with pytest.raises(R.IsaError, match="no hand-back block"):
        R.check_untracked_loads(k)


def test_hand_back_in_front_of_the_waits_is_rejected():
    k = sample(GOOD.replace(HAND_BACK, "\tv_cvt_f32_i32_e32 v6, v2\n").replace(FIRST_DMA, "\t;;#ASMSTART\n\t;;#ASMEND\n" + FIRST_DMA))
    with pytest.raises(R.IsaError, match="no inline-asm s_waitcnt vmcnt in front of it"):
        R.check_untracked_loads(k)


def test_wrong_number_of_operand_loads_is_rejected():
    with pytest.raises(R.IsaError, match="3 inline-asm operand loads, the source's constants give 5"):
        R.check_untracked_loads(sample(), expected=5)


def test_prologue_wait_off_the_dma_count_is_rejected():
    k = broken("\ts_waitcnt vmcnt(4)\n", "\ts_waitcnt vmcnt(5)\n")
    assert R.dma_per_stage(k) == 2
    with pytest.raises(R.IsaError, match=r"vmcnt\(0, 5, 6\), but 2 LDS-DMA per wave and stage \(counted\) need vmcnt\(0, 4, 6\)"):
        R.check_prologue_waits(k, 2)


def test_a_third_dma_per_stage_is_seen_by_the_count():
    k = broken("\tglobal_load_lds_dwordx4 v[22:23], off offset:1024\n",
               "\tglobal_load_lds_dwordx4 v[22:23], off offset:1024\n\tglobal_load_lds_dwordx4 v[22:23], off offset:2048\n")
    with pytest.raises(R.IsaError, match=r"\[2, 3\] LDS-DMA per wave"):
        R.dma_per_stage(k)


def test_hand_over_wait_off_the_dma_count_is_rejected():
    k = broken("\ts_waitcnt vmcnt(3)\n", "\ts_waitcnt vmcnt(4)\n")
    with pytest.raises(R.IsaError, match=r"vmcnt\(4\) in front of the s_barrier .* allow vmcnt\(0\), vmcnt\(2\), vmcnt\(3\)"):
        R.check_hand_overs(k, 2)


def test_barrier_without_lgkmcnt_is_rejected():
    k = broken(RAW, RAW.replace("\ts_waitcnt lgkmcnt(0)\n", ""))
    with pytest.raises(R.IsaError, match=r"s_barrier at line \d+ without `s_waitcnt lgkmcnt\(0\)` directly in front of it"):
        R.check_hand_overs(k, 2)


def test_compilers_barrier_is_rejected():
    # what __syncthreads() compiles to: the wait drains the LDS-DMA as well
    k = broken(RAW, "\ts_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier\n\ts_cbranch_vccnz .LBB0_15\n")
    with pytest.raises(R.IsaError, match=r"s_barrier at line \d+ without .*compiler-emitted"):
        R.check_hand_overs(k, 2)


def test_compilers_drain_between_hand_overs_is_listed():
    k = broken("\tds_read_b128 v[30:33], v8\n", "\ts_waitcnt vmcnt(0)\n\tds_read_b128 v[30:33], v8\n")
    _, drains = R.check_hand_overs(k, 2)
    flushes = R.flush_regions(k)
    assert len([i for i, _ in drains if not any(a < i < b for a, b in flushes)]) == 1


def test_record_store_without_a_drain_is_rejected():
    k = broken(DRAIN, "\tglobal_store_dwordx2 v[64:65], v[62:63], off\n")
    with pytest.raises(R.IsaError, match=r"record store `global_store_dwordx2 v\[64:65\], v\[62:63\], off` .*vmcnt\(2\)"):
        R.check_flush(k)


def test_record_store_behind_a_conditional_drain_is_rejected():
    k = broken(DRAIN, DRAIN.replace("\t;;#ASMSTART\n", "\ts_cbranch_execz .LBB0_17\n\t;;#ASMSTART\n"))
    with pytest.raises(R.IsaError, match=r"`s_cbranch_execz \.LBB0_17` \(line \d+\) can pass the vmcnt\(0\)"):
        R.check_flush(k)


def test_inline_asm_lds_dma_is_rejected():
    k = broken("\tglobal_load_lds_dwordx4 v[24:25], off\n", "\t;;#ASMSTART\n\tglobal_load_lds_dwordx4 v[24:25], off\n\t;;#ASMEND\n")
    with pytest.raises(R.IsaError, match="inline-asm LDS-DMA `global_load_lds_dwordx4 v\\[24:25\\], off`"):
        R.check_no_asm_lds_dma(k)
