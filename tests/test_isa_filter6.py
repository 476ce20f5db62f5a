"""CPU (hipcc cross-compiles): what filter6_kernel (K12, filter6.hip) relies on and the compiler does not know, read off
its gfx950 ISA as the product's flags give it.

1. The stationary operand and the row statistics are loaded by inline-asm global_load statements whose completion the
   compiler does not track; the hand-counted s_waitcnt behind the first two stages' LDS-DMA covers them, and only the
   empty "+v" asm statement behind that wait hands the registers over.  A copy, a re-allocation or a spill of a
   destination register in front of the wait would use data that has not landed -- usually it has, so the parity
   tests would pass on a quiet machine and lose matches on a busy one.
2. The waits are counted: vmcnt(2 D) / vmcnt(2 (D + 1)) in the prologue, vmcnt(D) / vmcnt(D + 1) at a hand-over, for D
   LDS-DMA per wave and stage plus one in the last wave.  D is counted in the code here, not taken from the source.
3. The hand-over barrier is raw: s_waitcnt lgkmcnt(0) + s_barrier.  A __syncthreads() would drain the DMA.
4. A flush of a wave's hit list drains with vmcnt(0), so that the DMA are again the wave's newest vector memory
   operations.
The checks are functions of isa_read.py; test_isa_read.py shows on hand-written snippets that each of them fails when it
should."""
import re

import pytest

import isa_read as R

pytestmark = pytest.mark.skipif(not R.have_hipcc(), reason="no hipcc")


@pytest.fixture(scope="module")
def k(tmp_path_factory):
    return R.kernel(R.isa("filter6", tmp_path_factory), "filter6_kernel")


@pytest.fixture(scope="module")
def d(k):
    return R.dma_per_stage(k)


def test_product_flags_are_the_makefiles():
    assert R.product_flags("filter6") == ["-O3", "-std=c++17", "-fno-honor-nans"]
    assert R.product_flags("rowreduce") == ["-O3", "-std=c++17"]


def test_operand_loads_are_not_named_before_the_hand_back(k):
    nc = int(re.search(r"constexpr int kF6NC = (\d+)", R.source("filter6")).group(1))
    # per block of 32 output rows: two K-halves of a 16-byte and an 8-byte load, and the row's statistics
    assert R.check_untracked_loads(k, expected=nc * (2 * 2 + 1)) == nc * 5


def test_dma_count_matches_the_source(k, d):
    # (the counted D is what the waits are held against; that it also is the source's 16 / kF6NW is a check of the counting)
    nw = int(re.search(r"constexpr int kF6NC = \d+, kF6NW = (\d+)", R.source("filter6")).group(1))
    assert d == 16 // nw


def test_prologue_waits_follow_the_dma_count(k, d):
    assert R.check_prologue_waits(k, d) == sorted({0, 2 * d, 2 * (d + 1)})


def test_hand_overs_are_raw_and_counted(k, d):
    n, drains = R.check_hand_overs(k, d)
    assert n == 3, n                                         # the stage loop is unrolled over the three stage buffers
    # Waits for vmcnt(0) that the compiler put between the first and the last hand-over.  Every one of today's stands
    # inside a flush, between its atomic and its own drain: one for the atomic's return value, one per 64 records in
    # front of the read of the list (an LDS read behind LDS-DMA in flight, which the compiler takes for a pending LDS
    # write).  The flush drains anyway.  Outside a flush such a wait is a drained pipeline: none today.
    flushes = R.flush_regions(k)
    outside = [(i, l) for i, l in drains if not any(a < i < b for a, b in flushes)]
    assert outside == [], "compiler-emitted vmcnt(0) between hand-overs, outside a flush: %s" % outside
    slots = int(re.search(r"constexpr int kF6HitSlots = (\d+)", R.source("filter6")).group(1))
    per_flush = [sum(1 for i, _ in drains if a < i < b) for a, b in flushes]
    assert max(per_flush) <= 1 + slots // 64, per_flush


def test_every_flush_drains(k):
    # (one copy of the flush per block and unit of the unrolled loop and the last one; two record stores each)
    assert R.check_flush(k) >= 2


def test_all_lds_dma_is_the_builtins(k):
    assert R.check_no_asm_lds_dma(k) > 0
