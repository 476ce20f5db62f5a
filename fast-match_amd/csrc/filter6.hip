// K12 -- the accepted-only sweep as an FP6 matrix-core filter, with exact rescoring of what it keeps.
//
// The accepted-only calls hand K1 the ratio test's distance cut D* (ratio_cut.h): only candidates at d2 < D* can reach the
// output, and on descriptor data those are a few in a million.  K1 still pays the full int8 MFMA rate to find them.  This
// file sweeps splits of the streamed bank -- its own count of them, chosen for the launch as a whole (fp6_plan.h: one
// workgroup fills a CU, K1's count was tuned for 16 waves per CU) --, two of K1's 512-row output chunks per workgroup, with
// K1's staging -- three LDS stage buffers filled by LDS-DMA two stages ahead, the source-side XOR swizzle, the hand-over
// waits -- but on v_mfma_f32_32x32x64_f8f6f4 with e2m3 operands (cbsz:2 blgp:2, the form without
// scale operands: the builtin with all four scale arguments 0): a wave holds 128 output rows and multiplies a 32-row
// unit of the streamed bank against them with 8 instructions, in two halves of four with the max trees of the half
// before between them (no priority flips: there is no burst and no epilogue to tell apart).  FP6 is lossy, so the sweep is a FILTER with a static
// per-row threshold that provably keeps every candidate at d2 <= D* - 1 (fp6_filter.h); there are no shared bounds, no
// atomics on the fast path and no top-K state.  The accumulators start at zero; the rows' start values -|m|^2 / 2 (the 1 KiB
// behind a stage's rows in the plane, staged into a ring of four slots beside the stage buffers) are read only by a block
// that passes a screen against thr - (the stage's largest start), which is then tested exactly.  A lane whose 16 candidates of a 32-row unit (one output row, half of the
// unit's rows) clear its threshold writes (output row, unit, half) to its wave's list in LDS, which the wave copies to the
// pair's list when it is full and when its sweep ends;
// rescore6_kernel then computes the exact int32 d2 of each listed row against those 16 streamed rows from the int8
// plane, as K1 does, and folds (d2 << 32 | row) into slice 0 of the pair's `partial` with a 64-bit atomic minimum -- the key
// K1 writes and the order the election reduces with (lowest streamed row on ties).  The sweep's workgroups preset K1's
// slices of `partial` for their output rows to "none" (split f of the filter takes slices f, f + nsplit_f, ...), so the
// kernels behind it see K1's layout.
// A list that overflows, or a pair without a finite cut, sets the pair's need_k1 word; the guarded K1 launch behind the
// rescoring (rowreduce.hip) then redoes such pairs in full.  Nothing waits on the host.  The batched call runs the
// rescoring and the guard on a stream beside the sweep's (Filter6Ws::side), under the next launch's sweep.
//
// Bank plane (Bank::rows6 / aux6 / stat6 / max6, prep6_kernel): the 128 codes of a row as four K-chunks of 32 codes (24
// bytes) in 32-byte slots -- a row stays 128 bytes, so K1's LDS image and its swizzle carry over; lane (row, half) of a
// fragment reads slot 2 h + half for the instruction of K-half h, both operands through the same lane -> byte map, so the
// instruction's k order cancels.
#include "tile_ops.h"
#include "fp6_filter.h"
#include "fp6_plan.h"

namespace fm {

typedef int   v8i_6  __attribute__((ext_vector_type(8)));
typedef int   v2i_6  __attribute__((ext_vector_type(2)));
typedef float v4f_6  __attribute__((ext_vector_type(4)));
typedef float v16f_6 __attribute__((ext_vector_type(16)));

#define F6_LDS_PTR(p) ((__attribute__((address_space(3))) void*)(p))
#define F6_GLB_PTR(p) ((const __attribute__((address_space(1))) void*)(p))
#define F6_INLINE __attribute__((always_inline))
// the scheduler's order inside a basic block: one matrix instruction, then N vector instructions (masks 0x8, 0x2)
#define F6_MFMA_THEN_VALU(N) do { __builtin_amdgcn_sched_group_barrier(0x8, 1, 0); __builtin_amdgcn_sched_group_barrier(0x2, N, 0); } while (0)

constexpr int kF6NC = 4, kF6NW = 8;                       // blocks of 32 output rows per wave, waves per workgroup
constexpr int kF6PieceRows = 512;                         // K1's chunk in the batched shape: the granule of the plan and of `partial`
constexpr int kF6ChunkRows = 32 * kF6NC * kF6NW;          // 1024: two of K1's chunks per workgroup
constexpr int kF6Units = kStageRows / kTileRows;          // 32-row units per stage: 4
constexpr int kF6HitSlots = 128;                          // records of a wave's private list in LDS (one block's ballot delivers <= 64)
static_assert(kF6HitSlots >= 64 && kF6HitSlots % 64 == 0, "a block's ballot must fit an empty list; the flush copies 64 at a time");
// static LDS: three stage buffers of rows alone, a ring of four stages' accumulator starts, the waves' lists
constexpr int kF6RingSlots = 4;
constexpr int kF6RingOff = 3 * kStageRowBytes;
constexpr int kF6HitsOff = kF6RingOff + kF6RingSlots * kStageAuxBytes;
constexpr int kF6LdsBytes = kF6HitsOff + kF6NW * kF6HitSlots * 8;
constexpr int kF6SmaxWord = kStageRows;                   // aux6[stage][128]: the largest start among the stage's real rows
static_assert(kF6LdsBytes == 61440 && kF6LdsBytes <= 65536, "the kernel's static LDS");

struct F6Params {
    const uint8_t* col_rows6;
    const int32_t* col_stat;      // [row][4]: |c|^2, |c^|^2, |c - c^|^2, 0
    int            ncols;         // real output rows
    int            ncols_pad;
    const uint8_t* red_rows6;
    const float*   red_aux6;      // [stage][256]: accumulator start of the stage's 128 rows, their maximum, 127 unused words
    const int32_t* red_max;       // [2]: largest |m|^2, largest |m - m^|^2 of the streamed bank
    int            nstages, nsplit, nchunks, stages_per_split, ncols_alloc;      // K1's plan: the layout of `partial`
    int            nsplit_f, stages_per_split_f;                                 // the filter's own splits of the streamed bank (fp6_plan.h)
    unsigned long long* partial;  // K1's [nsplit][ncols_alloc] keys
    const unsigned* cut;          // device word D*
    uint2*         rec;           // the pair's list: (output row, 32-row unit of the streamed bank | half of the unit << 31)
    unsigned       cap;
    unsigned*      cnt;           // [0] records appended (may exceed cap), [1] need_k1
    // rescoring: the int8 planes
    const int8_t*  col_rows8;
    const int32_t* col_norm;
    const int8_t*  red_rows8;
    const int32_t* red_norm;
    int            nred;
};

struct F6Batch {
    F6Params p[kRRBatchMax];
    int      n;
    int      first_block[kRRBatchMax + 1];
};

// K1's issue_stage<true, 8>: 128 rows (16 KiB) into a stage buffer, the stage's 1 KiB of accumulator starts into `aux`, its
// slot of the ring.  `wave` is the wave's number in a scalar register, so that the source and the LDS address of a piece are
// scalar too; `off` is the lane's byte offset in a piece.  A wave's pieces are wave, wave + 8: 64 rows apart, they have one
// swizzle and share `off`.  `last` (the last wave: it also brings the starts) is a lane value: that DMA stands under EXEC.
__device__ __forceinline__ void f6_issue_stage(const uint8_t* red_rows6, const float* red_aux6, int stage, char* buf, char* aux, int wave, bool last,
                                               unsigned off, unsigned aux_off)
{
    const uint8_t* src_rows = red_rows6 + (size_t)stage * kStageRowBytes;
    constexpr int kPieces = 16 / kF6NW;
#pragma unroll
    for (int i = 0; i < kPieces; ++i) {
        const int g = wave + kF6NW * i;
        __builtin_amdgcn_global_load_lds(F6_GLB_PTR(src_rows + g * 1024 + off), F6_LDS_PTR(buf + g * 1024), 16, 0, 0);
    }
    if (last) __builtin_amdgcn_global_load_lds(F6_GLB_PTR((const char*)(red_aux6 + (size_t)stage * (kStageAuxBytes / 4)) + aux_off), F6_LDS_PTR(aux), 16, 0, 0);
}

// One 32-row unit of the streamed bank as a lane reads it: per K-half h the two 16-byte pieces of slot 2 h + (lane >> 5) of
// row lane & 31 (the last 8 bytes are the slot's padding: the 6-register operand ends in front of them).  The accumulator
// starts of the lane's 16 rows -- in the 32 x 32 C layout register r holds streamed row (r & 3) + 8 (r >> 2) + 4 (lane >> 5) --
// are not part of it: they are read where a block passes the screen (below).
struct F6Unit {
    v8i_6  a[2];      // (registers 6 and 7 are never written: the operand is the first six)
};

__device__ __forceinline__ float f6_max16(const v16f_6& a)
{
    const float m0 = fmaxf(fmaxf(a[0], a[1]), a[2]);
    const float m1 = fmaxf(fmaxf(a[3], a[4]), a[5]);
    const float m2 = fmaxf(fmaxf(a[6], a[7]), a[8]);
    const float m3 = fmaxf(fmaxf(a[9], a[10]), a[11]);
    const float m4 = fmaxf(fmaxf(a[12], a[13]), a[14]);
    const float m5 = fmaxf(fmaxf(m0, m1), m2);
    const float m6 = fmaxf(fmaxf(m3, m4), a[15]);
    return fmaxf(m5, m6);
}

// thr_s of two blocks from the stage's largest start (wave-uniform, in a scalar register): fp6_screen_threshold twice under
// one change of the rounding mode (bits 1:0 of the MODE register, 2 = towards -infinity; fp6_filter.h)
__device__ __forceinline__ void f6_screen2(float& s0, float& s1, float t0, float t1, float smax)
{
    asm("s_setreg_imm32_b32 hwreg(HW_REG_MODE, 0, 2), 2\n\t"
        "v_subrev_f32 %0, %4, %2\n\t"
        "v_subrev_f32 %1, %4, %3\n\t"
        "s_nop 1\n\t"
        "s_setreg_imm32_b32 hwreg(HW_REG_MODE, 0, 2), 0\n\t"
        "s_nop 1" : "=&v"(s0), "=&v"(s1) : "v"(t0), "v"(t1), "s"(smax));
}

// The sweep on v_mfma_f32_32x32x64_f8f6f4: a wave owns 128 output rows (4 blocks of 32, the stationary B operand: 48
// registers) and multiplies every 32-row unit of the streamed bank against them with 8 instructions, two per block chained
// along K.  The reads of a unit are issued one unit ahead into a second register set, across the stage hand-over too: a
// wave enters the barrier with the last unit of the stage it leaves in registers and multiplies it behind the barrier.
__global__ __launch_bounds__(64 * kF6NW, 2)
void filter6_kernel(F6Batch b)
{
    __shared__ __attribute__((aligned(16))) char smem[kF6LdsBytes];
    int pair = 0;
#pragma unroll
    for (int i = 1; i < kRRBatchMax; ++i) pair += (int)blockIdx.x >= b.first_block[i] ? 1 : 0;
    const F6Params& p = b.p[pair];
    const int bid = (int)blockIdx.x - b.first_block[pair];

    const int tid  = threadIdx.x;
    const int lane = tid & 63;
    // (the wave's number twice: in a scalar register for every address made of it, as a lane value for the conditions on it)
    const int wave_v = tid >> 6;
    const int wave = __builtin_amdgcn_readfirstlane(wave_v);
    // a lane's place in a 1 KiB piece of the LDS-DMA: row lane >> 3 of the piece's 8, 16-byte slot lane & 7, swizzled by the
    // row's number in the stage (the piece's first row is a multiple of 8, and a wave's pieces are 64 rows apart)
    const unsigned dma_off = (unsigned)((lane >> 3) * kDim + 16 * ((lane & 7) ^ ((((wave & 1) * 8 + (lane >> 3)) >> 1) & 7)));
    const unsigned dma_aux_off = (unsigned)(lane * 16);
    const int r32  = lane & 31;
    const int hs   = lane >> 5;
    // everything the loop uses, once: a field read through `p` inside the loop is a scalar load of the kernel argument there
    const int nsplit = p.nsplit_f, nstages = p.nstages, per = p.stages_per_split_f, ncols = p.ncols, ncols_pad = p.ncols_pad;
    const int ncols_alloc = p.ncols_alloc;
    const int nch = (p.nchunks + 1) >> 1;
    const uint8_t* const red_rows6 = p.red_rows6;
    const float* const red_aux6 = p.red_aux6;
    uint2* const rec = p.rec;
    unsigned* const cnt = p.cnt;
    const unsigned cap = p.cap;
    // (uniform, but the quotient comes out of the vector unit: left there, the stage counter and the DMA addresses of every
    // hand-over follow it into vector registers)
    const int split = __builtin_amdgcn_readfirstlane(bid / nch), chunk = bid - split * nch;
    if (split >= nsplit) return;
    const int st0 = split * per;
    const int st1 = min(st0 + per, nstages);
    const int cb  = chunk * kF6ChunkRows + wave * (32 * kF6NC);

    const unsigned dstar = *p.cut;
    if (dstar == kNoRatioCut) {               // no finite cut (device-side knowledge: the largest self distance): K1 redoes the pair
        if (tid == 0) cnt[1] = 1u;
        return;
    }
    // this workgroup's pieces of K1's key array start empty (the rescoring folds into slice 0 after this kernel): of K1's
    // slices of its rows -- the election reads them all -- the filter's split f takes s = f, f + nsplit_f, ... below K1's
    // count (none where f is beyond it); an odd number of K1 chunks leaves the last workgroup's second piece outside the array
    {
        const int nslices = p.nsplit;
        const bool second = chunk * kF6ChunkRows + kF6PieceRows < ncols_alloc;
        for (int s = split; s < nslices; s += nsplit) {
            unsigned long long* mine = p.partial + (size_t)s * ncols_alloc + chunk * kF6ChunkRows;
            mine[tid] = ~0ull;
            if (second) mine[kF6PieceRows + tid] = ~0ull;
        }
    }

    // stationary operand: per block j and K-half h, slot 2 h + (lane >> 5) (32 codes, 24 of 32 bytes) of output row
    // cb + 32 j + (lane & 31); one threshold per lane and block
    v8i_6 bf[kF6NC][2];
    float thr[kF6NC];
    constexpr int kDmaPerWave = 16 / kF6NW;
    {
        const int um = p.red_max[0], em = p.red_max[1];
        v4i lo[kF6NC][2], stat[kF6NC];
        v2i_6 hi[kF6NC][2];
        // The loads as asm statements, unconditional (a lane beyond the bank reads its last row and drops it below), for
        // two reasons.  Behind a condition each load is waited for where its branch ends, one round trip after the other.
        // And with LDS-DMA in flight the compiler's own wait at the first use of a loaded register is vmcnt(0), which
        // would drain the DMA issued below: it does not know of these loads, and the counted wait below is ours.
#pragma unroll
        for (int j = 0; j < kF6NC; ++j) {
            const int n = min(cb + 32 * j + r32, ncols_pad - 1);
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const uint8_t* src = p.col_rows6 + (size_t)n * kDim + 32 * (2 * h + hs);
                asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(lo[j][h]) : "v"(src) : "memory");
                asm volatile("global_load_dwordx2 %0, %1, off offset:16" : "=v"(hi[j][h]) : "v"(src) : "memory");
            }
            asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(stat[j]) : "v"(p.col_stat + 4 * (size_t)n) : "memory");
        }
        // The first two stages' LDS-DMA are issued HERE, behind the operand loads, and fly under the threshold arithmetic
        // below.  They are this wave's newest vector memory operations (wave 7 issues one more per stage) and reads return
        // in order, so the loads have landed at a counted vmcnt; the stage loop's hand-over waits count on the same order.
        // (The presets of `partial` above are older stores: they can only make the wait longer.)
        const int nfirst = min(st1 - st0, 2);
        if (nfirst > 0) f6_issue_stage(red_rows6, red_aux6, st0, smem, smem + kF6RingOff + (st0 & 3) * kStageAuxBytes, wave, wave_v == kF6NW - 1, dma_off, dma_aux_off);
        if (nfirst > 1) f6_issue_stage(red_rows6, red_aux6, st0 + 1, smem + kStageRowBytes, smem + kF6RingOff + ((st0 + 1) & 3) * kStageAuxBytes, wave, wave_v == kF6NW - 1, dma_off, dma_aux_off);
        if (nfirst > 1) {
            if (wave_v == kF6NW - 1) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(2 * (kDmaPerWave + 1)) : "memory");
            else                   asm volatile("s_waitcnt vmcnt(%0)" :: "n"(2 * kDmaPerWave) : "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        // (no loaded register is read in front of this statement, which stands behind the wait: every later use goes
        // through it.  It is also the use in front of the stage loop: with the first use inside the loop the operand would
        // be assembled there)
#pragma unroll
        for (int j = 0; j < kF6NC; ++j)
            asm volatile("" : "+v"(lo[j][0]), "+v"(hi[j][0]), "+v"(lo[j][1]), "+v"(hi[j][1]), "+v"(stat[j]));
#pragma unroll
        for (int j = 0; j < kF6NC; ++j)
            if (cb + 32 * j + r32 >= ncols_pad) {
                lo[j][0] = lo[j][1] = v4i{0, 0, 0, 0};
                hi[j][0] = hi[j][1] = v2i_6{0, 0};
            }
#pragma unroll
        for (int j = 0; j < kF6NC; ++j) {
            const int n = cb + 32 * j + r32;
            thr[j] = n < ncols ? fp6_threshold_acc(fp6_threshold(stat[j][0], stat[j][1], stat[j][2], um, em, dstar)) : kF6Never;
#pragma unroll
            for (int h = 0; h < 2; ++h)
                bf[j][h] = v8i_6{lo[j][h][0], lo[j][h][1], lo[j][h][2], lo[j][h][3], hi[j][h][0], hi[j][h][1], 0, 0};
        }
    }

    // per-lane LDS offsets of the streamed fragments (the two 16-byte pieces of slot 2 h + hs, swizzled as staged)
    const int sw = (r32 >> 1) & 7;
    int aoff0[2], aoff1[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        aoff0[h] = r32 * kDim + 16 * ((2 * (2 * h + hs)) ^ sw);
        aoff1[h] = r32 * kDim + 16 * ((2 * (2 * h + hs) + 1) ^ sw);
    }

    // stage st becomes readable in buffer BUF; the DMA of stage st + 2 goes where stage st - 1 was (every wave has the whole
    // of that stage in registers or behind it: its reads are waited for in front of the barrier).  The starts go to slot
    // stage & 3 of a ring of FOUR: the last unit of stage st - 1 is multiplied behind this hand-over and may still read its
    // starts, and the slot the DMA of stage st + 2 takes is that of stage st - 2, whose last unit every wave finished in
    // front of this barrier.
    auto hand_over = [&](auto buf_tag, int st) F6_INLINE {
        constexpr int BUF = decltype(buf_tag)::value;
        // stage st's DMA was issued two hand-overs ago; only the DMA of stage st + 1 may still be in flight (a wave that
        // flushed its records since has drained its vector memory counter there, which only makes this wait a no-op)
        if (st + 1 < st1) {
            if (wave_v == kF6NW - 1) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(kDmaPerWave + 1) : "memory");
            else                   asm volatile("s_waitcnt vmcnt(%0)" :: "n"(kDmaPerWave) : "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        if (st + 2 < st1)
            f6_issue_stage(red_rows6, red_aux6, st + 2, smem + ((BUF + 2) % 3) * kStageRowBytes, smem + kF6RingOff + ((st + 2) & 3) * kStageAuxBytes, wave, wave_v == kF6NW - 1, dma_off, dma_aux_off);
    };

    auto read_unit = [&](F6Unit& x, const char* buf, int u) F6_INLINE {
        const char* rows = buf + 32 * u * kDim;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const v4i   lo = *(const v4i*)(rows + aoff0[h]);
            const v2i_6 hi = *(const v2i_6*)(rows + aoff1[h]);       // the 8 real bytes of the second piece
            x.a[h] = __builtin_shufflevector(__builtin_shufflevector(lo, lo, 0, 1, 2, 3, -1, -1, -1, -1),
                                             __builtin_shufflevector(hi, hi, 0, 1, -1, -1, -1, -1, -1, -1), 0, 1, 2, 3, 8, 9, -1, -1);
        }
    };

    // A wave's records wait in a private list in LDS behind the stage buffers until the list is full or the sweep ends:
    // nothing reads them before the kernel has ended (the rescoring folds with an atomic minimum, in any order), and a
    // global atomic inside the loop makes the wave, and at the next barrier the workgroup, wait for an L2 round trip.
    // `nrec`, the list's fill, is wave-uniform.  The flush reserves the records on the pair's counter with one atomic,
    // copies them out and drains the vector memory counter: the hand-over waits count on the LDS-DMA being this wave's
    // newest vector memory operations.  No barrier: only this wave touches its list.
    // The lane's number where the cold paths need it (hit path, flush): two instructions there instead of lane constants
    // (lane half, row of the block, output row) that would hold registers across the whole loop.  (volatile: not hoisted)
    auto lane_id = [&]() F6_INLINE {
        unsigned l;
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
        return l;
    };
    const uint2* const hits = (const uint2*)(smem + kF6HitsOff) + wave * kF6HitSlots;
    const unsigned hits_lds = (unsigned)(uintptr_t)F6_LDS_PTR(hits);
    unsigned nrec = 0;
    auto flush = [&]() F6_INLINE {
        const unsigned lane = lane_id();
        unsigned base = 0;
        if (lane == 0) base = atomicAdd(cnt, nrec);
        base = (unsigned)__builtin_amdgcn_readfirstlane((int)base);
#pragma unroll
        for (int k = 0; k < kF6HitSlots / 64; ++k) {
            const unsigned i = (unsigned)(64 * k + lane);
            if (i < nrec) {
                const uint2 r = hits[i];
                if (base + i < cap) rec[base + i] = r;
                else                cnt[1] = 1u;
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        nrec = 0;
    };

    // The accumulators start at ZERO (the instruction's inline constant: no C operand is read for the first K-half), so a
    // block's maximum lacks the rows' start values.  It is screened against thr_s[j] = thr[j] - (the largest start of the
    // unit's STAGE), rounded down (fp6_filter.h): nothing the exact test keeps fails that.  Only where a lane of the wave
    // passes the screen (`pass`, the wave's ballot) does a block read the lane's 16 starts -- slot (stage & 3) of the ring,
    // `xs` the byte offset of the unit's 32 starts in the kernel's LDS -- and repeat the test on acc + start, which is the
    // accumulator a start value in the C operand would have given, bit for bit (every partial sum is exact).
    // (both halves of the wave hold candidates of an output row: a row may be listed twice for a unit, which the
    // rescoring's atomic minimum does not mind)
    v16f_6 acc[kF6NC];
#pragma unroll
    for (int j = 0; j < kF6NC; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = kFp6PadInit;
    auto test_block = [&](auto j_tag, unsigned long long pass, unsigned unit, int xs) F6_INLINE {
        constexpr int j = decltype(j_tag)::value;
        if (pass == 0ull) return;
        const unsigned l = lane_id(), hs = l >> 5;
        // the lane's 16 starts: rows (r & 3) + 8 (r >> 2) + 4 hs of the unit, four 16-byte reads (two addresses per
        // wave: broadcasts)
        float emax = kFp6PadInit;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const v4f_6 s = *(const v4f_6*)(smem + xs + 16 * hs + 32 * q);
#pragma unroll
            for (int k = 0; k < 4; ++k) emax = fmaxf(emax, acc[j][4 * q + k] + s[k]);
        }
        const bool hit = emax >= thr[j];
        const unsigned long long m = __builtin_amdgcn_ballot_w64(hit);
        if (m == 0ull) return;
        const unsigned pc = (unsigned)__popcll(m);
        if (nrec + pc > (unsigned)kF6HitSlots) flush();
        const unsigned rank = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
        // (LDS only: the hand-over's lgkmcnt(0) covers the write, which touches no stage buffer.  As a statement of
        // its own: in front of a store to LDS the compiler waits for vmcnt(0), the LDS-DMA being a pending LDS write)
        if (hit) {
            // (bit 31 of the unit word: which 16 of the unit's rows this lane's accumulators are)
            const unsigned long long r = ((unsigned long long)(unit | (hs << 31)) << 32) | (unsigned)(cb + 32 * j + (l & 31));
            asm volatile("ds_write_b64 %0, %1" :: "v"(hits_lds + 8u * (nrec + rank)), "v"(r) : "memory");
        }
        nrec += pc;
    };

    float thr_s[kF6NC];
#pragma unroll
    for (int j = 0; j < kF6NC; ++j) thr_s[j] = kF6Never;
    float smax = 0.f;
    std::integral_constant<int, 0> b0;  std::integral_constant<int, 1> b1;  std::integral_constant<int, 2> b2;
    std::integral_constant<int, 3> b3;

    // One unit in two halves, each one basic block of four instructions that ends in its own branch.  The max trees and
    // compares stand BETWEEN a half's matrix instructions, on accumulators those do not write: a wave's own vector
    // instructions issue beside its matrix instruction in flight, while behind a burst of eight they waited for the
    // SIMD's other wave.  Half 1 multiplies blocks 0, 1 of unit `unit` and tests blocks 2, 3 of the unit before it
    // (`punit`, starts at `pxs`), whose accumulators half 2 then overwrites; half 2 multiplies blocks 2, 3 and tests blocks
    // 0, 1 of `unit`, with the reads of the next unit (`y`) among them.  The compiler cannot count LDS reads while an
    // LDS-DMA is in flight -- its wait in front of a unit's first instruction is lgkmcnt(0) -- so those reads stay behind
    // that wait; they have the rest of half 2 to land.
    // thr_s is a STAGE's value and a unit's blocks are tested at two times.  The first unit behind a hand-over is the last
    // one of the stage before: its blocks 0, 1 are tested in that multiply's half 2 and its blocks 2, 3 in half 1 of the
    // next.  `smax_tag`: the wave reads the stage's largest start at ring offset `smax_off` beside the next unit's reads and
    // moves thr_s[0], thr_s[1] to it behind this unit's second test; `late_tag`: thr_s[2], thr_s[3] follow behind the first
    // test of this multiply.
    auto multiply = [&](const F6Unit& x, unsigned unit, int xs, unsigned punit, int pxs, F6Unit& y, const char* ybuf, auto yu_tag,
                        auto smax_tag, auto late_tag, int smax_off) F6_INLINE {
        const v16f_6 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        // K-half major: the two instructions of a block are two apart
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int j = 0; j < 2; ++j)
                acc[j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(x.a[h], bf[j][h], h == 0 ? zero : acc[j], 2, 2, 0, 0, 0, 0);
        const unsigned long long p2 = __builtin_amdgcn_ballot_w64(f6_max16(acc[2]) >= thr_s[2]);
        const unsigned long long p3 = __builtin_amdgcn_ballot_w64(f6_max16(acc[3]) >= thr_s[3]);
        F6_MFMA_THEN_VALU(5); F6_MFMA_THEN_VALU(5); F6_MFMA_THEN_VALU(5); F6_MFMA_THEN_VALU(3);
        if ((p2 | p3) != 0ull) {
            test_block(b2, p2, punit, pxs);
            test_block(b3, p3, punit, pxs);
        }
        if constexpr (decltype(late_tag)::value) f6_screen2(thr_s[2], thr_s[3], thr[2], thr[3], smax);
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int j = 2; j < 4; ++j)
                acc[j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(x.a[h], bf[j][h], h == 0 ? zero : acc[j], 2, 2, 0, 0, 0, 0);
        if constexpr (decltype(yu_tag)::value >= 0) read_unit(y, ybuf, decltype(yu_tag)::value);
        float sm = 0.f;
        if constexpr (decltype(smax_tag)::value) sm = *(const float*)(smem + smax_off);
        const unsigned long long p0 = __builtin_amdgcn_ballot_w64(f6_max16(acc[0]) >= thr_s[0]);
        const unsigned long long p1 = __builtin_amdgcn_ballot_w64(f6_max16(acc[1]) >= thr_s[1]);
        __builtin_amdgcn_sched_group_barrier(0x8, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x2, 5, 0);
        F6_MFMA_THEN_VALU(5); F6_MFMA_THEN_VALU(5); F6_MFMA_THEN_VALU(3);
        if ((p0 | p1) != 0ull) {
            test_block(b0, p0, unit, xs);
            test_block(b1, p1, unit, xs);
        }
        if constexpr (decltype(smax_tag)::value) {
            smax = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, sm)));
            f6_screen2(thr_s[0], thr_s[1], thr[0], thr[1], smax);
        }
    };

    // The two register sets: even and odd units of a stage.  The last unit of a stage is multiplied behind the NEXT hand-over,
    // so a wave enters the barrier with that unit's reads issued a unit earlier and leaves it with work in registers; in
    // front of the first stage its place is taken by a unit of zero codes, screened against "never" (thr_s above), and the
    // first test of all finds the accumulators' preset values, which "never" holds back as well.
    F6Unit ua, ub;
    ub.a[0] = ub.a[1] = v8i_6{0, 0, 0, 0, 0, 0, 0, 0};
    std::integral_constant<int, 0> u0;  std::integral_constant<int, 1> u1;  std::integral_constant<int, 2> u2;
    std::integral_constant<int, 3> u3;  std::integral_constant<int, -1> none;
    std::true_type yes;  std::false_type no;
    auto stage = [&](auto buf_tag, int st) F6_INLINE {
        constexpr int BUF = decltype(buf_tag)::value;
        const char* buf = smem + BUF * kStageRowBytes;
        const unsigned unit0 = (unsigned)(st * kF6Units);
        // the starts of this stage's units and of the stage before: its unit 2 is tested in the first half behind the
        // hand-over, its unit 3, carried in, in the two halves after that -- the slot is intact until the next hand-over
        const int xs = kF6RingOff + (st & 3) * kStageAuxBytes, xp = kF6RingOff + ((st - 1) & 3) * kStageAuxBytes;
        hand_over(buf_tag, st);
        multiply(ub, unit0 - 1, xp + 384, unit0 - 2, xp + 256, ua, buf, u0, yes, no, xs + 4 * kF6SmaxWord);
        multiply(ua, unit0,     xs,       unit0 - 1, xp + 384, ub, buf, u1, no, yes, 0);
        multiply(ub, unit0 + 1, xs + 128, unit0,     xs,       ua, buf, u2, no, no, 0);
        multiply(ua, unit0 + 2, xs + 256, unit0 + 1, xs + 128, ub, buf, u3, no, no, 0);
    };

    if (st0 >= st1) return;
    for (int st = st0; st < st1; st += 3) {
        stage(std::integral_constant<int, 0>{}, st);
        if (st + 1 < st1) stage(std::integral_constant<int, 1>{}, st + 1);
        if (st + 2 < st1) stage(std::integral_constant<int, 2>{}, st + 2);
    }
    {
        const unsigned last = (unsigned)(st1 * kF6Units) - 1u;
        const int xl = kF6RingOff + ((st1 - 1) & 3) * kStageAuxBytes;
        multiply(ub, last, xl + 384, last - 1u, xl + 256, ua, smem, none, no, no, 0);
        // the drain: blocks 2, 3 of the last unit
        const unsigned long long p2 = __builtin_amdgcn_ballot_w64(f6_max16(acc[2]) >= thr_s[2]);
        const unsigned long long p3 = __builtin_amdgcn_ballot_w64(f6_max16(acc[3]) >= thr_s[3]);
        test_block(b2, p2, last, xl + 384);
        test_block(b3, p3, last, xl + 384);
    }
    if (nrec != 0u) flush();
}

// One wave per record: exact int32 d2 of the output row against the 16 streamed rows whose accumulators the recording lane
// held -- rows (r & 3) + 8 (r >> 2) + 4 half of the unit, r = 0 .. 15, half = bit 31 of the record's unit word -- from the
// int8 plane and its norms as K1 computes it (lane l: row r = l & 15, K-quarter l >> 4); the best (d2, row) below D* goes
// into slice 0 of `partial`.  The other 16 rows of the unit are not read: a candidate among them made its own lane fire, and
// the launch is bound by the bytes it reads, not by latency (387 076 records of the flagship step x 32 rows are 1.6 GB in
// 0.26 ms; several records in flight per wave did not shorten it).
__global__ __launch_bounds__(256)
void rescore6_kernel(F6Batch b)
{
    const int lane = threadIdx.x & 63;
    const unsigned wave = (blockIdx.x * 256u + threadIdx.x) >> 6, nwaves = gridDim.x * 4u;
    for (int pi = 0; pi < b.n; ++pi) {
        const F6Params& p = b.p[pi];
        if (p.cnt[1] != 0u) continue;                 // K1 redoes the pair
        unsigned n = p.cnt[0];
        n = n < p.cap ? n : p.cap;
        const unsigned dstar = *p.cut;
        for (unsigned r = wave; r < n; r += nwaves) {
            const uint2 rc = p.rec[r];
            const int c = (int)rc.x;
            const int rr = lane & 15, kq = lane >> 4;
            const int m = (int)((rc.y & 0x7fffffffu) * 32u) + (rr & 3) + 8 * (rr >> 2) + 4 * (int)(rc.y >> 31);
            // (m < n_pad of the streamed bank: the unit was staged from it)
            const int8_t* a = p.col_rows8 + (size_t)c * kDim + 32 * kq;
            const int8_t* y = p.red_rows8 + (size_t)m * kDim + 32 * kq;
            int dot = 0;
#pragma unroll
            for (int w = 0; w < 2; ++w) {
                const v4i x = *(const v4i*)(a + 16 * w);
                const v4i z = *(const v4i*)(y + 16 * w);
#pragma unroll
                for (int k = 0; k < 4; ++k) dot = __builtin_amdgcn_sdot4(x[k], z[k], dot, false);
            }
            dot += __shfl_xor(dot, 16);
            dot += __shfl_xor(dot, 32);
            const unsigned d2 = (unsigned)(p.col_norm[c] + p.red_norm[m] - 2 * dot);
            unsigned long long key = (m < p.nred && d2 < dstar) ? ((unsigned long long)d2 << 32) | (unsigned)m : ~0ull;
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) {
                const unsigned long long other = __shfl_xor(key, o);
                key = other < key ? other : key;
            }
            if (lane == 0 && key != ~0ull) atomicMin(p.partial + c, key);
        }
    }
}

// The FP6 plane of the rows [0, n_pad) of an integer-route bank from its int8 plane (rows8 = uint8 ^ 0x80): 4 threads per
// row, one K-chunk each, a workgroup per 128-row stage.  aux6[stage][128] takes the largest accumulator start among the
// stage's real rows (kFp6PadInit where it has none): the sweep's screen (fp6_screen_threshold).  max6 ([2], zeroed by the caller) takes the bank's largest |m|^2 and |m - m^|^2.
__global__ __launch_bounds__(256)
void prep6_kernel(const int8_t* __restrict__ rows8, int64_t n, int64_t n_pad, uint8_t* __restrict__ rows6,
                  float* __restrict__ aux6, int32_t* __restrict__ stat6, int32_t* __restrict__ max6)
{
    __shared__ uint8_t code[256];
    code[threadIdx.x] = (uint8_t)fp6_code((int)threadIdx.x);
    __syncthreads();
    __shared__ int stage_min[4];
    const int k = threadIdx.x & 3;
    int umax = 0, emax = 0;
    // a workgroup takes whole stages, 64 rows at a time (n_pad is a multiple of the stage), and leaves the largest start of
    // the stage's real rows -- the start of their least |m|^2 -- in the word behind the stage's starts
    int smin = INT32_MAX;
    for (int64_t i = 0; ; ++i) {
        const int64_t st = (i >> 1) * gridDim.x + blockIdx.x;
        if (st >= n_pad / kStageRows) break;
        const int64_t row = st * kStageRows + (i & 1) * 64 + (threadIdx.x >> 2);
        unsigned w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        int usq = 0, hsq = 0, esq = 0;
        if (row < n) {
            const uint4 lo = *(const uint4*)(rows8 + row * kDim + 32 * k), hi = *(const uint4*)(rows8 + row * kDim + 32 * k + 16);
            const unsigned src[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
            unsigned long long bits = 0;       // codes enter at the top of what is left, words leave at the bottom
            int have = 0, out = 0;
#pragma unroll
            for (int i = 0; i < 32; ++i) {
                const int v = (int)(((src[i >> 2] >> (8 * (i & 3))) & 0xffu) ^ 0x80u);
                const int cd = code[v], x = fp6_value32(cd);
                usq += v * v; hsq += x * x; esq += (v - x) * (v - x);
                bits |= (unsigned long long)cd << have;
                have += 6;
                if (have >= 32) { w[out++] = (unsigned)bits; bits >>= 32; have -= 32; }
            }
        }
        *(uint4*)(rows6 + row * kDim + 32 * k)      = make_uint4(w[0], w[1], w[2], w[3]);
        *(uint4*)(rows6 + row * kDim + 32 * k + 16) = make_uint4(w[4], w[5], w[6], w[7]);
        usq += __shfl_xor(usq, 1); usq += __shfl_xor(usq, 2);
        hsq += __shfl_xor(hsq, 1); hsq += __shfl_xor(hsq, 2);
        esq += __shfl_xor(esq, 1); esq += __shfl_xor(esq, 2);
        if (k == 0) {
            *(int4*)(stat6 + 4 * row) = make_int4(usq, hsq, esq, 0);
            const int64_t r = row % kStageRows;
            aux6[st * 256 + r] = row < n ? fp6_acc_init(usq) : kFp6PadInit;
            if (r != 0) aux6[st * 256 + kStageRows + r] = 0.f;
        }
        umax = max(umax, usq);
        emax = max(emax, esq);
        if (row < n) smin = min(smin, usq);
        if (i & 1) {           // (the trip count is the workgroup's: every thread is here)
            for (int o = 32; o > 0; o >>= 1) smin = min(smin, __shfl_xor(smin, o));
            if ((threadIdx.x & 63) == 0) stage_min[threadIdx.x >> 6] = smin;
            __syncthreads();
            if (threadIdx.x == 0) {
                const int m = min(min(stage_min[0], stage_min[1]), min(stage_min[2], stage_min[3]));
                aux6[st * 256 + kStageRows] = m != INT32_MAX ? fp6_acc_init(m) : kFp6PadInit;
            }
            __syncthreads();
            smin = INT32_MAX;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        umax = max(umax, __shfl_xor(umax, o));
        emax = max(emax, __shfl_xor(emax, o));
    }
    if ((threadIdx.x & 63) == 0) {
        if (umax > 0) atomicMax(max6, umax);
        if (emax > 0) atomicMax(max6 + 1, emax);
    }
}

hipError_t launch_prep6(const Bank& b, int grid_max, hipStream_t stream)
{
    hipError_t e = hipMemsetAsync(b.max6, 0, 8, stream);
    if (e != hipSuccess) return e;
    int64_t grid = b.n_pad / kStageRows;            // a workgroup per stage
    if (grid_max > 0 && grid > grid_max) grid = grid_max;
    hipLaunchKernelGGL(prep6_kernel, dim3((unsigned)grid), dim3(256), 0, stream, (const int8_t*)b.rows8, b.n, b.n_pad,
                       b.rows6, b.aux6, b.stat6, b.max6);
    return hipGetLastError();
}

bool filter6_usable(const Bank& cols, const Bank& red)
{
    return cols.kind == FM_BANK_I8 && red.kind == FM_BANK_I8 && cols.dim == kDim && red.dim == kDim &&
           cols.rows6 && red.rows6 && cols.rows8 && red.rows8;
}

// The filter sweep and the rescoring of n pairs, pair i under plans[i] (K1's batched shape: the layout of its keys) with the
// list ws.rec + i * ws.cap and the words ws.cnt + 2 i ([0] count, [1] need_k1, zeroed here).  The streamed banks are split
// by the filter's own rule for the launch as a whole (fp6_plan.h) unless ws.nsplit forces a count or K1's.  The guarded K1
// launch follows in launch_rowreduce_batch.
hipError_t launch_filter6(int n, const Bank* const* cols, const Bank* const* red, const RowReducePlan* plans,
                          unsigned long long* const* partial, const unsigned* const* cut, const Filter6Ws& ws, hipStream_t stream)
{
    if (n < 1 || n > kRRBatchMax) return hipErrorInvalidValue;
    uint2* const rec = ws.rec;  const unsigned cap = ws.cap;  unsigned* const cnt = ws.cnt;
    F6Batch b;
    long long total = 0;
    Fp6PlanPair pp[kRRBatchMax];
    for (int i = 0; i < n; ++i) pp[i] = Fp6PlanPair{(plans[i].nchunks + 1) / 2, (int)(red[i]->n_pad / kStageRows)};
    const int L = ws.nsplit == 0 ? fp6_plan_stages(pp, n, ws.resident, kFp6PlanOverhead) : 0;
    for (int i = 0; i < n; ++i) {
        const RowReducePlan& pl = plans[i];
        if (pl.nb != 4 || pl.nw != 8 || !filter6_usable(*cols[i], *red[i]) || !cut[i]) return hipErrorInvalidValue;
        F6Params& p = b.p[i];
        p.col_rows6 = cols[i]->rows6;  p.col_stat = cols[i]->stat6;  p.ncols = (int)cols[i]->n;  p.ncols_pad = (int)cols[i]->n_pad;
        p.red_rows6 = red[i]->rows6;   p.red_aux6 = red[i]->aux6;    p.red_max = red[i]->max6;
        p.nstages = (int)(red[i]->n_pad / kStageRows);
        p.nsplit = pl.nsplit;  p.nchunks = pl.nchunks;  p.stages_per_split = pl.stages_per_split;  p.ncols_alloc = pl.ncols_alloc;
        if (ws.nsplit < 0)      { p.nsplit_f = pl.nsplit;  p.stages_per_split_f = pl.stages_per_split; }
        else if (ws.nsplit > 0) fp6_plan_split_forced(p.nstages, ws.nsplit, &p.nsplit_f, &p.stages_per_split_f);
        else                    fp6_plan_split(p.nstages, L, &p.nsplit_f, &p.stages_per_split_f);
        p.partial = partial[i];  p.cut = cut[i];
        p.rec = rec + (size_t)i * cap;  p.cap = cap;  p.cnt = cnt + 2 * i;
        p.col_rows8 = cols[i]->rows8;  p.col_norm = cols[i]->norm;  p.red_rows8 = red[i]->rows8;  p.red_norm = red[i]->norm;
        p.nred = (int)red[i]->n;
        b.first_block[i] = (int)total;
        total += (long long)((pl.nchunks + 1) / 2) * p.nsplit_f;     // a workgroup takes two of K1's chunks
    }
    if (total > INT32_MAX) return hipErrorInvalidValue;
    for (int i = n; i < kRRBatchMax; ++i) b.p[i] = b.p[0];
    b.first_block[n] = (int)total;
    for (int i = n + 1; i <= kRRBatchMax; ++i) b.first_block[i] = INT32_MAX;
    b.n = n;
    hipError_t e = hipMemsetAsync(cnt, 0, (size_t)n * 8, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(filter6_kernel, dim3((unsigned)total), dim3(64 * kF6NW), 0, stream, b);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipStream_t tail = stream;
    if (ws.side) {          // the rescoring beside whatever follows the sweep on its stream
        if ((e = hipEventRecord(ws.ev_sweep, stream)) != hipSuccess || (e = hipStreamWaitEvent(ws.side, ws.ev_sweep, 0)) != hipSuccess) return e;
        tail = ws.side;
    }
    hipLaunchKernelGGL(rescore6_kernel, dim3(1024), dim3(256), 0, tail, b);
    return hipGetLastError();
}

}  // namespace fm
