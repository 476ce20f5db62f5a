// K11 -- cv2.BFMatcher(NORM_HAMMING) on binary descriptors (ORB / BRIEF / BRISK / FREAK / AKAZE rows of 1 .. 64 bytes).
// The reference matches SIFT only, but leaves room for other detectors (get_features(data, feature_type), matchutil.py:31);
// binary descriptors are the other half of cv2.BFMatcher use.  Contract: cv::batchDistance with dtype CV_32S --
// h(q, t) = popcount(q XOR t), candidates ordered by (h, index), strict insertion in ascending index (the earlier row wins a tie).
//
// Matrix-core route (knnMatch k = 1, 2; the reverse direction of crossCheck).  Every descriptor bit becomes one FP4 (e2m1)
// value: 1 -> +1.0 (nibble 0x2), 0 -> -1.0 (0xA), width padding -> 0.  The dot product of two encoded rows is then
//   sum over the W real bits of (+-1)(+-1) = (W - h) - h = W - 2 h,
// every partial sum an integer of magnitude <= 512, so the f32 accumulator of v_mfma_scale_f32_16x16x128_f8f6f4 (FP4
// operands, unit E8M0 scales) is exact in any summation order and h = (W - dot) / 2.  No row norms are needed.  A 256-bit
// ORB row is 128 FP4 bytes, the size of a SIFT int8 row: one 16 x 16 tile costs two MFMAs, like K1's two 16x16x64_i8.
//   Operand lane map: lane l supplies row (l & 15), bytes 16 (l >> 4) .. + 15 of each 64-byte K step, for BOTH operands;
//   whatever k order the instruction assigns to those bytes, it is the same for A and B, and a dot product does not depend
//   on the order of its terms.  A = the reduced-over rows (D row i = 4 (l >> 4) + reg), B = the output rows (D column
//   l & 15): a lane holds 4 candidates of one output row per tile.
//   In-lane top-K without index bookkeeping in the loop: the accumulator is initialised with (31 - p) / 32, p = 4 tile +
//   reg the candidate's position among the lane's 32 of a 128-row stage (exact: an integer <= 512 plus a multiple of
//   1/32).  The largest value of a stage is then the largest dot product and, among equal ones, the lowest position =
//   the lowest row; floor() is the dot product, the fraction names the row.  Across stages a strict compare on the
//   integer part keeps the earlier row.  The lane groups of an output row and the splits of the reduced range are
//   merged on 64-bit keys (float32 bits of h << 32 | row), lexicographic, so every tie goes to the lowest index.
//   Padded rows (an all-zero FP4 row is at h = W / 2 from everything) are excluded by index, never by value.
// partial[(split * ncols_alloc + c) * KTOP + k] = those keys, ascending, ~0 = none: the layout knn2_merge_kernel and
// xcheck_scatter_kernel (api_match.hip) read on the float32 route -- the high word is the float32 bits of the distance.
//
// Hamming self distances (fm_hamming_self_dist(_batch)): ham_self_kernel, the top-1 sweep of a bank against itself with the
// diagonal dropped, many banks per launch -- described where it stands, behind launch_hamming.
//
// k = 3 .. 8: a vector-ALU kernel in K9's shape (one query row per thread, train rows staged through LDS and read as
// broadcasts, XOR + popcount on the packed rows, knnk_insert), merged by K9's merge kernel.  Off the hot path.
#include "tile_ops.h"

#include <algorithm>
#include <type_traits>

namespace fm {

typedef int v8i_h __attribute__((ext_vector_type(8)));
typedef float v4f_h __attribute__((ext_vector_type(4)));

constexpr int kHamNB = 4;                 // blocks of 16 output rows per wave
constexpr int kHamNW = 4;                 // waves per workgroup
constexpr int kHamChunk = 16 * kHamNB * kHamNW;    // output rows per workgroup (256)

// ---- bank preparation -----------------------------------------------------------------------------------------------------
// One thread per (row, byte of the padded packed width wb; source rows `pitch` bytes apart): packed[row][byte] (0 beyond the row's bytes or rows) and the
// byte's four FP4 bytes: bit j -> nibble j (0x2 for 1, 0xA for 0), padding -> 0.
__global__ __launch_bounds__(256)
void ham_prep_kernel(const uint8_t* __restrict__ src, int64_t pitch, int64_t n, int bytes, int wb, int64_t n_pad,
                     uint8_t* __restrict__ packed, uint32_t* __restrict__ fp4)
{
    const int64_t total = n_pad * wb;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i / wb;
        const int c = (int)(i % wb);
        const bool real = row < n && c < bytes;
        const unsigned v = real ? src[row * pitch + c] : 0u;
        uint32_t w = 0;
        if (real) {
#pragma unroll
            for (int j = 0; j < 8; ++j) w |= ((v >> j) & 1u ? 0x2u : 0xAu) << (4 * j);
        }
        packed[i] = (uint8_t)v;
        fp4[i] = w;                     // (row stride 4 wb bytes = KSTEPS * 64)
    }
}

hipError_t launch_hamming_prep(const uint8_t* d_src, int64_t n, int bytes, const Bank& b, hipStream_t stream, int64_t pitch)
{
    if (pitch == 0) pitch = bytes;
    const int wb = b.ksteps * 16;
    const int64_t total = b.n_pad * wb;
    const int64_t grid = std::min<int64_t>(4096, (total + 255) / 256);
    hipLaunchKernelGGL(ham_prep_kernel, dim3((unsigned)grid), dim3(256), 0, stream, d_src, pitch, n, bytes, wb, b.n_pad, b.rowsb,
                       (uint32_t*)b.rows4);
    return hipGetLastError();
}

// ---- the matrix-core sweep --------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long ham_key(float dot, int idx, int W)
{
    if (idx < 0) return ~0ull;
    const int h = (W - (int)dot) >> 1;
    return ((unsigned long long)__float_as_uint((float)h) << 32) | (unsigned)idx;
}

template <int KTOP, int KS>
__global__ __launch_bounds__(256)
void ham_sweep_kernel(const uint8_t* __restrict__ col4, int ncols, const uint8_t* __restrict__ red4, int nred, int W,
                      int nchunks, int stages_per_split, int nstages, int ncols_alloc, unsigned long long* __restrict__ partial,
                      const int* __restrict__ stage_real = nullptr)
{
    // stage_real (train collections, api_collection.hip): the reduced bank holds many images, each from a stage of its own;
    // stage_real[st] = real rows of stage st, the rows behind them are padding -- the index mask of the tail, per stage
    constexpr int RB = KS * 64;             // FP4 bytes per row
    constexpr int LS = RB + 16;             // LDS row stride: the 16 rows of one 16-lane read land on distinct banks
    constexpr int PIECES = kStageRows * RB / 16 / 256;    // 16-byte pieces per thread per stage (2 KS)
    __shared__ __attribute__((aligned(16))) uint8_t lds[2][kStageRows * LS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4;
    const int chunk = blockIdx.x % nchunks, split = blockIdx.x / nchunks;
    const int st0 = split * stages_per_split, st1 = min(nstages, st0 + stages_per_split);

    // the wave's output rows, in registers (rows beyond the bank's real rows: zero operands, never merged)
    v8i_h bop[kHamNB][KS];
#pragma unroll
    for (int b = 0; b < kHamNB; ++b) {
        const int c = chunk * kHamChunk + wave * 16 * kHamNB + 16 * b + (lane & 15);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const v4i x = c < ncols ? *(const v4i*)(col4 + (size_t)c * RB + 64 * ks + 16 * g) : v4i{0, 0, 0, 0};
            bop[b][ks] = v8i_h{x[0], x[1], x[2], x[3], 0, 0, 0, 0};
        }
    }
    // per block: the best (integer dot, row) so far; KTOP = 2 also the second
    float bd0[kHamNB], bd1[kHamNB];
    int bi0[kHamNB], bi1[kHamNB];
#pragma unroll
    for (int b = 0; b < kHamNB; ++b) { bd0[b] = -INFINITY; bd1[b] = -INFINITY; bi0[b] = -1; bi1[b] = -1; }

    v4i pre[PIECES];
    auto load = [&](int st) {
#pragma unroll
        for (int i = 0; i < PIECES; ++i) {
            const int p = tid + 256 * i;
            pre[i] = *(const v4i*)(red4 + ((size_t)st * kStageRows) * RB + (size_t)p * 16);
        }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int i = 0; i < PIECES; ++i) {
            const int p = tid + 256 * i;
            const int r = p / (RB / 16), c = p % (RB / 16);
            *(v4i*)(&lds[buf][r * LS + 16 * c]) = pre[i];
        }
    };
    if (st0 < st1) { load(st0); store(0); }
    __syncthreads();
    for (int st = st0; st < st1; ++st) {
        const int buf = (st - st0) & 1;
        const bool more = st + 1 < st1;
        if (more) load(st + 1);
        const int sbase = st * kStageRows;
        const int lim = stage_real ? sbase + stage_real[st] : nred;
        const bool tail = sbase + kStageRows > lim;         // the bank's (an image's) last stage: rows from lim on are padding
        float m1[kHamNB], m2[kHamNB];
#pragma unroll
        for (int b = 0; b < kHamNB; ++b) { m1[b] = -INFINITY; m2[b] = -INFINITY; }
#pragma unroll
        for (int t = 0; t < kStageRows / 16; ++t) {
            v8i_h aop[KS];
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const v4i x = *(const v4i*)(&lds[buf][(16 * t + (lane & 15)) * LS + 64 * ks + 16 * g]);
                aop[ks] = v8i_h{x[0], x[1], x[2], x[3], 0, 0, 0, 0};
            }
            const v4f_h cinit = {(31 - 4 * t) * (1.f / 32), (30 - 4 * t) * (1.f / 32), (29 - 4 * t) * (1.f / 32), (28 - 4 * t) * (1.f / 32)};
#pragma unroll
            for (int b = 0; b < kHamNB; ++b) {
                v4f_h acc = cinit;
#pragma unroll
                for (int ks = 0; ks < KS; ++ks)
                    acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(aop[ks], bop[b][ks], acc, 4, 4, 0, 127, 0, 127);
                if (tail) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[r] = (sbase + 16 * t + 4 * g + r < lim) ? acc[r] : -INFINITY;
                }
                if constexpr (KTOP == 1) {
                    m1[b] = fmaxf(fmaxf(m1[b], acc[0]), acc[1]);
                    m1[b] = fmaxf(fmaxf(m1[b], acc[2]), acc[3]);
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {       // running top-2 of distinct values: (max, median of three)
                        m2[b] = __builtin_amdgcn_fmed3f(m1[b], m2[b], acc[r]);
                        m1[b] = fmaxf(m1[b], acc[r]);
                    }
                }
            }
        }
        // the stage's best (and second) against the state: strict on the integer part, the earlier row keeps a tie
        // (a value of -inf -- no candidate -- never passes a strict compare)
#pragma unroll
        for (int b = 0; b < kHamNB; ++b) {
            const float f1 = floorf(m1[b]);
            const int p1 = 31 - (int)((m1[b] - f1) * 32.f);
            const int i1 = sbase + 16 * ((p1 >> 2) & 7) + 4 * g + (p1 & 3);
            if constexpr (KTOP == 1) {
                const bool up = f1 > bd0[b];
                bd0[b] = up ? f1 : bd0[b];
                bi0[b] = up ? i1 : bi0[b];
            } else {
                const float f2 = floorf(m2[b]);
                const int p2 = 31 - (int)((m2[b] - f2) * 32.f);
                const int i2 = sbase + 16 * ((p2 >> 2) & 7) + 4 * g + (p2 & 3);
                const bool first = f1 > bd0[b], enter = f1 > bd1[b], both = f2 > bd0[b];
                const float n1d = first ? (both ? f2 : bd0[b]) : (enter ? f1 : bd1[b]);
                const int n1i = first ? (both ? i2 : bi0[b]) : (enter ? i1 : bi1[b]);
                bd0[b] = first ? f1 : bd0[b];
                bi0[b] = first ? i1 : bi0[b];
                bd1[b] = n1d;
                bi1[b] = n1i;
            }
        }
        if (more) store(buf ^ 1);
        __syncthreads();
    }
    // the four lane groups of an output row, then one write per row and rank
#pragma unroll
    for (int b = 0; b < kHamNB; ++b) {
        unsigned long long k0 = ham_key(bd0[b], bi0[b], W);
        unsigned long long k1 = KTOP == 2 ? ham_key(bd1[b], bi1[b], W) : ~0ull;
#pragma unroll
        for (int sh = 16; sh <= 32; sh <<= 1) {
            const unsigned long long o0 = __shfl_xor(k0, sh);
            if constexpr (KTOP == 1) {
                k0 = o0 < k0 ? o0 : k0;
            } else {
                const unsigned long long o1 = __shfl_xor(k1, sh);
                // the two smallest of two ascending pairs (distinct keys but for ~0)
                const unsigned long long lo0 = k0 < o0 ? k0 : o0;
                const unsigned long long hi0 = k0 < o0 ? o0 : k0;
                const unsigned long long lo1 = k0 < o0 ? k1 : o1;
                k0 = lo0;
                k1 = hi0 < lo1 ? hi0 : lo1;
            }
        }
        const int c = chunk * kHamChunk + wave * 16 * kHamNB + 16 * b + (lane & 15);
        if (g == 0) {
            unsigned long long* o = partial + ((size_t)split * ncols_alloc + c) * KTOP;
            o[0] = k0;
            if constexpr (KTOP == 2) o[1] = k1;
        }
    }
}

HamPlan plan_hamming(int64_t ncols_pad, int64_t nred_pad)
{
    HamPlan p;
    p.nchunks = (int)((ncols_pad + kHamChunk - 1) / kHamChunk);
    p.ncols_alloc = p.nchunks * kHamChunk;
    p.nstages = (int)(nred_pad / kStageRows);
    // ~2048 workgroups on the chip (256 CUs), each at least 4 stages (512 reduced rows) long
    int ns = (2048 + p.nchunks - 1) / p.nchunks;
    const int most = (p.nstages + 3) / 4;
    if (ns > most) ns = most;
    if (ns < 1) ns = 1;
    p.stages_per_split = (p.nstages + ns - 1) / ns;
    p.nsplit = (p.nstages + p.stages_per_split - 1) / p.stages_per_split;
    return p;
}

hipError_t launch_hamming(const Bank& cols, const Bank& red, int ktop, const HamPlan& p, unsigned long long* partial, hipStream_t stream,
                          const int* stage_real)
{
    if (cols.kind != FM_BANK_BIN || red.kind != FM_BANK_BIN || cols.ksteps != red.ksteps || cols.dim != red.dim) return hipErrorInvalidValue;
    const int W = 8 * cols.dim;
    const dim3 grid((unsigned)(p.nchunks * p.nsplit)), block(256);
#define FM_HAM(KT_, KS_)                                                                                                       \
    if (ktop == KT_ && cols.ksteps == KS_) {                                                                                   \
        hipLaunchKernelGGL((ham_sweep_kernel<KT_, KS_>), grid, block, 0, stream, (const uint8_t*)cols.rows4, (int)cols.n,     \
                           (const uint8_t*)red.rows4, (int)red.n, W, p.nchunks, p.stages_per_split, p.nstages, p.ncols_alloc,  \
                           partial, stage_real);                                                                                        \
        return hipGetLastError();                                                                                              \
    }
    FM_HAM(1, 1) FM_HAM(1, 2) FM_HAM(1, 3) FM_HAM(1, 4)
    FM_HAM(2, 1) FM_HAM(2, 2) FM_HAM(2, 3) FM_HAM(2, 4)
#undef FM_HAM
    return hipErrorInvalidValue;
}

// ---- Hamming self distances: the top-1 sweep of a bank against itself, diagonal dropped ----------------------------------
// selfdist[i] = min over j != i of h(i, j): fm_knn2(b, b)'s second column, the value only (cache.pyx:250-252 for L2).  The loop
// is ham_sweep_kernel<1, KS>'s with cols = red = the bank.  In that kernel's lane map acc[r] of tile t is reduced row
// sbase + 16 t + 4 g + r and the lane's output row is c, so the candidate (i, i) sits in ONE 16 x 16 tile per block b of a wave:
// the wave's 64 output rows lie in stage 2 chunk + (wave >> 1), tiles 4 (wave & 1) .. + 3.  Only that stage runs the body with
// the v_cmp / v_cndmask of the diagonal (DIAG); the test is wave-uniform (st, chunk and wave are), every other stage -- all but
// one per wave -- runs K11's unmasked body.  Padding rows stay excluded by index (tail), as in K11.
// One launch covers the banks of a Metric_Cache build (many small images): table[workgroup] = {bank, chunk, split, 0}, the
// banks' arrays and plans in the kernel arguments.  Banks of one KS share a launch; W (bits per row) is per bank.
// (The loop is restated here and not shared with ham_sweep_kernel, which stays as it was built and measured: its prologue reads
// launch arguments where this one reads a table entry and a bank record, and its stage body has no second form.)
template <int KS>
__global__ __launch_bounds__(256)
void ham_self_kernel(HamSelfArgs a, const int4* __restrict__ table)
{
    constexpr int RB = KS * 64;             // FP4 bytes per row
    constexpr int LS = RB + 16;             // LDS row stride (ham_sweep_kernel's)
    constexpr int PIECES = kStageRows * RB / 16 / 256;
    __shared__ __attribute__((aligned(16))) uint8_t lds[2][kStageRows * LS];
    const int4 e = table[blockIdx.x];
    const HamSelfBank& bk = a.b[e.x];
    const uint8_t* __restrict__ rows4 = bk.rows4;
    const int n = bk.n;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4;
    const int chunk = e.y, split = e.z;
    const int st0 = split * bk.plan.stages_per_split, st1 = min(bk.plan.nstages, st0 + bk.plan.stages_per_split);
    const int diag_stage = 2 * chunk + (wave >> 1);

    v8i_h bop[kHamNB][KS];
#pragma unroll
    for (int b = 0; b < kHamNB; ++b) {
        const int c = chunk * kHamChunk + wave * 16 * kHamNB + 16 * b + (lane & 15);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const v4i x = c < n ? *(const v4i*)(rows4 + (size_t)c * RB + 64 * ks + 16 * g) : v4i{0, 0, 0, 0};
            bop[b][ks] = v8i_h{x[0], x[1], x[2], x[3], 0, 0, 0, 0};
        }
    }
    float bd0[kHamNB];
    int bi0[kHamNB];
#pragma unroll
    for (int b = 0; b < kHamNB; ++b) { bd0[b] = -INFINITY; bi0[b] = -1; }

    v4i pre[PIECES];
    auto load = [&](int st) {
#pragma unroll
        for (int i = 0; i < PIECES; ++i) {
            const int p = tid + 256 * i;
            pre[i] = *(const v4i*)(rows4 + ((size_t)st * kStageRows) * RB + (size_t)p * 16);
        }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int i = 0; i < PIECES; ++i) {
            const int p = tid + 256 * i;
            const int r = p / (RB / 16), c = p % (RB / 16);
            *(v4i*)(&lds[buf][r * LS + 16 * c]) = pre[i];
        }
    };
    float m1[kHamNB];
    // one 128-row stage out of LDS buffer `buf` into m1[]; DIAG: the stage holds this wave's diagonal tiles
    auto stage = [&](auto diag, int buf, int sbase, bool tail) {
        constexpr bool DIAG = decltype(diag)::value;
#pragma unroll
        for (int t = 0; t < kStageRows / 16; ++t) {
            v8i_h aop[KS];
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const v4i x = *(const v4i*)(&lds[buf][(16 * t + (lane & 15)) * LS + 64 * ks + 16 * g]);
                aop[ks] = v8i_h{x[0], x[1], x[2], x[3], 0, 0, 0, 0};
            }
            const v4f_h cinit = {(31 - 4 * t) * (1.f / 32), (30 - 4 * t) * (1.f / 32), (29 - 4 * t) * (1.f / 32), (28 - 4 * t) * (1.f / 32)};
#pragma unroll
            for (int b = 0; b < kHamNB; ++b) {
                v4f_h acc = cinit;
#pragma unroll
                for (int ks = 0; ks < KS; ++ks)
                    acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(aop[ks], bop[b][ks], acc, 4, 4, 0, 127, 0, 127);
                if (tail) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[r] = (sbase + 16 * t + 4 * g + r < n) ? acc[r] : -INFINITY;
                }
                if constexpr (DIAG) {
                    // reduced row == output row: 16 t + 4 g + r == 16 (4 (wave & 1) + b) + (lane & 15) inside the stage
                    const int own = 16 * (4 * (wave & 1) + b - t) + (lane & 15) - 4 * g;
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[r] = (own == r) ? -INFINITY : acc[r];
                }
                m1[b] = fmaxf(fmaxf(m1[b], acc[0]), acc[1]);
                m1[b] = fmaxf(fmaxf(m1[b], acc[2]), acc[3]);
            }
        }
    };
    if (st0 < st1) { load(st0); store(0); }
    __syncthreads();
    for (int st = st0; st < st1; ++st) {
        const int buf = (st - st0) & 1;
        const bool more = st + 1 < st1;
        if (more) load(st + 1);
        const int sbase = st * kStageRows;
        const bool tail = sbase + kStageRows > n;
#pragma unroll
        for (int b = 0; b < kHamNB; ++b) m1[b] = -INFINITY;
        if (st == diag_stage) stage(std::true_type{}, buf, sbase, tail);
        else                  stage(std::false_type{}, buf, sbase, tail);
        // (a stage whose every candidate was dropped leaves -inf, which never passes the strict compare)
#pragma unroll
        for (int b = 0; b < kHamNB; ++b) {
            const float f1 = floorf(m1[b]);
            const int p1 = 31 - (int)((m1[b] - f1) * 32.f);
            const int i1 = sbase + 16 * ((p1 >> 2) & 7) + 4 * g + (p1 & 3);
            const bool up = f1 > bd0[b];
            bd0[b] = up ? f1 : bd0[b];
            bi0[b] = up ? i1 : bi0[b];
        }
        if (more) store(buf ^ 1);
        __syncthreads();
    }
#pragma unroll
    for (int b = 0; b < kHamNB; ++b) {
        unsigned long long k0 = ham_key(bd0[b], bi0[b], bk.W);
#pragma unroll
        for (int sh = 16; sh <= 32; sh <<= 1) {
            const unsigned long long o0 = __shfl_xor(k0, sh);
            k0 = o0 < k0 ? o0 : k0;
        }
        const int c = chunk * kHamChunk + wave * 16 * kHamNB + 16 * b + (lane & 15);
        if (g == 0) bk.partial[(size_t)split * bk.plan.ncols_alloc + c] = k0;
    }
}

// out[i] = (double)h of the smallest key over the splits, +inf where there is none; blockIdx.y = the bank of the launch
__global__ __launch_bounds__(256)
void ham_self_merge_kernel(HamSelfArgs a)
{
    const HamSelfBank& bk = a.b[blockIdx.y];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= bk.n) return;
    unsigned long long k = ~0ull;
    for (int s = 0; s < bk.plan.nsplit; ++s) {
        const unsigned long long v = bk.partial[(size_t)s * bk.plan.ncols_alloc + i];
        k = v < k ? v : k;
    }
    bk.out[i] = (k == ~0ull) ? (double)INFINITY : (double)__uint_as_float((unsigned)(k >> 32));
}

hipError_t launch_hamming_self(const HamSelfArgs& a, int nbanks, int ksteps, const void* d_table, int n_workgroups, hipStream_t stream)
{
    if (nbanks < 1 || nbanks > kHamSelfMax || n_workgroups < 1 || !d_table) return hipErrorInvalidValue;
    const dim3 grid((unsigned)n_workgroups), block(256);
    switch (ksteps) {
    case 1: hipLaunchKernelGGL((ham_self_kernel<1>), grid, block, 0, stream, a, (const int4*)d_table); break;
    case 2: hipLaunchKernelGGL((ham_self_kernel<2>), grid, block, 0, stream, a, (const int4*)d_table); break;
    case 3: hipLaunchKernelGGL((ham_self_kernel<3>), grid, block, 0, stream, a, (const int4*)d_table); break;
    case 4: hipLaunchKernelGGL((ham_self_kernel<4>), grid, block, 0, stream, a, (const int4*)d_table); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_hamming_self_merge(const HamSelfArgs& a, int nbanks, hipStream_t stream)
{
    int nmax = 0;
    for (int j = 0; j < nbanks; ++j) nmax = a.b[j].n > nmax ? a.b[j].n : nmax;
    if (nbanks < 1 || nbanks > kHamSelfMax || nmax < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ham_self_merge_kernel, dim3((unsigned)((nmax + 255) / 256), (unsigned)nbanks), dim3(256), 0, stream, a);
    return hipGetLastError();
}

// ---- k = 3 .. 8 on the vector ALUs ------------------------------------------------------------------------------------------
constexpr int kHamKnnStage = 64;         // train rows per LDS stage (64 x at most 64 packed bytes)

// MASKED (K13, masked.hip): the thread's word of the bit mask per 64-row stage, one bit per candidate (as knn_k.hip's kernels).
template <int K, int KS, bool MASKED = false>
__global__ __launch_bounds__(256)
void ham_knnk_kernel(const uint8_t* __restrict__ qrows, int nq, const uint8_t* __restrict__ trows, int nt, int rows_per_split,
                     unsigned long long* __restrict__ partial, const int* __restrict__ stage_real = nullptr,
                     const unsigned long long* __restrict__ mask = nullptr, int64_t mwords = 0)
{
    constexpr int WB = KS * 16;            // packed bytes per row (zero padded)
    __shared__ __attribute__((aligned(16))) uint8_t srow[kHamKnnStage * WB];
    const int tid = threadIdx.x;
    const int q = blockIdx.x * 256 + tid;
    const bool live = q < nq;
    v4i qv[KS];
#pragma unroll
    for (int c = 0; c < KS; ++c) qv[c] = live ? *(const v4i*)(qrows + (size_t)q * WB + 16 * c) : v4i{0, 0, 0, 0};
    unsigned long long keys[K];
#pragma unroll
    for (int i = 0; i < K; ++i) keys[i] = ~0ull;
    const int t0 = blockIdx.y * rows_per_split, t1 = min(nt, t0 + rows_per_split);
    for (int base = t0; base < t1; base += kHamKnnStage) {
        __syncthreads();
        // 64 rows x WB bytes; a stage never reads past the bank's padding (n_pad % 128 == 0, base % 64 == 0)
        for (int p = tid; p < kHamKnnStage * KS; p += 256) {
            const int r = p / KS, c = p % KS;
            *(v4i*)(srow + r * WB + 16 * c) = *(const v4i*)(trows + (size_t)(base + r) * WB + 16 * c);
        }
        __syncthreads();
        int rn = min(kHamKnnStage, t1 - base);
        if (stage_real) rn = min(rn, stage_real[base >> 7] - (base & 127));      // (a collection's stage: see ham_sweep_kernel)
        unsigned long long mw = 0ull;
        if constexpr (MASKED) mw = live ? mask[(size_t)q * mwords + (base >> 6)] : 0ull;
        for (int r = 0; r < rn; ++r) {
            if constexpr (MASKED) { if (!((mw >> r) & 1ull)) continue; }
            int h = 0;
#pragma unroll
            for (int c = 0; c < KS; ++c) {
                const v4i y = *(const v4i*)(srow + r * WB + 16 * c);
#pragma unroll
                for (int w = 0; w < 4; ++w) h += __popc((unsigned)(qv[c][w] ^ y[w]));
            }
            const unsigned long long key = ((unsigned long long)__float_as_uint((float)h) << 32) | (unsigned)(base + r);
            if (key < keys[K - 1]) knnk_insert<K>(keys, key);
        }
    }
    if (live) {
#pragma unroll
        for (int i = 0; i < K; ++i) partial[((size_t)blockIdx.y * nq + q) * K + i] = keys[i];
    }
}

// (partial: knnk_partial_bytes(q.n, t.n, k) bytes -- the split rule of K9)
hipError_t launch_hamming_knnk(const Bank& q, const Bank& t, int k, unsigned long long* partial, int32_t* d_idx, float* d_dist,
                               hipStream_t stream, const int* stage_real, const unsigned long long* mask, int64_t mwords)
{
    if (k < 1 || k > 8 || q.kind != FM_BANK_BIN || t.kind != FM_BANK_BIN || q.ksteps != t.ksteps || q.n <= 0) return hipErrorInvalidValue;
    const int nq = (int)q.n, nt = (int)t.n;
    const int nsplit = knnk_splits(q.n, t.n);
    int per = (nt + nsplit - 1) / nsplit;
    per = (per + kHamKnnStage - 1) / kHamKnnStage * kHamKnnStage;
    if (per < kHamKnnStage) per = kHamKnnStage;
    const dim3 grid((unsigned)((nq + 255) / 256), (unsigned)nsplit);
    bool launched = false;
#define FM_HAMK(K_, KS_)                                                                                                       \
    if (k == K_ && q.ksteps == KS_) {                                                                                          \
        if (mask)                                                                                                              \
            hipLaunchKernelGGL((ham_knnk_kernel<K_, KS_, true>), grid, dim3(256), 0, stream, (const uint8_t*)q.rowsb, nq,      \
                               (const uint8_t*)t.rowsb, nt, per, partial, stage_real, mask, mwords);                          \
        else                                                                                                                   \
            hipLaunchKernelGGL((ham_knnk_kernel<K_, KS_>), grid, dim3(256), 0, stream, (const uint8_t*)q.rowsb, nq,           \
                               (const uint8_t*)t.rowsb, nt, per, partial, stage_real);                                         \
        launched = true;                                                                                                       \
    }
#define FM_HAMK4(K_) FM_HAMK(K_, 1) FM_HAMK(K_, 2) FM_HAMK(K_, 3) FM_HAMK(K_, 4)
    FM_HAMK4(1) FM_HAMK4(2) FM_HAMK4(3) FM_HAMK4(4) FM_HAMK4(5) FM_HAMK4(6) FM_HAMK4(7) FM_HAMK4(8)
#undef FM_HAMK4
#undef FM_HAMK
    if (!launched) return hipErrorInvalidValue;
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_knnk_merge(partial, nsplit, nq, k, d_idx, d_dist, stream);
}

}  // namespace fm
