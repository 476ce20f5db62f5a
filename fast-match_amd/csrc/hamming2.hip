// K11b -- cv2.BFMatcher(NORM_HAMMING2) on binary descriptors whose elements are 2-bit values (ORB with WTA_K = 3 or 4), rows of
// 1 .. 64 bytes.  Contract: cv::normHamming(a, b, n, cellSize = 2) -- h2(q, t) = the number of 2-bit cells of q XOR t that are
// non-zero, a cell being bits 2c, 2c + 1 of a byte; P = 4 bytes cells per row; candidates ordered by (h2, index), strict
// insertion in ascending index (the earlier row wins a tie): K11's rules (hamming.hip) with h2 for h.
//
// Matrix-core route (knnMatch k = 1, 2; the reverse direction of crossCheck; radiusMatch).  A cell (a, b) becomes THREE FP4
// (e2m1) values (s_a, s_b, s_a s_b), s = +1.0 (nibble 0x2) for a 1 bit and -1.0 (0xA) for a 0 bit -- the four vertices of a
// tetrahedron:  00 -> (-,-,+)   01 -> (+,-,-)   10 -> (-,+,-)   11 -> (+,+,+)   (a = bit 2c, the low one).
// Two equal cells add +3 to the dot product of two encoded rows, two different ones -1, whether they differ in one bit or
// both (two vertices of a regular tetrahedron are always at the same angle):
//   dot = 3 (P - h2) - h2 = 3 P - 4 h2,      h2 = (3 P - dot) / 4,
// every partial sum an integer of magnitude <= 768, so the f32 accumulator of v_mfma_scale_f32_16x16x128_f8f6f4 is exact in
// any order, K11's (31 - p) / 32 position fraction included.  A row is 12 bytes FP4 values = 6 bytes FP4 bytes, in
// KS = ceil(12 bytes / 128) K steps of 64 bytes (a 32-byte ORB row: exactly three; 64 bytes: six), width padding 0: half as
// much again as K11's image, not the double of a one-hot code.  Values sit in cell order, a cell's three side by side; the
// order is the same for both operands and a dot product does not depend on the order of its terms.
// Padding rows (an all-zero FP4 row: dot 0, h2 = 3 P / 4 -- the MODE of random data) are excluded by index, never by value.
// Lane map, double-buffered 128-row stages, in-lane top-K by position fraction and the 64-bit keys are K11's, restated here:
// ham_sweep_kernel stays as it was built and measured, and this loop has up to six K steps where that one has four.
// partial[(split * ncols_alloc + c) * KTOP + k]: K11's layout, the high word the float32 bits of h2.
//
// k = 3 .. 8: K11's vector-ALU kernel with popc((x | x >> 1) & 0x55555555) of x = q XOR t on the packed rows, merged by K9's
// merge kernel.  radiusMatch: K10's Hamming route (radius_sweeps.inc) with the threshold dot >= 3 P - 4 H (ham_radius.h),
// launched by radius.hip's r_sweep.
#include "tile_ops.h"
#include "ham_radius.h"

#include <algorithm>

namespace fm {

typedef int v8i_h2 __attribute__((ext_vector_type(8)));
typedef float v4f_h2 __attribute__((ext_vector_type(4)));

constexpr int kHam2NB = 4;                 // blocks of 16 output rows per wave
constexpr int kHam2NW = 4;                 // waves per workgroup
constexpr int kHam2Chunk = 16 * kHam2NB * kHam2NW;    // output rows per workgroup (256): plan_hamming's chunk

// ---- bank preparation -----------------------------------------------------------------------------------------------------
// Two grid-stride passes over a bank (source rows `pitch` bytes apart): packed[row][byte of the padded width wb] (0 beyond the
// row's bytes or rows), and one 32-bit word = 8 FP4 values of the tetrahedral image per work-item: value m of a row is
// component m % 3 of cell m / 3 (byte cell / 4, bits 2 (cell & 3) and + 1); 0 beyond the row's 12 bytes values or rows.
__global__ __launch_bounds__(256)
void ham2_prep_kernel(const uint8_t* __restrict__ src, int64_t pitch, int64_t n, int bytes, int wb, int w4, int64_t n_pad,
                      uint8_t* __restrict__ packed, uint32_t* __restrict__ fp4)
{
    const int64_t total = n_pad * wb;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i / wb;
        const int c = (int)(i % wb);
        packed[i] = (row < n && c < bytes) ? src[row * pitch + c] : (uint8_t)0;
    }
    const int64_t total4 = n_pad * w4;      // (w4 = 16 KS words per row)
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i / w4;
        const int w = (int)(i % w4);
        uint32_t out = 0;
        if (row < n) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int m = 8 * w + j, cell = m / 3, comp = m - 3 * cell, byte = cell >> 2;
                if (byte < bytes) {
                    const unsigned v = src[row * pitch + byte] >> (2 * (cell & 3));
                    const unsigned a = v & 1u, b = (v >> 1) & 1u;
                    const unsigned plus = comp == 0 ? a : comp == 1 ? b : (a ^ b ^ 1u);
                    out |= (plus ? 0x2u : 0xAu) << (4 * j);
                }
            }
        }
        fp4[i] = out;
    }
}

hipError_t launch_hamming2_prep(const uint8_t* d_src, int64_t n, int bytes, const Bank& b, hipStream_t stream, int64_t pitch)
{
    if (b.kind != FM_BANK_BIN2 || b.ksteps != (bytes + 15) / 16 || b.ksteps4 != ham2_fp4_steps(bytes)) return hipErrorInvalidValue;
    if (pitch == 0) pitch = bytes;
    const int wb = b.ksteps * 16, w4 = b.ksteps4 * 16;
    const int64_t total = b.n_pad * w4;
    const int64_t grid = std::min<int64_t>(4096, (total + 255) / 256);
    hipLaunchKernelGGL(ham2_prep_kernel, dim3((unsigned)grid), dim3(256), 0, stream, d_src, pitch, n, bytes, wb, w4, b.n_pad, b.rowsb,
                       (uint32_t*)b.rows4);
    return hipGetLastError();
}

// ---- the matrix-core sweep --------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long ham2_key(float dot, int idx, int P3)
{
    if (idx < 0) return ~0ull;
    const int h2 = (P3 - (int)dot) >> 2;
    return ((unsigned long long)__float_as_uint((float)h2) << 32) | (unsigned)idx;
}

template <int KTOP, int KS>
__global__ __launch_bounds__(256)
void ham2_sweep_kernel(const uint8_t* __restrict__ col4, int ncols, const uint8_t* __restrict__ red4, int nred, int P3,
                       int nchunks, int stages_per_split, int nstages, int ncols_alloc, unsigned long long* __restrict__ partial,
                       const int* __restrict__ stage_real = nullptr)
{
    // stage_real: ham_sweep_kernel's (real rows per stage of a collection's stack); no caller passes one yet
    constexpr int RB = KS * 64;             // FP4 bytes per row
    constexpr int LS = RB + 16;             // LDS row stride: the 16 rows of one 16-lane read land on distinct banks
    constexpr int PIECES = kStageRows * RB / 16 / 256;    // 16-byte pieces per thread per stage (2 KS)
    __shared__ __attribute__((aligned(16))) uint8_t lds[2][kStageRows * LS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4;
    const int chunk = blockIdx.x % nchunks, split = blockIdx.x / nchunks;
    const int st0 = split * stages_per_split, st1 = min(nstages, st0 + stages_per_split);

    // the wave's output rows, in registers (rows beyond the bank's real rows: zero operands, never merged)
    v8i_h2 bop[kHam2NB][KS];
#pragma unroll
    for (int b = 0; b < kHam2NB; ++b) {
        const int c = chunk * kHam2Chunk + wave * 16 * kHam2NB + 16 * b + (lane & 15);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const v4i x = c < ncols ? *(const v4i*)(col4 + (size_t)c * RB + 64 * ks + 16 * g) : v4i{0, 0, 0, 0};
            bop[b][ks] = v8i_h2{x[0], x[1], x[2], x[3], 0, 0, 0, 0};
        }
    }
    // per block: the best (integer dot, row) so far; KTOP = 2 also the second
    float bd0[kHam2NB], bd1[kHam2NB];
    int bi0[kHam2NB], bi1[kHam2NB];
#pragma unroll
    for (int b = 0; b < kHam2NB; ++b) { bd0[b] = -INFINITY; bd1[b] = -INFINITY; bi0[b] = -1; bi1[b] = -1; }

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
        const bool tail = sbase + kStageRows > lim;         // the bank's last stage: rows from lim on are padding
        float m1[kHam2NB], m2[kHam2NB];
#pragma unroll
        for (int b = 0; b < kHam2NB; ++b) { m1[b] = -INFINITY; m2[b] = -INFINITY; }
#pragma unroll
        for (int t = 0; t < kStageRows / 16; ++t) {
            v8i_h2 aop[KS];
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const v4i x = *(const v4i*)(&lds[buf][(16 * t + (lane & 15)) * LS + 64 * ks + 16 * g]);
                aop[ks] = v8i_h2{x[0], x[1], x[2], x[3], 0, 0, 0, 0};
            }
            const v4f_h2 cinit = {(31 - 4 * t) * (1.f / 32), (30 - 4 * t) * (1.f / 32), (29 - 4 * t) * (1.f / 32), (28 - 4 * t) * (1.f / 32)};
#pragma unroll
            for (int b = 0; b < kHam2NB; ++b) {
                v4f_h2 acc = cinit;
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
        for (int b = 0; b < kHam2NB; ++b) {
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
    for (int b = 0; b < kHam2NB; ++b) {
        unsigned long long k0 = ham2_key(bd0[b], bi0[b], P3);
        unsigned long long k1 = KTOP == 2 ? ham2_key(bd1[b], bi1[b], P3) : ~0ull;
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
        const int c = chunk * kHam2Chunk + wave * 16 * kHam2NB + 16 * b + (lane & 15);
        if (g == 0) {
            unsigned long long* o = partial + ((size_t)split * ncols_alloc + c) * KTOP;
            o[0] = k0;
            if constexpr (KTOP == 2) o[1] = k1;
        }
    }
}

static bool ham2_pair_ok(const Bank& a, const Bank& b)
{
    return a.kind == FM_BANK_BIN2 && b.kind == FM_BANK_BIN2 && a.dim == b.dim && a.ksteps == b.ksteps && a.ksteps4 == b.ksteps4 &&
           a.ksteps4 == ham2_fp4_steps(a.dim) && a.rows4 && b.rows4 && a.rowsb && b.rowsb;
}

hipError_t launch_hamming2(const Bank& cols, const Bank& red, int ktop, const HamPlan& p, unsigned long long* partial, hipStream_t stream,
                           const int* stage_real)
{
    if (!ham2_pair_ok(cols, red) || p.ncols_alloc != p.nchunks * kHam2Chunk) return hipErrorInvalidValue;
    const int P3 = 12 * cols.dim;
    const dim3 grid((unsigned)(p.nchunks * p.nsplit)), block(256);
#define FM_HAM2(KT_, KS_)                                                                                                      \
    if (ktop == KT_ && cols.ksteps4 == KS_) {                                                                                  \
        hipLaunchKernelGGL((ham2_sweep_kernel<KT_, KS_>), grid, block, 0, stream, (const uint8_t*)cols.rows4, (int)cols.n,    \
                           (const uint8_t*)red.rows4, (int)red.n, P3, p.nchunks, p.stages_per_split, p.nstages, p.ncols_alloc, \
                           partial, stage_real);                                                                               \
        return hipGetLastError();                                                                                              \
    }
    FM_HAM2(1, 1) FM_HAM2(1, 2) FM_HAM2(1, 3) FM_HAM2(1, 4) FM_HAM2(1, 5) FM_HAM2(1, 6)
    FM_HAM2(2, 1) FM_HAM2(2, 2) FM_HAM2(2, 3) FM_HAM2(2, 4) FM_HAM2(2, 5) FM_HAM2(2, 6)
#undef FM_HAM2
    return hipErrorInvalidValue;
}

// ---- k = 3 .. 8 on the vector ALUs ------------------------------------------------------------------------------------------
constexpr int kHam2KnnStage = 64;         // train rows per LDS stage (64 x at most 64 packed bytes)

// PK: 16-byte pieces of a packed row.  ham_knnk_kernel's loop with the cell count for the bit count.
template <int K, int PK>
__global__ __launch_bounds__(256)
void ham2_knnk_kernel(const uint8_t* __restrict__ qrows, int nq, const uint8_t* __restrict__ trows, int nt, int rows_per_split,
                      unsigned long long* __restrict__ partial)
{
    constexpr int WB = PK * 16;            // packed bytes per row (zero padded)
    __shared__ __attribute__((aligned(16))) uint8_t srow[kHam2KnnStage * WB];
    const int tid = threadIdx.x;
    const int q = blockIdx.x * 256 + tid;
    const bool live = q < nq;
    v4i qv[PK];
#pragma unroll
    for (int c = 0; c < PK; ++c) qv[c] = live ? *(const v4i*)(qrows + (size_t)q * WB + 16 * c) : v4i{0, 0, 0, 0};
    unsigned long long keys[K];
#pragma unroll
    for (int i = 0; i < K; ++i) keys[i] = ~0ull;
    const int t0 = blockIdx.y * rows_per_split, t1 = min(nt, t0 + rows_per_split);
    for (int base = t0; base < t1; base += kHam2KnnStage) {
        __syncthreads();
        // 64 rows x WB bytes; a stage never reads past the bank's padding (n_pad % 128 == 0, base % 64 == 0)
        for (int p = tid; p < kHam2KnnStage * PK; p += 256) {
            const int r = p / PK, c = p % PK;
            *(v4i*)(srow + r * WB + 16 * c) = *(const v4i*)(trows + (size_t)(base + r) * WB + 16 * c);
        }
        __syncthreads();
        const int rn = min(kHam2KnnStage, t1 - base);
        for (int r = 0; r < rn; ++r) {
            int h2 = 0;
#pragma unroll
            for (int c = 0; c < PK; ++c) {
                const v4i y = *(const v4i*)(srow + r * WB + 16 * c);
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    const unsigned x = (unsigned)(qv[c][w] ^ y[w]);
                    h2 += __popc((x | (x >> 1)) & 0x55555555u);
                }
            }
            const unsigned long long key = ((unsigned long long)__float_as_uint((float)h2) << 32) | (unsigned)(base + r);
            if (key < keys[K - 1]) knnk_insert<K>(keys, key);
        }
    }
    if (live) {
#pragma unroll
        for (int i = 0; i < K; ++i) partial[((size_t)blockIdx.y * nq + q) * K + i] = keys[i];
    }
}

// (partial: knnk_partial_bytes(q.n, t.n, k) bytes -- the split rule of K9)
hipError_t launch_hamming2_knnk(const Bank& q, const Bank& t, int k, unsigned long long* partial, int32_t* d_idx, float* d_dist,
                                hipStream_t stream)
{
    if (k < 3 || k > 8 || !ham2_pair_ok(q, t) || q.n <= 0) return hipErrorInvalidValue;
    const int nq = (int)q.n, nt = (int)t.n;
    const int nsplit = knnk_splits(q.n, t.n);
    int per = (nt + nsplit - 1) / nsplit;
    per = (per + kHam2KnnStage - 1) / kHam2KnnStage * kHam2KnnStage;
    if (per < kHam2KnnStage) per = kHam2KnnStage;
    const dim3 grid((unsigned)((nq + 255) / 256), (unsigned)nsplit);
    bool launched = false;
#define FM_HAM2K(K_, PK_)                                                                                                      \
    if (k == K_ && q.ksteps == PK_) {                                                                                          \
        hipLaunchKernelGGL((ham2_knnk_kernel<K_, PK_>), grid, dim3(256), 0, stream, (const uint8_t*)q.rowsb, nq,               \
                           (const uint8_t*)t.rowsb, nt, per, partial);                                                         \
        launched = true;                                                                                                       \
    }
#define FM_HAM2K4(K_) FM_HAM2K(K_, 1) FM_HAM2K(K_, 2) FM_HAM2K(K_, 3) FM_HAM2K(K_, 4)
    FM_HAM2K4(3) FM_HAM2K4(4) FM_HAM2K4(5) FM_HAM2K4(6) FM_HAM2K4(7) FM_HAM2K4(8)
#undef FM_HAM2K4
#undef FM_HAM2K
    if (!launched) return hipErrorInvalidValue;
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_knnk_merge(partial, nsplit, nq, k, d_idx, d_dist, stream);
}

// ---- radiusMatch: K10's Hamming route at the tetrahedral image ----------------------------------------------------------------
constexpr int kR2NB = 4;                    // blocks of 16 query rows per wave
constexpr int kR2QPerWG = 16 * kR2NB * 4;   // query rows per workgroup (radius.hip's kRQPerWG)

__global__ void ham2_radius_limits_kernel(const float* __restrict__ radius, float radius_all, int nq, int P, float* __restrict__ thr)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nq) return;
    thr[i] = ham2_radius_dot_min(ham_radius_limit(radius ? radius[i] : radius_all, P), P);
}

hipError_t launch_hamming2_radius_limits(const float* radius, float radius_all, int nq, int P, float* thr, hipStream_t stream)
{
    hipLaunchKernelGGL(ham2_radius_limits_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, stream, radius, radius_all, nq, P, thr);
    return hipGetLastError();
}

// radius.hip's r_emit, restated for this unit: the hits of one lane for one query block in a 64-row half stage (mask over 16
// candidates: tile tt, register r -> bit 4 tt + r) into the row's segment; the four lanes of one query row take one cursor
// increment together.
__device__ __forceinline__ void ham2_emit(const Ham2RSweep& p, unsigned mask, const unsigned (&hi)[16], int q, bool live, int base, int lane)
{
    const int n = __popc(mask);
    if (!__any(n != 0)) return;
    const int j = lane & 15, g = lane >> 4;
    const int n0 = __shfl(n, j), n1 = __shfl(n, j + 16), n2 = __shfl(n, j + 32), n3 = __shfl(n, j + 48);
    const int tot = n0 + n1 + n2 + n3;
    const int pre = (g > 0 ? n0 : 0) + (g > 1 ? n1 : 0) + (g > 2 ? n2 : 0);
    unsigned b0 = 0;
    if (g == 0 && live && tot > 0) b0 = atomicAdd(&p.cnt[q], (unsigned)tot);
    b0 = __shfl(b0, j);
    if (n == 0) return;
    // (the fill recomputes what the count sweep counted, bit for bit; the segment's end is checked all the same)
    const int64_t s0 = p.off[q] - p.base, s1 = p.off[q + 1] - p.base;
    int64_t at = s0 + b0 + pre;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        if (mask & (1u << c)) {
            const unsigned row = (unsigned)(base + 16 * (c >> 2) + 4 * g + (c & 3));
            if (at < s1) p.keys[at] = ((unsigned long long)hi[c] << 32) | row;
            ++at;
        }
    }
}

// radius_ham_kernel's loop (radius_sweeps.inc) with KS up to 6: a hit is dot >= thr, h2 = (3 P - dot) / 4.  Padding rows sit
// at dot = 0 -- h2 = 3 P / 4, inside any r > 3 P / 4 -- and are kept out by index: rows from nt on never count.
template <bool FILL, int KS>
__global__ __launch_bounds__(256)
void radius_ham2_kernel(Ham2RSweep p)
{
    constexpr int RB = KS * 64;             // FP4 bytes per row
    constexpr int LS = RB + 16;             // LDS row pitch
    constexpr int PIECES = kStageRows * RB / 16 / 256;    // 16-byte pieces per thread per stage (2 KS)
    __shared__ __attribute__((aligned(16))) uint8_t lds[2][kStageRows * LS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
    const int qw = blockIdx.x * kR2QPerWG + wave * 16 * kR2NB;
    const int nstages = (p.nt + kStageRows - 1) / kStageRows;
    const int st0 = blockIdx.y * (p.per / kStageRows), st1 = min(nstages, st0 + p.per / kStageRows);

    v8i_h2 bop[kR2NB][KS];
    float thr[kR2NB];
    unsigned count[kR2NB];
#pragma unroll
    for (int b = 0; b < kR2NB; ++b) {
        const int q = qw + 16 * b + j;
        const bool live = q < p.nq;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const v4i x = live ? *(const v4i*)(p.q4 + (size_t)q * RB + 64 * ks + 16 * g) : v4i{0, 0, 0, 0};
            bop[b][ks] = v8i_h2{x[0], x[1], x[2], x[3], 0, 0, 0, 0};
        }
        thr[b] = live ? p.thr[q] : INFINITY;
        count[b] = 0;
    }

    v4i pre[PIECES];
    auto load = [&](int st) {
#pragma unroll
        for (int i = 0; i < PIECES; ++i)      // (whole stages: st < nstages <= n_pad / 128)
            pre[i] = *(const v4i*)(p.t4 + ((size_t)st * kStageRows) * RB + (size_t)(tid + 256 * i) * 16);
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int i = 0; i < PIECES; ++i) {
            const int pc = tid + 256 * i;
            *(v4i*)(&lds[buf][(pc / (RB / 16)) * LS + 16 * (pc % (RB / 16))]) = pre[i];
        }
    };
    if (st0 < st1) { load(st0); store(0); }
    __syncthreads();
    for (int st = st0; st < st1; ++st) {
        const int buf = (st - st0) & 1;
        const bool more = st + 1 < st1;
        if (more) load(st + 1);
        const int sbase = st * kStageRows;
        const bool tail = sbase + kStageRows > p.nt;
        const int rowlim = p.nt - sbase - 4 * g;     // tail: register r of tile t is a real train row iff 16 t + r < rowlim
#pragma unroll
        for (int half = 0; half < 2; ++half) {       // ham2_emit takes the 16 candidates a lane has in 64 rows
            unsigned mask[kR2NB];
            float dot[FILL ? kR2NB : 1][16];
#pragma unroll
            for (int b = 0; b < kR2NB; ++b) mask[b] = 0;
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) {
                const int t = 4 * half + tt;
                v8i_h2 aop[KS];
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    const v4i x = *(const v4i*)(&lds[buf][(16 * t + j) * LS + 64 * ks + 16 * g]);
                    aop[ks] = v8i_h2{x[0], x[1], x[2], x[3], 0, 0, 0, 0};
                }
#pragma unroll
                for (int b = 0; b < kR2NB; ++b) {
                    v4f_h2 acc = v4f_h2{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int ks = 0; ks < KS; ++ks)
                        acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(aop[ks], bop[b][ks], acc, 4, 4, 0, 127, 0, 127);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        bool hit = acc[r] >= thr[b];
                        if (tail) hit = hit && 16 * t + r < rowlim;
                        if constexpr (FILL) { mask[b] |= hit ? (1u << (4 * tt + r)) : 0u; dot[b][4 * tt + r] = acc[r]; }
                        else count[b] += hit ? 1u : 0u;
                    }
                }
            }
            if constexpr (FILL) {
#pragma unroll
                for (int b = 0; b < kR2NB; ++b) {
                    if (!__any(mask[b] != 0)) continue;
                    unsigned hi[16];
#pragma unroll
                    for (int c = 0; c < 16; ++c) hi[c] = __float_as_uint((float)((p.P3 - (int)dot[b][c]) >> 2));
                    ham2_emit(p, mask[b], hi, qw + 16 * b + j, qw + 16 * b + j < p.nq, sbase + 64 * half, lane);
                }
            }
        }
        if (more) store(buf ^ 1);
        __syncthreads();
    }
    if constexpr (!FILL) {
#pragma unroll
        for (int b = 0; b < kR2NB; ++b) {
            unsigned c = count[b];
            c += __shfl_xor(c, 16);
            c += __shfl_xor(c, 32);
            const int q = qw + 16 * b + j;
            if (g == 0 && q < p.nq && c) atomicAdd(&p.cnt[q], c);
        }
    }
}

// p.per: whole 128-row stages per split; nsplit splits cover the train rows (r_sweep's plan)
hipError_t launch_hamming2_radius(const Ham2RSweep& p, bool fill, int nsplit, hipStream_t stream)
{
    if (p.nq < 1 || nsplit < 1 || p.per < kStageRows || p.per % kStageRows != 0 || !p.q4 || !p.t4 || !p.thr || !p.cnt) return hipErrorInvalidValue;
    if (fill && (!p.off || !p.keys)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((p.nq + kR2QPerWG - 1) / kR2QPerWG), (unsigned)nsplit);
#define FM_RHAM2(KS_)                                                                                       \
    if (p.ks == KS_) {                                                                                      \
        if (fill) hipLaunchKernelGGL((radius_ham2_kernel<true, KS_>), grid, dim3(256), 0, stream, p);       \
        else      hipLaunchKernelGGL((radius_ham2_kernel<false, KS_>), grid, dim3(256), 0, stream, p);      \
        return hipGetLastError();                                                                           \
    }
    FM_RHAM2(1) FM_RHAM2(2) FM_RHAM2(3) FM_RHAM2(4) FM_RHAM2(5) FM_RHAM2(6)
#undef FM_RHAM2
    return hipErrorInvalidValue;
}

}  // namespace fm
