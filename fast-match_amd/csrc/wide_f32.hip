// K14 -- wide float32 banks (FM_BANK_F32W): rows of 129 .. 256 values.  gfx950 only.
//
// The contract is K5's (dist_f32.hip) at the wider row: dist = sqrtf(s), s = fmaf(v_k, v_k, s), v_k = a_k - b_k in float32,
// k ascending over the real dim -- the oracle's order 1 -- and keys (float32 distance bits << 32 | reduced row) per split of the
// reduction range in `partial`, so the merge / election / compaction kernels behind a sweep serve wide banks unchanged.
//
// Planes of a wide bank (Bank::wrows ...; the 128-wide planes of the other kinds stay null):
//   wrows  float32 [n_pad][256]  the rows, ZERO PADDED from dim to 256 and from n to n_pad.  The chain may run past dim: a
//                                padding term is fmaf(+0, +0, s) = s for every s (s starts at +0 and never becomes -0; inf and
//                                NaN stay what they are), so the kernels stop at dim rounded up to their unroll step, not at dim.
//   wrowsh fp16    [n_pad][256]  the rows times 2^kscale (K8's rule: the bank's largest finite magnitude lies in [2^13, 2^14)),
//                                rounded to nearest even
//   normf  float32 [n_pad]       |scaled row|^2 (summed in float64)
//   auxf   float32 [n_pad]       -|scaled row|^2 / 2; padding rows -3.4e38
// Part 1 writes them in two kernels: one pass over the source (host rows staged as a dense float32 matrix, or a device
// tensor of float32 / half / bfloat16 read in place at its pitch, widened exactly) that leaves wrows and the largest finite
// magnitude / the "every value is finite" flag, then the scaled planes from wrows.  Host and device creators run the same
// two kernels on the same values, so they build the same bank bit for bit.
//
// Part 2, wide_exact_kernel: K5's tiling (256 threads, 64 x 64 rows per step, 4 x 4 patch per thread, k-major LDS images);
// the output rows' image holds all 256 k (68 KiB), the reduced rows' is staged in two halves of 128 k (34 KiB) with the
// accumulators carried across, which keeps the chain's order.  Bound: fp32 VALU, 2 ops per pair-dimension.
//
// Part 3, wide_filter_kernel + wide_rescore_kernel: the threshold form (radius_f16_kernel's), with a RUNNING threshold.
// Every wave keeps two blocks of 16 output rows as the B operand of v_mfma_f32_16x16x32_f16 in registers (KS = ceil(dim / 32)
// K steps, 4 VGPRs each: 64 VGPRs at 256-D, which is why it is two blocks and not K8's four) and streams the reduced rows'
// fp16 plane as the A operand straight from memory, one 16-row tile ahead (32 more VGPRs at KS = 8; the four waves of a
// workgroup read the same tiles, so three of four reads hit the cache; no LDS, no barrier).  A lane holds, per block, the
// scores s = q.t 2^(kt - kq) - |t'|^2 / 2 of ONE output row against 4 reduced rows of the tile; d2 = |q'|^2 - 2 s in the
// reduced bank's scale, so a larger score is a nearer row.  It keeps the KTOP best scores it has seen; the KTOP-th best,
// shared after every tile among the 4 lanes that own the same output row (max: any lane's is a valid bound), is the bound B.
// A reduced row whose score reaches B - M is appended to one global list of (output row, reduced row) records; every row of
// the exact top-KTOP is among them (margin below).  Most records are made early in a sweep, against a bound that is
// still poor; every wave leaves its final bound in gbound[output row] (atomic maximum) and wide_rescore_kernel drops the
// records whose score lies below that final bound minus M -- the same test against a better bound -- before it runs the
// exact chain for the rest, one thread per record, and inserts the key into split 0 of `partial` with 64-bit atomic minima -- top-2: the loser of the first
// slot's minimum goes to the second slot's, which leaves the two smallest keys whatever the order of arrival, because no
// (output row, reduced row) pair is recorded twice.  A list that overflows (cap records) sets flag[0] and the exact kernel
// redoes the whole call behind it, K8's protocol (run_flag); the overflow is sticky (64-bit count of reserved slots, a wave
// stops recording once its reservation fails: wide_push), however many records a call would make; there is no per-row rescan: a row that is hard for the
// filter only makes the list longer.  Padding rows are excluded by index.
//
// Margin.  Scores are compared in the reduced bank's scale; q' = 2^kt q, t' = 2^kt t below.  Sources of |s_fp16 - s_real|:
//   * operand rounding: both operands carry a relative error <= 2^-11 (fp16 subnormals: an absolute 2^-25 against a bank whose
//     largest value is >= 2^13, far below everything here), so each product errs by <= (2^-10 + 2^-22) |q'_k t'_k| and the
//     sum by <= 2^-10 |q'||t'| (1 + 2^-12) <= 2^-11 (|q'|^2 + |t'|^2)(1 + 2^-12), whatever the number of terms;
//   * the matrix core's float32 accumulation of n <= 256 exact fp16 products: <= n 2^-24 sum |products| <= 2^-16 |q'||t'|;
//   * -|t'|^2 / 2 rounded to float32 and the final fmaf: 2^-24 (|t'|^2 + |s|).
// So |s_fp16 - s_real| <= E = 2^-11 (1 + 2^-4) (|q'|^2 + max |t'|^2).  The exact chain's d2 differs from the real d2 by
// <= n 2^-24 d2 <= 2^-15 (|q'|^2 + |t'|^2), i.e. 2^-16 (...) in score units, and two d2 that share a float32 root differ by
// 2^-22 relative: both inside the 2^-4 slack as well.  A row x of the exact top-KTOP has s_real(x) >= s_real of the KTOP-th
// best of ANY KTOP rows, so s_fp16(x) >= B - 2 E.  M = 1.25 * 2^-10 * (|q'|^2 + max |t'|^2) against 2 E = 1.0625 * 2^-10 (...):
// K8's constant 1.1 enlarged to 1.25 for the terms that grow with n.
// Banks of different scales: the score is rescaled by 2^(kt - kq) (exact); pairs whose exponents differ by more than 8
// take the exact kernel.
// A view of a wide collection's stack (part 4) uses the STACK's largest scaled squared norm for max |t'|^2 and the stack's one
// scale: the derivation above holds for such a view exactly as for a bank, its "largest value >= 2^13" step included,
// because the stack's scale follows the stack's largest finite magnitude and is never lowered.
// A slot with an operand OUTSIDE the stack (part 5: a query bank against the images of a wide collection) is a bank pair of
// two scales, slot by slot: the outside bank has the scale of its own largest magnitude, fixed at its creation, the view the
// stack's, read at the call.  Each slot carries the exact powers of two that put its output rows' planes into its reduced
// side's scale (cscale, nscale) and its reduced side's largest scaled squared norm -- the stack's for a forward slot (an
// upper bound of the image's, as above), the outside bank's for a reverse slot -- so every term of E is the one derived
// above for "Banks of different scales", per slot; a call whose two exponents differ by more than 8 takes the exact kernel.
//
// Part 4, the table forms of the three kernels: the bodies of parts 2 and 3 (wide_exact_body, wide_filter_body) over a table
// of slots in device memory, one launch per chunk of image pairs (fm_collection_pairs_mutual_ratio).
// Part 5, the table forms with an outside operand (OUT = true): one side of every slot is a bank that is not part of the stack
// (fm_collection_wide_mutual_ratio_each, fm_collection_wide_knn2_each; with KTOP = 1 and reverse slots alone,
// fm_collection_wide_match_accepted_each).
// The SELF forms of the bank-pair kernels (fm_wide_self_dist): one sweep of a bank over itself with the diagonal dropped by
// index (wide_filter_body, wide_rescore_kernel, wide_exact_body).  The margin derivation above is unchanged: the diagonal
// leaves by index, not by value, so every bound is the KTOP-th best score of real OTHER rows and every row of the exact
// top-KTOP over the other rows is recorded against it.
// The parts the masked unit (wide_masked.hip) compiles too -- the parameter structs, wide_load_kmajor, wide_margin, wide_fbits,
// wide_push -- live in wide_parts.h.
#include "wide_parts.h"
#include <algorithm>

namespace fm {

// ---------------------------------------------------------------------------------------
// part 1: preparation
// ---------------------------------------------------------------------------------------
template <int DT>
__device__ __forceinline__ float wide_src_elem(const uint8_t* __restrict__ rowp, int k)
{
    if constexpr (DT == FM_DT_F32) return ((const float*)rowp)[k];
    else if constexpr (DT == FM_DT_F16) return (float)((const _Float16*)rowp)[k];
    else return __uint_as_float((unsigned)((const uint16_t*)rowp)[k] << 16);
}

// wrows from the source; stat[0] = largest finite magnitude (float bits), stat[1] |= 1 if a value is not finite
template <int DT>
__global__ __launch_bounds__(256)
void wide_copy_kernel(const uint8_t* __restrict__ src, int64_t pitch, int64_t n, int dim, float* __restrict__ dst, int64_t n_pad,
                      int* __restrict__ stat)
{
    float m = 0.f;
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_pad * kWideDim; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i >> 8;
        const int k = (int)(i & (kWideDim - 1));
        const float v = (row < n && k < dim) ? wide_src_elem<DT>(src + row * pitch, k) : 0.f;
        dst[i] = v;
        const float a = fabsf(v);
        const bool fin = a <= 3.0e38f;
        bad |= !fin;
        m = fin ? fmaxf(m, a) : m;
    }
#pragma unroll
    for (int mask = 1; mask < 64; mask <<= 1) m = fmaxf(m, __shfl_xor(m, mask));
    if (__builtin_amdgcn_ballot_w64(bad) != 0ull && (threadIdx.x & 63) == 0) atomicOr(stat + 1, 1);
    if ((threadIdx.x & 63) == 0 && m > 0.f) atomicMax(stat, (int)__float_as_uint(m));
}

// the scaled planes from wrows: 32 lanes per row, 8 values per lane; stat[0] = largest |scaled row|^2
__global__ __launch_bounds__(256)
void wide_planes_kernel(const float* __restrict__ rows, int64_t n, int64_t n_pad, int k, uint16_t* __restrict__ rowsh,
                        float* __restrict__ normf, float* __restrict__ auxf, int* __restrict__ stat)
{
    const int64_t row = (int64_t)blockIdx.x * 8 + (threadIdx.x >> 5);
    const int c = threadIdx.x & 31;
    if (row >= n_pad) return;
    const float4 v0 = *(const float4*)(rows + row * kWideDim + 8 * c);
    const float4 v1 = *(const float4*)(rows + row * kWideDim + 8 * c + 4);
    const float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
    unsigned h[8];
    double ss = 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float x = ldexpf(v[i], k);
        const _Float16 hx = (_Float16)x;
        h[i] = (unsigned)__builtin_bit_cast(unsigned short, hx);
        ss += (double)x * (double)x;
    }
    *(uint4*)(rowsh + row * kWideDim + 8 * c) =
        make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
#pragma unroll
    for (int mask = 1; mask < 32; mask <<= 1) ss += __shfl_xor(ss, mask);
    const float nm = (float)ss;
    if (c == 0) {
        normf[row] = row < n ? nm : 0.f;
        auxf[row] = row < n ? -0.5f * nm : -3.4e38f;
    }
    float m = (c == 0 && row < n) ? nm : 0.f;
    m = fmaxf(m, __shfl_xor(m, 32));
    if ((threadIdx.x & 63) == 0 && m > 0.f) atomicMax(stat, (int)__float_as_uint(m));
}

hipError_t launch_wide_copy(const void* src, int dtype, int64_t pitch, int64_t n, int dim, const Bank& b, int* stat, hipStream_t stream)
{
    const dim3 grid((unsigned)std::min<int64_t>(2048, (b.n_pad * kWideDim + 255) / 256));
#define FM_WIDE_COPY(DT_)                                                                                                  \
    case DT_: hipLaunchKernelGGL((wide_copy_kernel<DT_>), grid, dim3(256), 0, stream, (const uint8_t*)src, pitch, n, dim, b.wrows, b.n_pad, stat); break;
    switch (dtype) {
        FM_WIDE_COPY(FM_DT_F32) FM_WIDE_COPY(FM_DT_F16) FM_WIDE_COPY(FM_DT_BF16)
        default: return hipErrorInvalidValue;
    }
#undef FM_WIDE_COPY
    return hipGetLastError();
}

hipError_t launch_wide_planes(const Bank& b, int* stat, hipStream_t stream)
{
    hipLaunchKernelGGL(wide_planes_kernel, dim3((unsigned)(b.n_pad / 8)), dim3(256), 0, stream, (const float*)b.wrows, b.n, b.n_pad, b.kscale,
                       b.wrowsh, b.normf, b.auxf, stat);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// part 2: the exact all-pairs kernel
// ---------------------------------------------------------------------------------------
// (kWTile, kWLd, kWHalf, WideExactParams and wide_load_kmajor: wide_parts.h)
// The body of the exact kernels: 64 output rows (`chunk`) of p's output bank against split `split` of its reduced rows.  The
// bank-pair kernel and the table kernel (part 4) differ only in where p, chunk and split come from.
// SELF (the banks are one bank, fm_wide_self_dist): row n is no candidate of output row n -- dropped by index, like the padding.
// OWN: an instantiation of its own for the top-1 table kernel (wide_exact_table_kernel<1, true>), nothing else.  With ONE
// instantiation wide_exact_body<1> inlined into both that kernel and wide_exact_kernel<1>, hipcc compiled the pair kernel to
// other code than it had (its LDS staging: 2384 -> 2317 instructions, one more VGPR), unmeasured; with two, every kernel that
// existed before the table form keeps its instruction stream (tests/test_wide_fast_host.py pins them).
template <int KTOP, bool SELF = false, bool OWN = false>
__device__ __forceinline__ void wide_exact_body(const WideExactParams& p, int chunk, int split, float* __restrict__ colimg, float* __restrict__ redimg)
{
    const int tid = threadIdx.x;
    const int tn = tid & 15, tm = tid >> 4;
    const int c0 = chunk * kWTile;

    if (c0 < p.ncols_pad) wide_load_kmajor<64>(p.col_rows, c0, p.ncols_pad, 0, colimg, tid);

    float bd[4][KTOP];
    int   bi[4][KTOP];
    float thr[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        thr[i] = INFINITY;
#pragma unroll
        for (int k = 0; k < KTOP; ++k) { bd[i][k] = INFINITY; bi[i][k] = -1; }
    }

    const int s0 = split * p.steps_per_split;
    const int s1 = min(s0 + p.steps_per_split, p.nsteps);
    for (int st = s0; st < s1; ++st) {
        float s[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) s[i][j] = 0.f;
        for (int h = 0; h < 2; ++h) {
            __syncthreads();                                   // previous redimg fully consumed
            wide_load_kmajor<32>(p.red_rows, st * kWTile, p.nred_pad, h * kWHalf, redimg, tid);
            __syncthreads();
            const float* ci = colimg + h * kWHalf * kWLd;
            const int kn = h == 0 ? kWHalf : p.kend - kWHalf;
#pragma unroll 8
            for (int k = 0; k < kn; ++k) {
                const float4 a = *(const float4*)(ci + k * kWLd + 4 * tn);
                const float4 b = *(const float4*)(redimg + k * kWLd + 4 * tm);
                const float av[4] = {a.x, a.y, a.z, a.w};
                const float bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float v = av[i] - bv[j];
                        s[i][j] = __builtin_fmaf(v, v, s[i][j]);
                    }
            }
        }
        const int m0 = st * kWTile + 4 * tm;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float mn = fminf(fminf(s[i][0], s[i][1]), fminf(s[i][2], s[i][3]));
            if (mn <= thr[i]) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int idx = m0 + j;
                    bool cand = idx < p.nred && s[i][j] <= thr[i];
                    if constexpr (SELF) cand = cand && idx != c0 + 4 * tn + i;
                    if (cand) {
                        const float d = sqrtf(s[i][j]);
                        if (d < bd[i][KTOP - 1]) {            // strict: earlier row wins ties
                            if constexpr (KTOP == 2) {
                                if (d < bd[i][0]) { bd[i][1] = bd[i][0]; bi[i][1] = bi[i][0]; bd[i][0] = d; bi[i][0] = idx; }
                                else              { bd[i][1] = d; bi[i][1] = idx; }
                            } else {
                                bd[i][0] = d; bi[i][0] = idx;
                            }
                            const float B = bd[i][KTOP - 1];
                            thr[i] = (B * B) * 1.00000024f;    // d2 > thr  =>  sqrtf(d2) >= B
                        }
                    }
                }
            }
        }
    }

    // merge the 16 threads (tm) that own the same column through LDS (reuse redimg)
    __syncthreads();
    float* md = redimg;                                        // [64 cols][16][KTOP]
    int* mi = (int*)(redimg + kWTile * 16 * KTOP);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int k = 0; k < KTOP; ++k) {
            md[((4 * tn + i) * 16 + tm) * KTOP + k] = bd[i][k];
            mi[((4 * tn + i) * 16 + tm) * KTOP + k] = bi[i][k];
        }
    __syncthreads();
    if (tid < kWTile) {
        const int n = c0 + tid;
        float rd[KTOP]; int ri[KTOP];
#pragma unroll
        for (int k = 0; k < KTOP; ++k) { rd[k] = INFINITY; ri[k] = -1; }
        for (int t = 0; t < 16; ++t)
#pragma unroll
            for (int k = 0; k < KTOP; ++k) {
                const float d = md[(tid * 16 + t) * KTOP + k];
                const int ix = mi[(tid * 16 + t) * KTOP + k];
                if (ix < 0) continue;
                const bool b0 = ri[0] < 0 || d < rd[0] || (d == rd[0] && ix < ri[0]);
                if constexpr (KTOP == 2) {
                    const bool b1 = ri[1] < 0 || d < rd[1] || (d == rd[1] && ix < ri[1]);
                    if (b0) { rd[1] = rd[0]; ri[1] = ri[0]; rd[0] = d; ri[0] = ix; }
                    else if (b1) { rd[1] = d; ri[1] = ix; }
                } else {
                    if (b0) { rd[0] = d; ri[0] = ix; }
                }
            }
        if (n < p.ncols_alloc) {
            unsigned long long* out = p.partial + ((size_t)split * p.ncols_alloc + n) * KTOP;
#pragma unroll
            for (int k = 0; k < KTOP; ++k)
                out[k] = (ri[k] >= 0 && n < p.ncols_pad)
                    ? (((unsigned long long)__float_as_uint(rd[k]) << 32) | (unsigned)ri[k]) : ~0ull;
        }
    }
}

template <int KTOP, bool SELF = false>
__global__ __launch_bounds__(256)
void wide_exact_kernel(WideExactParams p)
{
    __shared__ __attribute__((aligned(16))) float colimg[kWideDim * kWLd];
    __shared__ __attribute__((aligned(16))) float redimg[kWHalf * kWLd];

    if (p.run_flag) {
        if (*p.run_flag == 0) return;                 // the filter's result stands
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd((int*)p.run_flag + 2, 1);
    }
    wide_exact_body<KTOP, SELF>(p, (int)(blockIdx.x / p.nsplit), (int)(blockIdx.x % p.nsplit), colimg, redimg);
}

hipError_t launch_wide_exact(const Bank& cols, const Bank& red, int ktop, const RowReducePlan& plan, unsigned long long* partial,
                             const int* run_flag, hipStream_t stream, bool self)
{
    if (self && (ktop != 1 || cols.wrows != red.wrows)) return hipErrorInvalidValue;
    WideExactParams p;
    p.run_flag = run_flag;
    p.col_rows = cols.wrows;
    p.ncols_pad = (int)cols.n_pad;
    p.red_rows = red.wrows;
    p.nred = (int)red.n;
    p.nsteps = (int)((red.n_pad + kWTile - 1) / kWTile);
    p.nred_pad = (int)red.n_pad;
    p.nsplit = plan.nsplit;
    p.steps_per_split = plan.stages_per_split;
    p.ncols_alloc = plan.ncols_alloc;
    p.kend = (cols.dim + 7) & ~7;
    p.partial = partial;
    const int grid = plan.nchunks * plan.nsplit;
    if (self)           hipLaunchKernelGGL((wide_exact_kernel<1, true>), dim3(grid), dim3(256), 0, stream, p);
    else if (ktop == 1) hipLaunchKernelGGL((wide_exact_kernel<1>), dim3(grid), dim3(256), 0, stream, p);
    else                hipLaunchKernelGGL((wide_exact_kernel<2>), dim3(grid), dim3(256), 0, stream, p);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// part 3: fp16 matrix-core filter + exact rescoring
// ---------------------------------------------------------------------------------------
// (kWFBlocks, kWFCols, WideFilterParams, wide_fbits, wide_bits_f, wide_margin and the record list's wide_pad_chunk / wide_push --
// chunks of 64 slots, sticky overflow -- : wide_parts.h)
// One block's tail of a tile: the tile's scores first into the lane's best, the bound shared among the 4 lanes of the output
// row, THEN the test -- a row is recorded against a bound that already knows its own tile.  MASK: the tile holds the block's
// diagonal (SELF form); lane (lr, lg) holds it in register lr - 4 lg, and it is no candidate.
template <int KTOP, bool MASK>
__device__ __forceinline__ void wide_tile_scores(const w_v4f& acc, const float (&ax)[4], int r0, int col, int lr, int lg, const WideFilterParams& p,
                                                 int rowbase, float (&best)[KTOP], float& bnd, float marg, unsigned& lbase, unsigned& lused)
{
    float sc[4];
    bool real[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        sc[r] = __builtin_fmaf(acc[r], p.cscale, ax[r]);
        real[r] = r0 + r < p.nred && col < p.ncols;
        if constexpr (MASK) real[r] = real[r] && 4 * lg + r != lr;
        if (real[r]) {
            if constexpr (KTOP == 2) {
                if (sc[r] > best[0]) { best[1] = best[0]; best[0] = sc[r]; }
                else if (sc[r] > best[1]) best[1] = sc[r];
            } else {
                if (sc[r] > best[0]) best[0] = sc[r];
            }
        }
    }
    bnd = fmaxf(bnd, best[KTOP - 1]);
    bnd = fmaxf(bnd, __shfl_xor(bnd, 16));
    bnd = fmaxf(bnd, __shfl_xor(bnd, 32));
#pragma unroll
    for (int r = 0; r < 4; ++r) wide_push(real[r] && sc[r] >= bnd - marg, rowbase + col, r0 + r, sc[r], p, lbase, lused);
}

// The body of the filter kernels: the 128 output rows `blk` of p's output bank against split `split` of its reduced rows.
// rowbase: where the output bank's row 0 lies in the row space of gbound and of the records (0 for a bank pair; a slot's
// first row in its chunk for the table kernel, part 4).
// SELF (the banks are one bank, fm_wide_self_dist; KTOP = 1): reduced row n is no candidate of output row n.  Its score is the
// row's maximum (d2 = 0), so it must be gone before it can enter best[] -- in the bound it would shut every real neighbour
// out -- and before it is pushed: it leaves by INDEX, under `real`, with the padding rows.  A block of 16 output rows meets its
// diagonal in ONE 16-row tile (both start on multiples of 16): tile c0 / 16 + b, where lane (lr, lg) holds it in register
// r = lr - 4 lg.  Only that tile takes the masked tail (wide_tile_scores<KTOP, true>); every other tile takes the unmasked
// one, behind a scalar compare of the tile index with the wave's first diagonal tile (read once into a scalar register).
template <int KS, int KTOP, bool SELF = false>
__device__ __forceinline__ void wide_filter_body(const WideFilterParams& p, int blk, int split, int rowbase)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lr = lane & 15, lg = lane >> 4;
    const int c0 = blk * kWFCols + wave * 16 * kWFBlocks;

    w_v8h bq[kWFBlocks][KS];
    float marg[kWFBlocks], bnd[kWFBlocks], best[kWFBlocks][KTOP];
#pragma unroll
    for (int b = 0; b < kWFBlocks; ++b) {
        const int col = c0 + 16 * b + lr;                       // (< the bank's n_pad: a multiple of 128 = kWFCols)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) bq[b][ks] = *(const w_v8h*)(p.colh + (size_t)col * kWideDim + 32 * ks + 8 * lg);
        marg[b] = wide_margin(p.colnorm[col], p.nscale, p.red_nm_max);
        bnd[b] = -INFINITY;
#pragma unroll
        for (int k = 0; k < KTOP; ++k) best[b][k] = -INFINITY;
    }

    const int t0 = split * p.tiles_per_split;
    const int t1 = min(t0 + p.tiles_per_split, p.ntiles);
    unsigned lbase = kWNoChunk, lused = 0;
    [[maybe_unused]] int dtile = 0;                             // SELF: the tile that holds block 0's diagonal (block b: dtile + b)
    if constexpr (SELF) dtile = __builtin_amdgcn_readfirstlane(c0 >> 4);
    w_v8h an[KS];
    if (t0 < t1) {
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) an[ks] = *(const w_v8h*)(p.redh + (size_t)(t0 * 16 + lr) * kWideDim + 32 * ks + 8 * lg);
    }
    for (int t = t0; t < t1; ++t) {
        w_v8h a[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) a[ks] = an[ks];
        if (t + 1 < t1) {
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) an[ks] = *(const w_v8h*)(p.redh + (size_t)((t + 1) * 16 + lr) * kWideDim + 32 * ks + 8 * lg);
        }
        const int r0 = t * 16 + 4 * lg;                         // this lane's 4 reduced rows
        const float4 ax4 = *(const float4*)(p.redaux + r0);
        const float ax[4] = {ax4.x, ax4.y, ax4.z, ax4.w};
#pragma unroll
        for (int b = 0; b < kWFBlocks; ++b) {
            w_v4f acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[ks], bq[b][ks], acc, 0, 0, 0);
            const int col = c0 + 16 * b + lr;
            if constexpr (SELF) {
                // (t and dtile are scalar values: one scalar branch per block and tile, and two copies of the tail)
                if (t == dtile + b) wide_tile_scores<KTOP, true>(acc, ax, r0, col, lr, lg, p, rowbase, best[b], bnd[b], marg[b], lbase, lused);
                else                wide_tile_scores<KTOP, false>(acc, ax, r0, col, lr, lg, p, rowbase, best[b], bnd[b], marg[b], lbase, lused);
            } else {
                // (the same tail, written out: the instantiations without SELF keep the instruction streams they had before
                // the SELF form existed, which a call of wide_tile_scores here does not give them)
                float sc[4];
                bool real[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    sc[r] = __builtin_fmaf(acc[r], p.cscale, ax[r]);
                    real[r] = r0 + r < p.nred && col < p.ncols;
                    if (real[r]) {
                        if constexpr (KTOP == 2) {
                            if (sc[r] > best[b][0]) { best[b][1] = best[b][0]; best[b][0] = sc[r]; }
                            else if (sc[r] > best[b][1]) best[b][1] = sc[r];
                        } else {
                            if (sc[r] > best[b][0]) best[b][0] = sc[r];
                        }
                    }
                }
                bnd[b] = fmaxf(bnd[b], best[b][KTOP - 1]);
                bnd[b] = fmaxf(bnd[b], __shfl_xor(bnd[b], 16));
                bnd[b] = fmaxf(bnd[b], __shfl_xor(bnd[b], 32));
#pragma unroll
                for (int r = 0; r < 4; ++r) wide_push(real[r] && sc[r] >= bnd[b] - marg[b], rowbase + col, r0 + r, sc[r], p, lbase, lused);
            }
        }
    }
    wide_pad_chunk(lbase, lused, p);
    // the bound this wave ended with, for the rescoring's second look at the records
    if (lg == 0) {
#pragma unroll
        for (int b = 0; b < kWFBlocks; ++b)
            if (bnd[b] > -INFINITY) atomicMax(p.gbound + rowbase + c0 + 16 * b + lr, wide_fbits(bnd[b]));
    }
}

template <int KS, int KTOP, bool SELF = false>
__global__ __launch_bounds__(256)
void wide_filter_kernel(WideFilterParams p)
{
    wide_filter_body<KS, KTOP, SELF>(p, (int)(blockIdx.x / p.nsplit), (int)(blockIdx.x % p.nsplit), 0);
}

struct WideRescoreParams {
    const float* col_rows; const float* red_rows; int dim;
    const uint2* list; const float* lscore; unsigned cap; const unsigned long long* cnt;
    const unsigned* gbound; const float* colnorm; float nscale, red_nm_max;
    unsigned long long* partial;      // split 0: [ncols_alloc][KTOP]
    int* flag;                        // [0] = 1: the list overflowed, the exact kernel redoes the call
};

// SELF: a record (i, i) is never inserted (the filter's SELF form makes none; the rescoring does not rely on it).
template <int KTOP, bool SELF = false>
__global__ __launch_bounds__(256)
void wide_rescore_kernel(WideRescoreParams p)
{
    const unsigned long long n64 = *p.cnt;
    const unsigned n = (unsigned)n64;
    if (n64 > p.cap) {
        if (blockIdx.x == 0 && threadIdx.x == 0) p.flag[0] = 1;
        return;
    }
    for (unsigned e = blockIdx.x * 256 + threadIdx.x; e < n; e += gridDim.x * 256) {
        const uint2 rec = p.list[e];
        if (rec.x == kWNoRecord) continue;                      // the padding of a chunk
        if constexpr (SELF) { if (rec.x == rec.y) continue; }
        // most records were made against a bound of the sweep's first tiles: the output row's final bound drops them
        if (p.lscore[e] < wide_bits_f(p.gbound[rec.x]) - wide_margin(p.colnorm[rec.x], p.nscale, p.red_nm_max)) continue;
        const float4* a = (const float4*)(p.col_rows + (size_t)rec.x * kWideDim);
        const float4* b = (const float4*)(p.red_rows + (size_t)rec.y * kWideDim);
        float s = 0.f;
        const int k4n = (p.dim + 3) >> 2;                       // (zero padding past dim: see the file comment)
        for (int k4 = 0; k4 < k4n; ++k4) {
            const float4 x = a[k4], y = b[k4];
            float v = x.x - y.x; s = __builtin_fmaf(v, v, s);
            v = x.y - y.y; s = __builtin_fmaf(v, v, s);
            v = x.z - y.z; s = __builtin_fmaf(v, v, s);
            v = x.w - y.w; s = __builtin_fmaf(v, v, s);
        }
        const float d = sqrtf(s);
        if (!(d < INFINITY)) continue;                          // K5's rule: an infinite or NaN distance is no candidate
        const unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | rec.y;
        unsigned long long* out = p.partial + (size_t)rec.x * KTOP;
        const unsigned long long old = atomicMin(out, key);
        if constexpr (KTOP == 2) atomicMin(out + 1, old > key ? old : key);
    }
}

bool wide_filter_usable(const Bank& cols, const Bank& red)
{
    if (!cols.filt_ok || !red.filt_ok || !cols.wrowsh || !red.wrowsh) return false;
    const int dk = red.kscale - cols.kscale;
    return dk >= -8 && dk <= 8;
}

WideFilterPlan plan_wide_filter(int64_t ncols_pad, int64_t ncols, int64_t nred_pad, const Tuning& tn)
{
    WideFilterPlan pl;
    pl.nchunks = (int)((ncols_pad + kWFCols - 1) / kWFCols);
    pl.ntiles = (int)(nred_pad / 16);
    // a split starts with an empty bound and records its first tile whole: at least 64 tiles (1024 rows) per split
    int64_t nsplit = (512 + pl.nchunks - 1) / pl.nchunks;
    if (nsplit > pl.ntiles / 64) nsplit = pl.ntiles / 64;
    if (tn.f32_nsplit > 0) nsplit = tn.f32_nsplit;
    if (nsplit > pl.ntiles) nsplit = pl.ntiles;
    if (nsplit < 1) nsplit = 1;
    pl.tiles_per_split = (int)((pl.ntiles + nsplit - 1) / nsplit);
    pl.nsplit = (pl.ntiles + pl.tiles_per_split - 1) / pl.tiles_per_split;
    int64_t cap = 256 * ncols;                                  // (a multiple of the chunk)
    if (cap < (1 << 20)) cap = 1 << 20;
    if (cap > (1 << 24)) cap = 1 << 24;
    pl.cap = (unsigned)cap;
    return pl;
}

template <int KS, int KTOP, bool SELF = false>
static void wide_filter_launch(const WideFilterParams& p, int grid, hipStream_t stream)
{
    hipLaunchKernelGGL((wide_filter_kernel<KS, KTOP, SELF>), dim3(grid), dim3(256), 0, stream, p);
}

hipError_t launch_wide_filter(const Bank& cols, const Bank& red, int ktop, const WideFilterPlan& plan, uint2* list, float* lscore,
                              unsigned* gbound, unsigned long long* cnt, int* flag, unsigned long long* partial, hipStream_t stream, bool self)
{
    if (self && (ktop != 1 || cols.wrows != red.wrows)) return hipErrorInvalidValue;
    WideFilterParams p;
    p.colh = cols.wrowsh; p.colnorm = cols.normf; p.ncols = (int)cols.n;
    p.redh = red.wrowsh; p.redaux = red.auxf; p.nred = (int)red.n;
    const int dk = red.kscale - cols.kscale;
    p.cscale = ldexpf(1.f, dk);
    p.nscale = ldexpf(1.f, 2 * dk);
    p.red_nm_max = red.nm_max;
    p.ntiles = plan.ntiles; p.tiles_per_split = plan.tiles_per_split; p.nsplit = plan.nsplit;
    p.list = list; p.lscore = lscore; p.cap = plan.cap; p.cnt = cnt; p.gbound = gbound;
    const int grid = plan.nchunks * plan.nsplit;
    const int ks = (cols.dim + 31) / 32;
    if (ks < 5 || ks > 8) return hipErrorInvalidValue;
#define FM_WIDE_F(KS_)                                                                            \
    case KS_: if (self) wide_filter_launch<KS_, 1, true>(p, grid, stream);                        \
              else if (ktop == 1) wide_filter_launch<KS_, 1>(p, grid, stream); else wide_filter_launch<KS_, 2>(p, grid, stream); break;
    switch (ks) { FM_WIDE_F(5) FM_WIDE_F(6) FM_WIDE_F(7) FM_WIDE_F(8) }
#undef FM_WIDE_F
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_wide_rescore(cols, red, ktop, plan.cap, list, lscore, gbound, cnt, flag, partial, stream, self);
}

// The rescoring alone, behind a filter that left its records in `list`: launch_wide_filter's, and the masked filter's
// (wide_masked.hip), which records permitted pairs only and so needs no rescoring of its own.
hipError_t launch_wide_rescore(const Bank& cols, const Bank& red, int ktop, unsigned cap, const uint2* list, const float* lscore,
                               const unsigned* gbound, const unsigned long long* cnt, int* flag, unsigned long long* partial, hipStream_t stream,
                               bool self)
{
    if ((ktop != 1 && ktop != 2) || (self && ktop != 1)) return hipErrorInvalidValue;
    WideRescoreParams r;
    r.col_rows = cols.wrows; r.red_rows = red.wrows; r.dim = cols.dim;
    r.list = list; r.lscore = lscore; r.cap = cap; r.cnt = cnt; r.partial = partial; r.flag = flag;
    r.gbound = gbound; r.colnorm = cols.normf; r.nscale = ldexpf(1.f, 2 * (red.kscale - cols.kscale)); r.red_nm_max = red.nm_max;
    if (self)           hipLaunchKernelGGL((wide_rescore_kernel<1, true>), dim3(2048), dim3(256), 0, stream, r);
    else if (ktop == 1) hipLaunchKernelGGL((wide_rescore_kernel<1>), dim3(2048), dim3(256), 0, stream, r);
    else                hipLaunchKernelGGL((wide_rescore_kernel<2>), dim3(2048), dim3(256), 0, stream, r);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// part 4: the table forms (fm_collection_pairs_mutual_ratio on a wide collection)
// ---------------------------------------------------------------------------------------
// A chunk of image pairs of ONE stack (a wide collection: every image a bank view that starts on a 128-row stage) in one
// launch per step.  A slot (WideSlot) is one direction of one pair; the slots of a chunk lie side by side in the chunk's
// output-row space (slot s owns the rows [row0, row0 + pad128(ncols))), which indexes gbound, partial and the records'
// output rows, so ONE record list, ONE 64-bit count and ONE overflow flag serve the chunk: reservation, padding and the
// sticky overflow are wide_push's, unchanged.  A record is (chunk row, row INSIDE the reduced image): the key the rescoring
// inserts carries the row the caller sees.  The grids are flat; a workgroup finds its slot with table_slot_of over a prefix
// array in device memory (the filter: first workgroups, one entry more than slots; the exact kernel and the rescoring: the
// first rows, which ascend the same way).
// Both operands of every slot are views of the one stack, so they share its scale (cscale = nscale = 1) and the margin takes
// the STACK's largest scaled squared norm for max |t'|^2: an upper bound of the image's, so 2 E <= M holds as derived in the
// file comment, and the stack's largest scaled value lies in [2^13, 2^14) or above whichever image is swept (the scale only
// ever follows the running maximum upwards), which is all the fp16-subnormal step asks: the derivation holds for a view
// exactly as for a bank.
// ---------------------------------------------------------------------------------------
// part 5: the table forms with an outside operand (a wide query bank against the images of a wide collection)
// ---------------------------------------------------------------------------------------
// The same three kernels, instantiated with OUT = true: ONE operand of every slot is a bank outside the stack, with planes,
// scale and largest norm of its own -- the table parameters carry two plane sets, WideSlot::outside says which side takes the
// second one (its first row is 0 there), and the slot carries the two exact scale factors and the reduced side's largest
// scaled squared norm, which feed the filter body, the rescoring's second look and nothing else (the exact chain reads the
// float32 rows alone).  A forward slot (output rows = the query's, reduced = image i) leaves keys whose low word is the row
// inside image i, a reverse slot keys whose low word is the query row: the merge, join, scan and compaction behind the sweeps
// serve unchanged.  All of it derives from the slot, which is the workgroup's (blockIdx.x): base pointers and scales stay in
// scalar registers; the rescoring finds a record's slot per lane, as part 4's does.
struct WideTableParams {
    const WideSlot* slots; const int* wg0; const int* rowp; int n;        // the chunk's table
    const float* rows; const uint16_t* rowsh; const float* normf; const float* auxf;   // the stack's planes
    const float* orows; const uint16_t* orowsh; const float* onormf; const float* oauxf;   // part 5: the outside bank's (else null)
    float nm_max; int dim;
    uint2* list; float* lscore; unsigned cap; unsigned long long* cnt; unsigned* gbound;
    unsigned long long* partial;      // [chunk rows][KTOP]
    int* flag;                        // the rescoring: [0] = 1, the list overflowed
    const int* run_flag;              // the exact kernel: null, or skip unless *run_flag != 0 (runs counted in run_flag[2])
};

template <int KS, int KTOP, bool OUT>
__global__ __launch_bounds__(256)
void wide_filter_table_kernel(WideTableParams t)
{
    const int s = table_slot_of(t.wg0, t.n, (int)blockIdx.x);
    const WideSlot sl = t.slots[s];
    const int local = (int)blockIdx.x - t.wg0[s];
    WideFilterParams p;
    if constexpr (OUT) {
        // (the slot is the workgroup's: the choice of a plane set and the slot's scales are scalar values)
        const bool oc = sl.outside == kWideOutCols, orr = sl.outside == kWideOutRed;
        p.colh = (oc ? t.orowsh : t.rowsh) + (size_t)sl.col0 * kWideDim; p.colnorm = (oc ? t.onormf : t.normf) + sl.col0;
        p.redh = (orr ? t.orowsh : t.rowsh) + (size_t)sl.red0 * kWideDim; p.redaux = (orr ? t.oauxf : t.auxf) + sl.red0;
        p.cscale = sl.cscale; p.nscale = sl.nscale; p.red_nm_max = sl.red_nm_max;
    } else {
        p.colh = t.rowsh + (size_t)sl.col0 * kWideDim; p.colnorm = t.normf + sl.col0;
        p.redh = t.rowsh + (size_t)sl.red0 * kWideDim; p.redaux = t.auxf + sl.red0;
        p.cscale = 1.f; p.nscale = 1.f; p.red_nm_max = t.nm_max;
    }
    p.ncols = sl.ncols; p.nred = sl.nred;
    p.ntiles = sl.ntiles; p.tiles_per_split = sl.tiles_per_split; p.nsplit = sl.nsplit;
    p.list = t.list; p.lscore = t.lscore; p.cap = t.cap; p.cnt = t.cnt; p.gbound = t.gbound;
    wide_filter_body<KS, KTOP>(p, local / sl.nsplit, local % sl.nsplit, sl.row0);
}

template <int KTOP, bool OUT>
__global__ __launch_bounds__(256)
void wide_rescore_table_kernel(WideTableParams t)
{
    const unsigned long long n64 = *t.cnt;
    const unsigned n = (unsigned)n64;
    if (n64 > t.cap) {
        if (blockIdx.x == 0 && threadIdx.x == 0) t.flag[0] = 1;
        return;
    }
    for (unsigned e = blockIdx.x * 256 + threadIdx.x; e < n; e += gridDim.x * 256) {
        const uint2 rec = t.list[e];
        if (rec.x == kWNoRecord) continue;                      // the padding of a chunk of the list
        const int s = table_slot_of(t.rowp, t.n, (int)rec.x);
        const WideSlot sl = t.slots[s];
        const size_t col = (size_t)sl.col0 + (rec.x - (unsigned)sl.row0), red = (size_t)sl.red0 + rec.y;
        const float4* a; const float4* b;
        if constexpr (OUT) {
            const bool oc = sl.outside == kWideOutCols, orr = sl.outside == kWideOutRed;
            if (t.lscore[e] < wide_bits_f(t.gbound[rec.x]) - wide_margin((oc ? t.onormf : t.normf)[col], sl.nscale, sl.red_nm_max)) continue;
            a = (const float4*)((oc ? t.orows : t.rows) + col * kWideDim);
            b = (const float4*)((orr ? t.orows : t.rows) + red * kWideDim);
        } else {
            if (t.lscore[e] < wide_bits_f(t.gbound[rec.x]) - wide_margin(t.normf[col], 1.f, t.nm_max)) continue;
            a = (const float4*)(t.rows + col * kWideDim);
            b = (const float4*)(t.rows + red * kWideDim);
        }
        float s2 = 0.f;
        const int k4n = (t.dim + 3) >> 2;                       // (zero padding past dim: see the file comment)
        for (int k4 = 0; k4 < k4n; ++k4) {
            const float4 x = a[k4], y = b[k4];
            float v = x.x - y.x; s2 = __builtin_fmaf(v, v, s2);
            v = x.y - y.y; s2 = __builtin_fmaf(v, v, s2);
            v = x.z - y.z; s2 = __builtin_fmaf(v, v, s2);
            v = x.w - y.w; s2 = __builtin_fmaf(v, v, s2);
        }
        const float d = sqrtf(s2);
        if (!(d < INFINITY)) continue;                          // K5's rule: an infinite or NaN distance is no candidate
        const unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | rec.y;
        unsigned long long* out = t.partial + (size_t)rec.x * KTOP;
        const unsigned long long old = atomicMin(out, key);
        if constexpr (KTOP == 2) atomicMin(out + 1, old > key ? old : key);
    }
}

// Workgroup b: the 64 chunk rows from 64 b on, the whole reduced image of their slot (one split).
template <int KTOP, bool OUT>
__global__ __launch_bounds__(256)
void wide_exact_table_kernel(WideTableParams t)
{
    __shared__ __attribute__((aligned(16))) float colimg[kWideDim * kWLd];
    __shared__ __attribute__((aligned(16))) float redimg[kWHalf * kWLd];

    if (t.run_flag) {
        if (*t.run_flag == 0) return;                 // the filter's result stands
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd((int*)t.run_flag + 2, 1);
    }
    const int row = (int)blockIdx.x * kWTile;
    const int s = table_slot_of(t.rowp, t.n, row);
    const WideSlot sl = t.slots[s];
    WideExactParams p;
    const float* crows = t.rows;
    const float* rrows = t.rows;
    if constexpr (OUT) {
        if (sl.outside == kWideOutCols) crows = t.orows;
        if (sl.outside == kWideOutRed) rrows = t.orows;
    }
    p.col_rows = crows + (size_t)sl.col0 * kWideDim;
    p.ncols_pad = (sl.ncols + kStageRows - 1) / kStageRows * kStageRows;
    p.red_rows = rrows + (size_t)sl.red0 * kWideDim;
    p.nred = sl.nred;
    p.nred_pad = (sl.nred + kStageRows - 1) / kStageRows * kStageRows;
    p.nsteps = p.nred_pad / kWTile;
    p.nsplit = 1;
    p.steps_per_split = p.nsteps;
    p.ncols_alloc = p.ncols_pad;
    p.kend = (t.dim + 7) & ~7;
    p.partial = t.partial + (size_t)sl.row0 * KTOP;
    p.run_flag = nullptr;
    wide_exact_body<KTOP, false, KTOP == 1>(p, (row - sl.row0) / kWTile, 0, colimg, redimg);
}

static WideTableParams wide_table_params(const Bank& stack, const WideTableLaunch& tl)
{
    WideTableParams t{};
    t.slots = tl.d_slots; t.wg0 = tl.d_wg0; t.rowp = tl.d_rowp; t.n = tl.n;
    t.rows = stack.wrows; t.rowsh = stack.wrowsh; t.normf = stack.normf; t.auxf = stack.auxf;
    if (tl.outside) { t.orows = tl.outside->wrows; t.orowsh = tl.outside->wrowsh; t.onormf = tl.outside->normf; t.oauxf = tl.outside->auxf; }
    t.nm_max = stack.nm_max; t.dim = stack.dim;
    return t;
}

// ktop 1: the top-1 table forms with an outside operand (fm_collection_wide_match_accepted_each: reverse slots, partial [rows])
template <int KS>
static void wide_filter_table_launch(const WideTableParams& t, int ktop, int grid, hipStream_t stream)
{
    if (ktop == 1)    hipLaunchKernelGGL((wide_filter_table_kernel<KS, 1, true>), dim3(grid), dim3(256), 0, stream, t);
    else if (t.orows) hipLaunchKernelGGL((wide_filter_table_kernel<KS, 2, true>), dim3(grid), dim3(256), 0, stream, t);
    else              hipLaunchKernelGGL((wide_filter_table_kernel<KS, 2, false>), dim3(grid), dim3(256), 0, stream, t);
}

hipError_t launch_wide_filter_table(const Bank& stack, const WideTableLaunch& tl, unsigned cap, uint2* list, float* lscore, unsigned* gbound,
                                    unsigned long long* cnt, int* flag, unsigned long long* partial, hipStream_t stream, int ktop)
{
    WideTableParams t = wide_table_params(stack, tl);
    t.list = list; t.lscore = lscore; t.cap = cap; t.cnt = cnt; t.gbound = gbound; t.partial = partial; t.flag = flag;
    const int ks = (stack.dim + 31) / 32;
    if (ks < 5 || ks > 8 || tl.n < 1 || tl.fwg < 1 || (ktop != 2 && (ktop != 1 || !t.orows))) return hipErrorInvalidValue;
    switch (ks) {
        case 5: wide_filter_table_launch<5>(t, ktop, tl.fwg, stream); break;
        case 6: wide_filter_table_launch<6>(t, ktop, tl.fwg, stream); break;
        case 7: wide_filter_table_launch<7>(t, ktop, tl.fwg, stream); break;
        default: wide_filter_table_launch<8>(t, ktop, tl.fwg, stream); break;
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (ktop == 1)    hipLaunchKernelGGL((wide_rescore_table_kernel<1, true>), dim3(2048), dim3(256), 0, stream, t);
    else if (t.orows) hipLaunchKernelGGL((wide_rescore_table_kernel<2, true>), dim3(2048), dim3(256), 0, stream, t);
    else              hipLaunchKernelGGL((wide_rescore_table_kernel<2, false>), dim3(2048), dim3(256), 0, stream, t);
    return hipGetLastError();
}

hipError_t launch_wide_exact_table(const Bank& stack, const WideTableLaunch& tl, unsigned long long* partial, const int* run_flag,
                                   hipStream_t stream, int ktop)
{
    WideTableParams t = wide_table_params(stack, tl);
    t.partial = partial; t.run_flag = run_flag;
    if (tl.n < 1 || tl.rows < kWTile || (ktop != 2 && (ktop != 1 || !t.orows))) return hipErrorInvalidValue;
    if (ktop == 1)    hipLaunchKernelGGL((wide_exact_table_kernel<1, true>), dim3((unsigned)(tl.rows / kWTile)), dim3(256), 0, stream, t);
    else if (t.orows) hipLaunchKernelGGL((wide_exact_table_kernel<2, true>), dim3((unsigned)(tl.rows / kWTile)), dim3(256), 0, stream, t);
    else              hipLaunchKernelGGL((wide_exact_table_kernel<2, false>), dim3((unsigned)(tl.rows / kWTile)), dim3(256), 0, stream, t);
    return hipGetLastError();
}

}  // namespace fm
