// K10 -- radiusMatch: cv2.BFMatcher(NORM_L2).radiusMatch(q, t, maxDistance), compactResult = False.  Every train row j
// with dist(i, j) < r_i, per query row i, ordered by (float32 bits of the distance, train index).
//   dist: the bits fm_knn2 returns -- integer route sqrtf((float)d2) of the exact int32 d2, float32 route K5's chain
//   (s = fmaf(v, v, s), k ascending, then sqrtf); r_i = float32(maxDistance) or the caller's per-row radius; r <= 0 or
//   NaN: no entries, r = +inf: every train row.
//
//   radius_limits_kernel  per query row: integer route D_i = the largest d2 with sqrtf((float)d2) < r_i (sqrt_bits is
//                         monotone, so "d2 <= D_i" is the exact test; from 4 197 200 on two d2 share one root, which
//                         the device search over sqrtf itself gets right); float32 route the fp16 filter's threshold
//                         A <= r_i^2 + M (M = K8's margin, filter_f16.hip) in the MFMA's accumulator units.
//   radius_*_kernel<FILL> the distance sweep on the matrix cores -- integer route v_mfma_i32_16x16x64_i8 on the
//                         bank's int8 rows, float32 route v_mfma_f32_16x16x32_f16 on its scaled fp16 rows -- whose
//                         epilogue is the threshold test: FILL = false counts the hits of every query row, FILL = true
//                         (after an exclusive scan of the counts) recomputes the tiles and writes 64-bit keys into the
//                         row's segment (integer route (dist bits << 32) | train row; float32 route (query row << 32) |
//                         train row, a candidate).
//   radius_rescore_kernel float32 route: the exact chain per candidate; a candidate at or beyond r_i becomes ~0.
//   sorting               per segment: <= kRSortThread keys one thread, <= kRSortLds one workgroup (bitonic in LDS),
//                         longer ones rocPRIM's segmented radix sort (off the hot path: r = inf against large banks).
//   radius_compact_kernel sorted keys -> train index / distance at the row's final offset.
//   radius_ham_kernel     Hamming route (fm_hamming_radius_match and kin, binary banks): K11's FP4 operands and K11's loop with
//                         the threshold test on the raw dot product W - 2 h (ham_radius.h); FILL keys are (float bits of h << 32)
//                         | train row, final like the integer route's: everything behind the count sweep is that route's path.
// Query rows go in chunks whose candidates fit in the option "radius_ws_bytes" (24 bytes per candidate; 28 against a collection).
// A train collection (fm_collection_radius_match): the train bank is the collection's stack, which has padding rows behind
//   EVERY image whose size is no multiple of 128.  Their values would pass (norm 2^26 against D = 0x7fffffff at r = +inf; 1e18
//   per float32 dimension is finite, and the `all` path filters nothing), so both sweeps mask them by INDEX: RSweep::st_real,
//   the real rows per 128-row stage, bounds `rowlim` beside the split's end -- one table word per 64-row stage, uniform.
//   No padding row ever becomes a key; radius_compact_kernel<true> turns a key's physical row into (image, row) with
//   coll_tab.h's lookup.  Physical order is logical order, so the keys sort as (distance bits, image, row) unchanged.
// A plain bank that grew by appends has padding rows INSIDE it (Bank::real, fm_internal.h): the integer sweep drops them by
//   the stage's real-row word (RSweep::real), the float32 route in radius_rescore_kernel -- the fp16 sweep is not touched.
// Device forms (fm_radius_match_dev, fm_collection_radius_match_dev): the limits kernel reads the caller's radii in place,
//   the offsets come from a device copy of the scan (integer route) or radius_offsets_kernel (float32 route, per chunk), the
//   compaction writes the caller's arrays at the final offsets for the rows that fit in cap.  The host still reads the
//   counts back (chunk plan, segment sort).
// Under a mask (fm_radius_match_masked, fm_collection_radius_match_masked and their _dev forms; K13's fm_mask): the four
//   sweeps live in radius_sweeps.inc, included once unmasked (radius_*_kernel, the code they always were) and once with
//   MASKED = true (rmask_*_kernel).  A masked sweep ANDs the query row's mask word of the stage into its hit bits in front of
//   the count and of r_emit, and skips the LDS reads and MFMAs of a stage in which its rows permit nothing (r_mask_word below).
//   Everything behind the sweeps -- scan, chunks, rescoring, sort, compaction -- sees permitted candidates only and is unchanged.
// Geometry of the sweeps: a workgroup = 4 waves, a wave = 4 blocks of 16 query rows (the MFMA's N, held in VGPRs for the
// whole sweep), the train rows (M) stream through LDS 64 at a time, rows padded by 16 bytes against bank conflicts.
// grid = (query groups of 256 rows, splits of the train range).
//
// Wide route (fm_wide_radius_match and kin: two FM_BANK_F32W banks, or a wide query bank against a wide collection's stack;
// K14's planes, wide_f32.hip): the float32 route at 129 .. 256 values per row.  dist is K14's chain over the real dim.
//   radius_wide_limits_kernel  the threshold on A, with K14's margin (derivation below).
//   radius_wide_kernel<FILL, KS>  the sweep: v_mfma_f32_16x16x32_f16 on the banks' wrowsh planes (pitch 256 halves, zero padded
//                         beyond dim: a padding product adds nothing), KS = ceil(dim / 32) = 5 .. 8 K steps, the epilogue
//                         radius_f16_kernel's -- A = |q'|^2 cq + |t'|^2 ct - 2 acc, a hit is A <= thr[q] -- and r_emit's keys.
//   radius_wide_rescore_kernel  the exact chain over wrows (pitch 256), to dim rounded up to 4: a padding term is
//                         fmaf(+0, +0, s) = s; keep = d < rr[q].
//   Everything else -- scan, chunks, sort tiers, compaction, the device forms' offsets -- is the float32 route's, unchanged.
// Geometry.  Four blocks of 16 query rows per wave as the B operand would be 4 * KS * 4 = 128 VGPRs at KS = 8, before a single
//   streamed row is held: a wave keeps TWO blocks (K14's choice: 64 VGPRs at 256-D), a workgroup of 4 waves 128 query rows,
//   grid = (query groups of 128 rows, splits of the train range).  The streamed rows come STRAIGHT FROM MEMORY, one 16-row
//   tile ahead in registers (2 * KS * 4 = 64 more VGPRs at KS = 8), as wide_filter_body reads them, and not through LDS:
//   a 64-row stage at a conflict-free pitch of 2 * 256 + 16 bytes is 33 KiB, so a double buffer (66 KiB) does not fit in
//   64 KiB of static LDS, and a single buffer puts two barriers and the whole load latency into every stage.  From memory the
//   four waves of a workgroup read the same tiles (three of four reads hit the cache), a lane's 16-byte pieces are its own MFMA
//   operands (no transpose, no bank conflict to pad against), there is no barrier, and the load of tile t + 1 is in flight
//   under the 2 * KS MFMAs and the epilogue of tile t.  This is the loop K14's filter already runs at these widths.
//   A split is whole 64-row stages (four tiles: r_emit's 16 candidates per lane); rows are read up to the stage's end, which
//   lies inside the bank's padded rows (n_pad is a multiple of 128).  Padding is masked by index exactly as on the float32
//   route: r_real_end / st_real for a collection's stack, row < nt for a bank.  Wide banks do not grow: no gap rows.
// Margin, in the accumulator's (d2) units 2^(kq + kt); q' and t' are the scaled rows.  K14's error terms (wide_f32.hip) are in
//   score units s = q'.t' - |t'|^2 / 2, and d2 = |q'|^2 - 2 s: they double.
//   * fp16 operand rounding: <= 2^-11 (1 + 2^-12)(|q'|^2 + |t'|^2) on the dot product, whatever the number of terms, so
//     <= 2^-10 (1 + 2^-12)(...) on A;
//   * the matrix core's float32 accumulation of n <= 256 exact fp16 products: <= n 2^-24 sum |products| <= 2^-16 |q'||t'| on
//     the dot product, <= 2^-16 (|q'|^2 + |t'|^2) on A;
//   * the norms (float64 sums of the unrounded scaled values, rounded to float32 once), their scaling by exact powers of two and the
//     epilogue's two float32 operations: a few 2^-24 (|q'|^2 + |t'|^2).
//   Together |A - d2_real| <= 2^-10 (1 + 2^-4)(|q'|^2 + max |t'|^2).  The exact chain's d2 is within n 2^-24 d2 <=
//   2^-15 (|q'|^2 + |t'|^2) of the real one (d2 <= 2 (|q'|^2 + |t'|^2)), and sqrtf(d2) < r implies d2 < r^2 (1 + 2^-22).  So a row the
//   exact chain keeps has A <= r^2 (1 + 2^-22) + (1 + 2^-4 + 2^-5) 2^-10 (...) = r^2 (...) + 1.094 * 2^-10 (...), inside
//   T = (r^2 unit + M)(1 + 2^-20), M = 1.25 * 2^-10 (|q'|^2 cq + nm_max ct): K14's constant, not K8's 1.1 -- the accumulation
//   terms grow with the number of products and are twice as large at 256 values.
//   The `all` path (every pair a candidate, the rescoring decides): a value that is not finite on either side, scale exponents
//   more than 8 apart (K14's rule), or a bank whose scale is above 2^72 (largest magnitude below 2^-59: filter_usable's value
//   window -- the exact chain's underflow error is absolute, 256 * 2^-150, and must stay inside the slack of M).
#include "ctx_internal.h"
#include "coll_tab.h"
#include "ham_radius.h"
#include <algorithm>
#include <optional>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_segmented_radix_sort.hpp>

namespace fm {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef _Float16 rv8h __attribute__((ext_vector_type(8)));
typedef float rv4f __attribute__((ext_vector_type(4)));
typedef int rv8i __attribute__((ext_vector_type(8)));

constexpr int kRStage = 64;                // train rows per LDS stage
constexpr int kRNB = 4;                    // blocks of 16 query rows per wave
constexpr int kRWaves = 4;
constexpr int kRQPerWG = 16 * kRNB * kRWaves;
constexpr int kRRowI8 = kDim + 16;         // LDS row pitch (bytes), int8 rows
constexpr int kRRowH = 2 * kDim + 16;      // ... fp16 rows
constexpr int kRSortThread = 16;
constexpr int kRSortLds = 2048;
constexpr float kREps = 1.1f / 1024.0f;    // K8's margin: |A - D| <= eps (|c|^2 + max |m|^2) (filter_f16.hip)
constexpr int kRWNB = 2;                   // wide route: blocks of 16 query rows per wave
constexpr int kRWQPerWG = 16 * kRWNB * kRWaves;
constexpr float kRWEps = 1.25f / 1024.0f;  // wide route: K14's margin (file comment)
constexpr int kRWScaleMax = 72;            // wide route: the largest bank scale the sweep takes (filter_f16.hip: kFScaleMax)

struct RSweep {
    const int8_t* qrows; const int32_t* qnorm;      // integer route (rows of this launch's first query row on)
    const int8_t* trows; const int32_t* tnorm;
    const uint16_t* qrowsh; const float* qnormf;    // float32 route
    const uint16_t* trowsh; const float* tnormf;
    const uint8_t* q4; const uint8_t* t4;           // Hamming route: the banks' FP4 planes (Bank::rows4), 64 ks bytes per row
    int ks, W;                 // Hamming route: MFMA K steps per row (0: another route), bits per row
    int ham2;                  // Hamming route on NORM_HAMMING2 banks (K11b): ks = the tetrahedral image's K steps, 1 .. 6, W = 4 bytes cells
                               // per row; r_sweep hands the launch to hamming2.hip's radius_ham2_kernel
    float cq, ct;              // float32 route: stored |q|^2, |t|^2 -> accumulator units 2^(kq + kt)
    int all;                   // float32 route without filter planes: every pair is a candidate
    int nq, nt, per;           // query rows of the launch, train rows, train rows per split (a multiple of kRStage; Hamming: of 128)
    const int* lim;            // integer route: D_i (-1: none)
    const float* thr;          // float32 route: threshold on A in accumulator units; Hamming route: the least dot product of a hit
    unsigned* cnt;             // FILL = false: hit counts; FILL = true: cursors (zeroed)
    const int64_t* off;        // FILL: segment offsets of the launch's query rows, minus `base`
    int64_t base;
    unsigned long long* keys;
    const int* st_real;        // a train collection's stack: real rows per 128-row stage (padding sits behind EVERY image and is
                               // masked by index, never by value); null: a plain bank, padding only behind row nt
    const unsigned long long* real;   // a plain bank that grew by appends and has padding rows below nt: its real-row bitmap
                                      // (Bank::real, one word per 64-row stage); null: none
    int wks;                   // wide route: MFMA K steps per row, 5 .. 8 (0: another route); the float32 route's fields then
                               // hold the wide planes (wrowsh at pitch kWideDim, normf)
    const unsigned long long* mask;   // the masked calls: fm_mask's words of this launch's first query row on ([nq][mwords], one word
    int64_t mwords;                   // per query row and 64-row stage, padding bits 0); null: none -- the unmasked kernels never read it
};

// Grown train banks: the 16 candidates of a lane in the stage at `base` (tile tt, register r -> bit 4 tt + r, train row
// base + 16 tt + 4 g + r) that are real rows.  One uniform 8-byte load per stage.
__device__ __forceinline__ unsigned r_word_bits(unsigned long long w, int g)
{
    const unsigned long long rw = w >> (4 * g);
    unsigned bits = 0;
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) bits |= ((unsigned)(rw >> (16 * tt)) & 0xFu) << (4 * tt);
    return bits;
}

__device__ __forceinline__ unsigned r_real_bits(const unsigned long long* __restrict__ real, int base, int g)
{
    return r_word_bits(real[base >> 6], g);
}

// The masked sweeps (MASKED, a compile-time parameter of the bodies below: the unmasked kernels hold none of this).  Query row
// q's word of the 64-row stage at `base`: the four lanes g of a row read the same 8 bytes; a lane without a query row reads
// nothing and permits nothing.  The word of stage s + 1 is loaded while stage s is worked on (r_mask_next) and turned into the
// lane's 16 candidate bits (r_word_bits: the layout of the hit mask) at the top of its own stage -- ahead of the stage's LDS
// traffic and MFMAs, and one whole stage ahead of its first use.  The bits are ANDed into the hit mask in front of the count
// and in front of r_emit: the count sweep and the fill sweep read the same words (nothing writes a mask during a call), so
// the fill finds exactly what the count counted.
__device__ __forceinline__ unsigned long long r_mask_word(const RSweep& p, int q, int base)
{
    return q < p.nq ? p.mask[(size_t)q * (size_t)p.mwords + (size_t)(base >> 6)] : 0ull;
}

// Rows of the 64-row stage at `base` that may be reported: up to the split's end t1 and, in a collection's stack, up to the
// real rows of the 128-row stage the 64 rows lie in (one table word per stage; <= base where the stage's half is padding).
__device__ __forceinline__ int r_real_end(const RSweep& p, int base, int t1)
{
    if (!p.st_real) return t1;
    return min(t1, (base & ~127) + p.st_real[base >> 7]);
}

// Hits of one lane for one query block in a stage (mask over 16 candidates: tile tt, register r -> bit 4 tt + r) into the
// row's segment: the four lanes of one query row (j, j + 16, j + 32, j + 48) take one cursor increment together.
__device__ __forceinline__ void r_emit(const RSweep& p, unsigned mask, const unsigned (&hi)[16], int q, bool live, int base, int lane)
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

#define R_SWEEP_MASKED false
#define R_SWEEP_KERNEL(route) radius_##route##_kernel
#include "radius_sweeps.inc"
#undef R_SWEEP_MASKED
#undef R_SWEEP_KERNEL
#define R_SWEEP_MASKED true
#define R_SWEEP_KERNEL(route) rmask_##route##_kernel
#include "radius_sweeps.inc"
#undef R_SWEEP_MASKED
#undef R_SWEEP_KERNEL

// Hamming route: the least dot product of a hit per query row (ham_radius.h).
__global__ void radius_ham_limits_kernel(const float* __restrict__ radius, float radius_all, int nq, int W, float* __restrict__ thr)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nq) return;
    thr[i] = ham_radius_dot_min(ham_radius_limit(radius ? radius[i] : radius_all, W), W);
}

// Per query row: the radius and what the sweep compares against (see the file comment).  `radius` is the staged copy of the
// host form's array or, in the device forms, the caller's own array read in place.
__global__ void radius_limits_kernel(const float* __restrict__ radius, float radius_all, int nq, int f32, int all,
                                     const float* __restrict__ qnormf, float cq, double unit, float nt_max,
                                     int* __restrict__ lim, float* __restrict__ thr, float* __restrict__ rr)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nq) return;
    const float r = radius ? radius[i] : radius_all;
    rr[i] = r;
    if (!f32) {
        int D = -1;
        if (r > 4096.f) D = 0x7fffffff;                  // beyond every d2 of two 128-byte rows (<= 128 * 255^2)
        else if (r > 0.f) {
            unsigned h = (unsigned)((double)r * (double)r) + 8u;
            while (h > 0u && !(sqrtf((float)h) < r)) --h;
            D = (sqrtf((float)h) < r) ? (int)h : -1;
        }
        lim[i] = D;
    } else {
        float T;
        if (!(r > 0.f)) T = -INFINITY;
        else if (all || __builtin_isinf(r)) T = INFINITY;
        else {
            const double r2 = (double)r * (double)r * unit;
            const double M = (double)kREps * ((double)qnormf[i] * cq + nt_max);
            T = (float)((r2 + M) * (1.0 + 1.0 / 1048576.0));    // (+ 2^-20: the roundings of r^2 and of the epilogue's A)
        }
        thr[i] = T;
    }
}

// Float32 route: the exact chain for every candidate key (query row << 32 | train row) of the chunk.  real != null (a
// grown train bank, Bank::real): the fp16 sweep let the bank's gap rows through as candidates like any row below nt -- they
// are dropped here, by index, before they can count.
__global__ __launch_bounds__(256)
void radius_rescore_kernel(unsigned long long* __restrict__ keys, int64_t n, const float* __restrict__ qrowsf,
                           const float* __restrict__ trowsf, const float* __restrict__ rr, unsigned* __restrict__ fcnt,
                           const unsigned long long* __restrict__ real)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned long long k = keys[i];
    const unsigned q = (unsigned)(k >> 32), t = (unsigned)k;
    const float4* a = (const float4*)(qrowsf + (size_t)q * kDim);
    const float4* b = (const float4*)(trowsf + (size_t)t * kDim);
    float s = 0.f;
    for (int k4 = 0; k4 < kDim / 4; ++k4) {
        const float4 x = a[k4], y = b[k4];
        float v;
        v = x.x - y.x; s = __builtin_fmaf(v, v, s);
        v = x.y - y.y; s = __builtin_fmaf(v, v, s);
        v = x.z - y.z; s = __builtin_fmaf(v, v, s);
        v = x.w - y.w; s = __builtin_fmaf(v, v, s);
    }
    const float d = sqrtf(s);
    const bool keep = d < rr[q] && !(real && !real_row(real, (int)t));
    keys[i] = keep ? (((unsigned long long)__float_as_uint(d) << 32) | t) : ~0ull;
    if (keep) atomicAdd(&fcnt[q], 1u);
}

// Wide route: the radius and the sweep's threshold per query row, T = (r^2 unit + M)(1 + 2^-20) with K14's margin
// M = 1.25 * 2^-10 (|q'|^2 cq + nm_max ct) (file comment); `all`, or r = +inf: every pair is a candidate.
__global__ void radius_wide_limits_kernel(const float* __restrict__ radius, float radius_all, int nq, int all,
                                          const float* __restrict__ qnormf, float cq, double unit, float nt_max,
                                          float* __restrict__ thr, float* __restrict__ rr)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nq) return;
    const float r = radius ? radius[i] : radius_all;
    rr[i] = r;
    float T;
    if (!(r > 0.f)) T = -INFINITY;
    else if (all || __builtin_isinf(r)) T = INFINITY;
    else {
        const double r2 = (double)r * (double)r * unit;
        const double M = (double)kRWEps * ((double)qnormf[i] * cq + nt_max);
        T = (float)((r2 + M) * (1.0 + 1.0 / 1048576.0));    // (+ 2^-20: the roundings of r^2 and of the epilogue's A)
    }
    thr[i] = T;
}

// Wide route: the exact chain for every candidate key (query row << 32 | train row) of the chunk over the float32 rows at
// pitch kWideDim, k4n = ceil(dim / 4) float4 steps (zero padding past dim: fmaf(+0, +0, s) = s).  A NaN or +inf distance is
// below no radius.
__global__ __launch_bounds__(256)
void radius_wide_rescore_kernel(unsigned long long* __restrict__ keys, int64_t n, const float* __restrict__ qrows,
                                const float* __restrict__ trows, const float* __restrict__ rr, unsigned* __restrict__ fcnt, int k4n)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned long long k = keys[i];
    const unsigned q = (unsigned)(k >> 32), t = (unsigned)k;
    const float4* a = (const float4*)(qrows + (size_t)q * kWideDim);
    const float4* b = (const float4*)(trows + (size_t)t * kWideDim);
    float s = 0.f;
    for (int k4 = 0; k4 < k4n; ++k4) {
        const float4 x = a[k4], y = b[k4];
        float v;
        v = x.x - y.x; s = __builtin_fmaf(v, v, s);
        v = x.y - y.y; s = __builtin_fmaf(v, v, s);
        v = x.z - y.z; s = __builtin_fmaf(v, v, s);
        v = x.w - y.w; s = __builtin_fmaf(v, v, s);
    }
    const float d = sqrtf(s);
    const bool keep = d < rr[q];
    keys[i] = keep ? (((unsigned long long)__float_as_uint(d) << 32) | t) : ~0ull;
    if (keep) atomicAdd(&fcnt[q], 1u);
}

// Segments of at most kRSortThread keys: one thread each, insertion sort.
__global__ __launch_bounds__(256)
void radius_sort_thread_kernel(unsigned long long* __restrict__ keys, const int64_t* __restrict__ off, int64_t base, int nrows)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nrows) return;
    const int64_t b = off[i] - base, len = off[i + 1] - off[i];
    if (len < 2 || len > kRSortThread) return;
    unsigned long long* s = keys + b;
    for (int64_t x = 1; x < len; ++x) {
        const unsigned long long v = s[x];
        int64_t y = x - 1;
        while (y >= 0 && s[y] > v) { s[y + 1] = s[y]; --y; }
        s[y + 1] = v;
    }
}

// Segments of kRSortThread + 1 .. kRSortLds keys: one workgroup each (rows[] lists them), bitonic sort in LDS.
__global__ __launch_bounds__(256)
void radius_sort_lds_kernel(unsigned long long* __restrict__ keys, const int64_t* __restrict__ off, int64_t base,
                            const int* __restrict__ rows)
{
    __shared__ unsigned long long s[kRSortLds];
    const int i = rows[blockIdx.x], tid = threadIdx.x;
    const int64_t b = off[i] - base;
    const int len = (int)(off[i + 1] - off[i]);
    int n = 2;
    while (n < len) n <<= 1;
    for (int x = tid; x < n; x += 256) s[x] = x < len ? keys[b + x] : ~0ull;
    __syncthreads();
    for (int k = 2; k <= n; k <<= 1)
        for (int m = k >> 1; m > 0; m >>= 1) {
            for (int x = tid; x < n; x += 256) {
                const int y = x ^ m;
                if (y > x) {
                    const unsigned long long u = s[x], v = s[y];
                    if ((u > v) == ((x & k) == 0)) { s[x] = v; s[y] = u; }
                }
            }
            __syncthreads();
        }
    for (int x = tid; x < len; x += 256) keys[b + x] = s[x];
}

// The long segments back from rocPRIM's output buffer.
__global__ __launch_bounds__(256)
void radius_copy_back_kernel(unsigned long long* __restrict__ keys, const unsigned long long* __restrict__ sorted,
                             const int64_t* __restrict__ beg, const int64_t* __restrict__ end)
{
    const int64_t b = beg[blockIdx.x], e = end[blockIdx.x];
    for (int64_t x = b + threadIdx.x; x < e; x += 256) keys[x] = sorted[x];
}

// One wave per row: the first n sorted keys of the row's segment -> train index / distance at its output offset
// dst_off[row] - dst_base, for the rows whose lists end at or before `limit` there (the device forms write the caller's arrays
// at the final offsets and stop at the first row that does not fit in cap; the host forms' staging takes every row).
// COLL: the key's low word is a physical row of the collection's stack, reported as (image, row inside it) -- the sweeps
// let no padding row through, so the lookup always finds one.
template <bool COLL>
__global__ __launch_bounds__(256)
void radius_compact_kernel(const unsigned long long* __restrict__ keys, const int64_t* __restrict__ src_off, int64_t src_base,
                           const int64_t* __restrict__ dst_off, int64_t dst_base, int nrows, int64_t limit, CollTab tab,
                           int32_t* __restrict__ img, int32_t* __restrict__ idx, float* __restrict__ dist)
{
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= nrows) return;
    const unsigned long long* s = keys + (src_off[row] - src_base);
    const int64_t d = dst_off[row] - dst_base, n = dst_off[row + 1] - dst_off[row];
    if (d + n > limit) return;
    for (int64_t x = lane; x < n; x += 64) {
        const unsigned long long k = s[x];
        if constexpr (COLL) {
            int32_t im = -1, lo = -1;
            (void)coll_lookup(tab, (unsigned)k, im, lo);
            img[d + x] = im;
            idx[d + x] = lo;
        } else {
            idx[d + x] = (int32_t)(unsigned)k;
        }
        dist[d + x] = __uint_as_float((unsigned)(k >> 32));
    }
}

// Device forms: out[i] = add + rel[i] (rel null: add) -- a chunk's final offsets into the caller's array.
__global__ void radius_offsets_kernel(const int64_t* __restrict__ rel, int64_t add, int64_t n, int64_t* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = add + (rel ? rel[i] : 0);
}

// ---- host side -------------------------------------------------------------------------------------------------------
static int r_splits(int64_t nq, int64_t nt, int qper = kRQPerWG)
{
    // ~2048 workgroups on the chip, a split of at least 1024 train rows (qper: query rows per workgroup)
    const int64_t qg = (nq + qper - 1) / qper;
    int64_t s = (2048 + qg - 1) / qg;
    if (s > (nt + 1023) / 1024) s = (nt + 1023) / 1024;
    if (s < 1) s = 1;
    if (s > 65535) s = 65535;
    return (int)s;
}

// Hamming route: splits of whole 128-row stages -- ~2048 workgroups on the chip, a split of at least 4 stages (K11's rule,
// plan_hamming); returns the stages per split.  (Restated in tests/hamming_radius_ref.py.)
static int r_ham_stages_per_split(int64_t nq, int64_t nt, int* nsplit)
{
    const int64_t qg = (nq + kRQPerWG - 1) / kRQPerWG, nstages = (nt + kStageRows - 1) / kStageRows;
    int64_t ns = (2048 + qg - 1) / qg;
    if (ns > (nstages + 3) / 4) ns = (nstages + 3) / 4;
    if (ns < 1) ns = 1;
    if (ns > 65535) ns = 65535;
    const int64_t sps = (nstages + ns - 1) / ns;
    *nsplit = (int)((nstages + sps - 1) / sps);
    return (int)sps;
}

static hipError_t r_sweep(const RSweep& base, bool f32, bool fill, int64_t q0, int64_t nq, hipStream_t stream)
{
    RSweep p = base;
    p.nq = (int)nq;
    const bool masked = p.mask != nullptr;
    if (masked) p.mask += q0 * p.mwords;
    if (p.ham2) {
        // K11b: the Hamming route's plan and pointers, the sweep of hamming2.hip (no masks, no collections: refused by the entry points)
        if (masked || p.st_real || p.real) return hipErrorInvalidValue;
        int ns = 1;
        const int per = r_ham_stages_per_split(nq, p.nt, &ns) * kStageRows;
        const Ham2RSweep h{p.q4 + q0 * p.ks * 64, p.t4, p.ks, 3 * p.W, (int)nq, p.nt, per, p.thr + q0, p.cnt + (fill ? 0 : q0),
                           fill ? p.off + q0 : nullptr, p.base, p.keys};
        return launch_hamming2_radius(h, fill, ns, stream);
    }
    if (p.ks) {
        p.q4 += q0 * p.ks * 64; p.thr += q0;
        if (fill) p.off += q0;
        else p.cnt += q0;
        int ns = 1;
        p.per = r_ham_stages_per_split(nq, p.nt, &ns) * kStageRows;
        const dim3 grid((unsigned)((nq + kRQPerWG - 1) / kRQPerWG), (unsigned)ns);
#define FM_RHAM(KS_)                                                                                      \
        if (p.ks == KS_) {                                                                                \
            if (masked && fill) hipLaunchKernelGGL((rmask_ham_kernel<true, KS_>), grid, dim3(256), 0, stream, p);   \
            else if (masked)    hipLaunchKernelGGL((rmask_ham_kernel<false, KS_>), grid, dim3(256), 0, stream, p);  \
            else if (fill) hipLaunchKernelGGL((radius_ham_kernel<true, KS_>), grid, dim3(256), 0, stream, p);  \
            else      hipLaunchKernelGGL((radius_ham_kernel<false, KS_>), grid, dim3(256), 0, stream, p); \
            return hipGetLastError();                                                                     \
        }
        FM_RHAM(1) FM_RHAM(2) FM_RHAM(3) FM_RHAM(4)
#undef FM_RHAM
        return hipErrorInvalidValue;
    }
    if (p.wks) {
        // wide route: 128 query rows per workgroup, splits of whole 64-row stages
        if (!p.all) { p.qrowsh += q0 * kWideDim; p.qnormf += q0; }
        p.thr += q0;
        if (fill) p.off += q0;
        else p.cnt += q0;
        const int ns = r_splits(nq, p.nt, kRWQPerWG);
        const int per = (p.nt + ns - 1) / ns;
        p.per = (per + kRStage - 1) / kRStage * kRStage;
        const dim3 grid((unsigned)((nq + kRWQPerWG - 1) / kRWQPerWG), (unsigned)ns);
#define FM_RWIDE(KS_)                                                                                      \
        if (p.wks == KS_) {                                                                                \
            if (masked && fill) hipLaunchKernelGGL((rmask_wide_kernel<true, KS_>), grid, dim3(256), 0, stream, p);   \
            else if (masked)    hipLaunchKernelGGL((rmask_wide_kernel<false, KS_>), grid, dim3(256), 0, stream, p);  \
            else if (fill) hipLaunchKernelGGL((radius_wide_kernel<true, KS_>), grid, dim3(256), 0, stream, p);  \
            else      hipLaunchKernelGGL((radius_wide_kernel<false, KS_>), grid, dim3(256), 0, stream, p); \
            return hipGetLastError();                                                                      \
        }
        FM_RWIDE(5) FM_RWIDE(6) FM_RWIDE(7) FM_RWIDE(8)
#undef FM_RWIDE
        return hipErrorInvalidValue;
    }
    if (f32) { if (!p.all) { p.qrowsh += q0 * kDim; p.qnormf += q0; } p.thr += q0; }
    else     { p.qrows += q0 * kDim; p.qnorm += q0; p.lim += q0; }
    if (fill) p.off += q0;
    else p.cnt += q0;
    const int ns = r_splits(nq, p.nt);
    int per = (p.nt + ns - 1) / ns;
    p.per = (per + kRStage - 1) / kRStage * kRStage;
    const dim3 grid((unsigned)((nq + kRQPerWG - 1) / kRQPerWG), (unsigned)ns);
    if (f32) {
        if (masked && fill) hipLaunchKernelGGL(rmask_f16_kernel<true>, grid, dim3(256), 0, stream, p);
        else if (masked)    hipLaunchKernelGGL(rmask_f16_kernel<false>, grid, dim3(256), 0, stream, p);
        else if (fill) hipLaunchKernelGGL(radius_f16_kernel<true>, grid, dim3(256), 0, stream, p);
        else      hipLaunchKernelGGL(radius_f16_kernel<false>, grid, dim3(256), 0, stream, p);
    } else {
        if (masked && fill) hipLaunchKernelGGL(rmask_i8_kernel<true>, grid, dim3(256), 0, stream, p);
        else if (masked)    hipLaunchKernelGGL(rmask_i8_kernel<false>, grid, dim3(256), 0, stream, p);
        else if (fill) hipLaunchKernelGGL(radius_i8_kernel<true>, grid, dim3(256), 0, stream, p);
        else      hipLaunchKernelGGL(radius_i8_kernel<false>, grid, dim3(256), 0, stream, p);
    }
    return hipGetLastError();
}

static int r_tmp(fm_ctx* ctx, size_t need) { return ws_ensure(ctx, &ctx->ws_rtmp, &ctx->ws_rtmp_bytes, need + 256); }

// offsets[0 .. n] = exclusive scan of counts[0 .. n] (counts[n] = 0) on the device
static int r_scan(fm_ctx* ctx, const unsigned* counts, int64_t* offsets, int64_t n)
{
    size_t bytes = 0;
    HIP_TRY(ctx, rocprim::exclusive_scan(nullptr, bytes, counts, offsets, (int64_t)0, (size_t)(n + 1), rocprim::plus<int64_t>(), ctx->stream));
    int rc = r_tmp(ctx, bytes);
    if (rc != FM_OK) return rc;
    HIP_TRY(ctx, rocprim::exclusive_scan(ctx->ws_rtmp, bytes, counts, offsets, (int64_t)0, (size_t)(n + 1), rocprim::plus<int64_t>(), ctx->stream));
    return FM_OK;
}

static inline size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }

// Sorts the segments [h_off[r] - c0, h_off[r + 1] - c0) of rows r0 .. r1 of the chunk's keys (d_off: the same offsets on the
// device, from row r0 on).
static int r_sort(fm_ctx* ctx, unsigned long long* keys, unsigned long long* alt, int64_t nkeys, const int64_t* h_off,
                  const int64_t* d_off, int64_t r0, int64_t r1, int* d_rows, int64_t* d_beg, int64_t* d_end)
{
    const int64_t c0 = h_off[r0], nr = r1 - r0;
    hipLaunchKernelGGL(radius_sort_thread_kernel, dim3((unsigned)((nr + 255) / 256)), dim3(256), 0, ctx->stream, keys, d_off, c0, (int)nr);
    HIP_TRY(ctx, hipGetLastError());
    std::vector<int> mid;
    std::vector<int64_t> beg, end;
    for (int64_t r = r0; r < r1; ++r) {
        const int64_t len = h_off[r + 1] - h_off[r];
        if (len > kRSortLds) { beg.push_back(h_off[r] - c0); end.push_back(h_off[r + 1] - c0); }
        else if (len > kRSortThread) mid.push_back((int)(r - r0));
    }
    if (!mid.empty()) {
        HIP_TRY(ctx, hipMemcpyAsync(d_rows, mid.data(), mid.size() * 4, hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(radius_sort_lds_kernel, dim3((unsigned)mid.size()), dim3(256), 0, ctx->stream, keys, d_off, c0, (const int*)d_rows);
        HIP_TRY(ctx, hipGetLastError());
    }
    if (!beg.empty()) {
        const size_t nb = beg.size();
        HIP_TRY(ctx, hipMemcpyAsync(d_beg, beg.data(), nb * 8, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(d_end, end.data(), nb * 8, hipMemcpyHostToDevice, ctx->stream));
        size_t bytes = 0;
        HIP_TRY(ctx, rocprim::segmented_radix_sort_keys(nullptr, bytes, keys, alt, (unsigned)nkeys, (unsigned)nb, d_beg, d_end,
                                                         0, 64, ctx->stream));
        int rc = r_tmp(ctx, bytes);
        if (rc != FM_OK) return rc;
        HIP_TRY(ctx, rocprim::segmented_radix_sort_keys(ctx->ws_rtmp, bytes, keys, alt, (unsigned)nkeys, (unsigned)nb, d_beg, d_end,
                                                         0, 64, ctx->stream));
        hipLaunchKernelGGL(radius_copy_back_kernel, dim3((unsigned)nb), dim3(256), 0, ctx->stream, keys, (const unsigned long long*)alt,
                           (const int64_t*)d_beg, (const int64_t*)d_end);
        HIP_TRY(ctx, hipGetLastError());
    }
    // (the host vectors above were handed to hipMemcpyAsync from pageable memory: staged before the call returns)
    return FM_OK;
}

static hipError_t r_compact(fm_ctx* ctx, const RadiusArgs& a, const unsigned long long* keys, const int64_t* src_off, int64_t src_base,
                            const int64_t* dst_off, int64_t dst_base, int64_t nr, int64_t limit, int32_t* img, int32_t* idx, float* dist)
{
    const dim3 grid((unsigned)((nr + 3) / 4));
    if (a.tab)
        hipLaunchKernelGGL(radius_compact_kernel<true>, grid, dim3(256), 0, ctx->stream, keys, src_off, src_base, dst_off, dst_base, (int)nr,
                           limit, *a.tab, img, idx, dist);
    else
        hipLaunchKernelGGL(radius_compact_kernel<false>, grid, dim3(256), 0, ctx->stream, keys, src_off, src_base, dst_off, dst_base, (int)nr,
                           limit, CollTab{nullptr, nullptr, nullptr}, img, idx, dist);
    return hipGetLastError();
}

static hipError_t r_offsets(fm_ctx* ctx, const int64_t* rel, int64_t add, int64_t n, int64_t* out)
{
    hipLaunchKernelGGL(radius_offsets_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, rel, add, n, out);
    return hipGetLastError();
}

// The entry points' one driver (RadiusArgs, ctx_internal.h), by the kind of q: the integer, float32, Hamming or wide route.  t: a plain bank, or (a.tab set) a collection's stack, whose n counts
// the padding rows behind every image: the sweeps mask them by index, a.real_rows is what the call is accounted with.
// a.dev: radius / offsets / img / idx / dist are the caller's DEVICE arrays -- the limits kernel reads the radii in place, the
// offsets are written by a device copy (integer route: the scan) or kernel (float32 route: per chunk), the compaction writes
// the lists at their final offsets; the host still reads the counts back to plan the chunks and the segment sort.
int radius_match(fm_ctx* ctx, const Bank& q, const Bank& t, const RadiusArgs& a)
{
    const int64_t nq = q.n, nt = t.n, cap = a.cap;
    const int64_t real = a.tab ? a.real_rows : nt;
    const bool dev = a.dev;
    const float* radius = a.radius;
    int64_t* offsets = a.offsets;
    int rc;
    // device forms: the context's stream waits for the consumer's work in front of the first kernel that touches a caller array
    bool waited = false;
    auto caller_arrays = [&]() -> int {
        if (!dev || waited) return FM_OK;
        waited = true;
        return wait_for_stream(ctx, a.consumer);
    };
    if (nq == 0 || real == 0 || (!radius && !(a.radius_all > 0.f))) {       // (NaN and r <= 0 included: no entries)
        if (dev) {
            HIP_TRY(ctx, hipSetDevice(ctx->device));
            if ((rc = caller_arrays()) != FM_OK) return rc;
            HIP_TRY(ctx, hipMemsetAsync(offsets, 0, (size_t)(nq + 1) * 8, ctx->stream));
            if (a.n_total) *a.n_total = 0;
            return results_written(ctx, a.consumer);
        }
        for (int64_t i = 0; i <= nq; ++i) offsets[i] = 0;
        if (a.n_total) *a.n_total = 0;
        return FM_OK;
    }
    if (nt > 0x7fffffff || nq > 0x7fffffff) return fail(ctx, FM_EUNSUPPORTED, std::string(a.who) + ": more than 2^31 - 1 rows in a bank");
    // (a mask spans the padded train rows, in whole 128-row stages: every word a sweep reads lies inside it)
    if (a.mask && a.mwords * 64 < ((nt + 127) & ~(int64_t)127)) return fail(ctx, FM_EINVAL, std::string(a.who) + ": the mask does not span the train rows");
    const bool wide = q.kind == FM_BANK_F32W;     // (the wide entry points: both operands wide, of one dim; the float32 route's
                                                  // path with the wide sweep, limits and rescoring kernels)
    const bool f32 = q.kind == FM_BANK_F32 || wide;
    const bool ham2 = q.kind == FM_BANK_BIN2;     // (fm_hamming_radius_match(_dev) on a NORM_HAMMING2 pair: the Hamming route with h2 for h)
    if (ham2 && (t.kind != FM_BANK_BIN2 || a.tab || a.mask || fp4_steps(q) != fp4_steps(t)))
        return fail(ctx, FM_EUNSUPPORTED, std::string(a.who) + ": NORM_HAMMING2 banks are served as plain, unmasked bank pairs only");
    const bool ham = q.kind == FM_BANK_BIN || ham2;       // (the Hamming entry points: both banks binary, of one width; counts are final,
                                                  // so everything behind the count sweep is the integer route's path)
    const bool all = wide ? !(wide_filter_usable(q, t) && q.kscale <= kRWScaleMax && t.kscale <= kRWScaleMax)
                          : f32 && !filter_usable(q, t);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::optional<CallScope> cs;          // (the device forms are not accounted in fm_stats)
    if (!dev) cs.emplace(ctx);
    auto done = [&]() -> int { return dev ? results_written(ctx, a.consumer) : cs->finish(); };
    // per-row arrays: radius | limit | threshold | exact radius | counts [nq+1] | offsets [nq+1] | cursors [nq+1] |
    // final counts [nq+1] | final offsets [nq+1] | sort row list | long-segment begins | ends
    const size_t b4 = al256((size_t)(nq + 1) * 4), b8 = al256((size_t)(nq + 1) * 8);
    rc = ws_ensure(ctx, &ctx->ws_rrows, &ctx->ws_rrows_bytes, 9 * b4 + 4 * b8);
    if (rc != FM_OK) return rc;
    char* w = (char*)ctx->ws_rrows;
    float* d_rad = (float*)w;            w += b4;
    int* d_lim = (int*)w;                w += b4;
    float* d_thr = (float*)w;            w += b4;
    float* d_rr = (float*)w;             w += b4;
    unsigned* d_cnt = (unsigned*)w;      w += b4;
    unsigned* d_cur = (unsigned*)w;      w += b4;
    unsigned* d_fcnt = (unsigned*)w;     w += b4;
    int* d_rows = (int*)w;               w += b4;
    w += b4;
    int64_t* d_off = (int64_t*)w;        w += b8;
    int64_t* d_foff = (int64_t*)w;       w += b8;
    int64_t* d_beg = (int64_t*)w;        w += b8;
    int64_t* d_end = (int64_t*)w;
    const float* k_rad = nullptr;         // what the limits kernel reads
    if (radius && dev) {
        if ((rc = caller_arrays()) != FM_OK) return rc;
        k_rad = radius;                   // (in place: no staging copy)
    } else if (radius) {
        HIP_TRY(ctx, hipMemcpyAsync(d_rad, radius, (size_t)nq * 4, hipMemcpyHostToDevice, ctx->stream));
        k_rad = d_rad;
    }
    const int dk = q.kscale - t.kscale;
    const float cq = f32 && !all ? ldexpf(1.f, -dk) : 1.f, ct = f32 && !all ? ldexpf(1.f, dk) : 1.f;
    const double unit = f32 && !all ? ldexp(1.0, q.kscale + t.kscale) : 1.0;
    // (a collection's nm_max is the real rows': the planes of an image are made while its padding rows still hold 0, the
    // far value goes in afterwards -- coll_f32_finish)
    if (ham2)
        HIP_TRY(ctx, launch_hamming2_radius_limits(k_rad, a.radius_all, (int)nq, 4 * q.dim, d_thr, ctx->stream));
    else if (ham)
        hipLaunchKernelGGL(radius_ham_limits_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, ctx->stream,
                           k_rad, a.radius_all, (int)nq, 8 * q.dim, d_thr);
    else if (wide)
        // (a collection: the stack's scale and largest scaled squared norm as they are NOW -- a later add may rewrite them)
        hipLaunchKernelGGL(radius_wide_limits_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, ctx->stream,
                           k_rad, a.radius_all, (int)nq, all ? 1 : 0, (const float*)(all ? nullptr : q.normf), cq, unit,
                           all ? 0.f : t.nm_max * ct, d_thr, d_rr);
    else
        hipLaunchKernelGGL(radius_limits_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, ctx->stream,
                           k_rad, a.radius_all, (int)nq, f32 ? 1 : 0, all ? 1 : 0,
                           (const float*)(f32 && !all ? q.normf : nullptr), cq, unit, f32 && !all ? t.nm_max * ct : 0.f, d_lim, d_thr, d_rr);
    HIP_TRY(ctx, hipGetLastError());

    RSweep sw{};
    sw.qrows = q.rows8; sw.qnorm = q.norm; sw.trows = t.rows8; sw.tnorm = t.norm;
    sw.qrowsh = wide ? q.wrowsh : q.rowsh; sw.qnormf = q.normf; sw.trowsh = wide ? t.wrowsh : t.rowsh; sw.tnormf = t.normf;
    sw.wks = wide ? (q.dim + 31) / 32 : 0;
    if (wide && !all) ctx->filter_launches += 1;      // (fm_f32_filter_stats: a call that ran the fp16 sweep; `all` runs none)
    sw.q4 = q.rows4; sw.t4 = t.rows4; sw.ks = ham ? fp4_steps(q) : 0; sw.W = ham2 ? 4 * q.dim : 8 * q.dim; sw.ham2 = ham2 ? 1 : 0;
    sw.cq = cq; sw.ct = ct; sw.all = all ? 1 : 0;
    sw.nt = (int)nt; sw.lim = d_lim; sw.thr = d_thr;
    sw.st_real = a.tab ? (const int*)a.tab->st_real : nullptr;
    sw.real = a.tab ? nullptr : t.real;
    sw.mask = a.mask; sw.mwords = a.mwords;      // (the masked entry points; r_sweep moves the pointer to a chunk's first row)
    // 1. counts (candidates on the float32 route), 2. their exclusive scan
    HIP_TRY(ctx, hipMemsetAsync(d_cnt, 0, (size_t)(nq + 1) * 4, ctx->stream));
    HIP_TRY(ctx, hipEventRecord(ctx->ev_k0, ctx->stream));
    sw.cnt = d_cnt;
    HIP_TRY(ctx, r_sweep(sw, f32, false, 0, nq, ctx->stream));
    HIP_TRY(ctx, hipEventRecord(ctx->ev_k1, ctx->stream));
    if (!dev) {
        ctx->kernel_timed = true;
        ctx->pending_pairs += nq * real;
        ctx->pending_bytes += bank_bytes(&q) + bank_bytes(&t);
    }
    if ((rc = r_scan(ctx, d_cnt, d_off, nq)) != FM_OK) return rc;
    std::vector<int64_t> h_off((size_t)nq + 1);
    HIP_TRY(ctx, hipMemcpyAsync(h_off.data(), d_off, (size_t)(nq + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));

    // rows whose candidates are processed: the integer route's counts are final, so only the rows that fit in cap
    int64_t rows_done = nq;
    if (!f32) {
        if (dev) {
            if ((rc = caller_arrays()) != FM_OK) return rc;
            HIP_TRY(ctx, hipMemcpyAsync(offsets, d_off, (size_t)(nq + 1) * 8, hipMemcpyDeviceToDevice, ctx->stream));
        } else {
            for (int64_t i = 0; i <= nq; ++i) offsets[i] = h_off[i];
        }
        if (a.n_total) *a.n_total = h_off[nq];
        rows_done = (int64_t)(std::upper_bound(h_off.begin(), h_off.end(), cap) - h_off.begin()) - 1;
        if (rows_done <= 0) return done();
    }
    if ((rc = caller_arrays()) != FM_OK) return rc;
    // 3. chunks of query rows whose candidates fit the budget: 24 B each (keys, rocPRIM's output, idx + dist), 28 B against a
    // collection (+ img).  The device forms keep the same chunks although they stage no lists.
    int64_t cmax = (int64_t)ctx->tune.radius_ws_bytes / (a.tab ? 28 : 24);
    for (int64_t i = 0; i < rows_done; ++i) cmax = std::max(cmax, h_off[i + 1] - h_off[i]);
    int64_t final_total = 0;      // float32 route: entries of the rows before the chunk
    bool open = true;             // ... every row so far fitted in cap
    std::vector<int64_t> h_foff;
    for (int64_t r0 = 0; r0 < rows_done;) {
        int64_t r1 = r0 + 1;
        while (r1 < rows_done && h_off[r1 + 1] - h_off[r0] <= cmax) ++r1;
        const int64_t c0 = h_off[r0], nc = h_off[r1] - c0, nr = r1 - r0;
        if (nc == 0) {
            if (f32 && dev) HIP_TRY(ctx, r_offsets(ctx, nullptr, final_total, nr, offsets + r0));
            else if (f32) for (int64_t r = r0; r < r1; ++r) offsets[r] = final_total;
            r0 = r1;
            continue;
        }
        const size_t kb = al256((size_t)nc * 8), ob = al256((size_t)nc * 4);
        if ((rc = ws_ensure(ctx, &ctx->ws_rkeys, &ctx->ws_rkeys_bytes, 2 * kb + (dev ? 0 : 3 * ob))) != FM_OK) return rc;
        unsigned long long* keys = (unsigned long long*)ctx->ws_rkeys;
        unsigned long long* alt = (unsigned long long*)((char*)ctx->ws_rkeys + kb);
        // host forms: the chunk's lists are staged behind the keys and copied out
        int32_t* s_idx = (int32_t*)((char*)ctx->ws_rkeys + 2 * kb);
        float* s_dist = (float*)((char*)s_idx + ob);
        int32_t* s_img = (int32_t*)((char*)s_idx + 2 * ob);
        HIP_TRY(ctx, hipMemsetAsync(d_cur, 0, (size_t)nr * 4, ctx->stream));
        sw.cnt = d_cur; sw.off = d_off; sw.base = c0; sw.keys = keys;
        HIP_TRY(ctx, r_sweep(sw, f32, true, r0, nr, ctx->stream));
        if (wide) {
            HIP_TRY(ctx, hipMemsetAsync(d_fcnt, 0, (size_t)(nr + 1) * 4, ctx->stream));
            hipLaunchKernelGGL(radius_wide_rescore_kernel, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, ctx->stream, keys, nc,
                               (const float*)(q.wrows + (size_t)r0 * kWideDim), (const float*)t.wrows, (const float*)(d_rr + r0), d_fcnt,
                               (q.dim + 3) >> 2);
            HIP_TRY(ctx, hipGetLastError());
        } else if (f32) {
            HIP_TRY(ctx, hipMemsetAsync(d_fcnt, 0, (size_t)(nr + 1) * 4, ctx->stream));
            hipLaunchKernelGGL(radius_rescore_kernel, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, ctx->stream, keys, nc,
                               (const float*)(q.rowsf + (size_t)r0 * kDim), (const float*)t.rowsf, (const float*)(d_rr + r0), d_fcnt,
                               (const unsigned long long*)sw.real);
            HIP_TRY(ctx, hipGetLastError());
        }
        if ((rc = r_sort(ctx, keys, alt, nc, h_off.data(), d_off + r0, r0, r1, d_rows, d_beg, d_end)) != FM_OK) return rc;
        if (!f32 && dev) {
            // (rows_done: every row of the chunk fits in cap; no synchronisation -- the next chunk follows on the stream)
            HIP_TRY(ctx, r_compact(ctx, a, keys, d_off + r0, c0, d_off + r0, 0, nr, cap, a.img, a.idx, a.dist));
        } else if (!f32) {
            HIP_TRY(ctx, r_compact(ctx, a, keys, d_off + r0, c0, d_off + r0, c0, nr, INT64_MAX, s_img, s_idx, s_dist));
            HIP_TRY(ctx, hipMemcpyAsync(a.idx + c0, s_idx, (size_t)nc * 4, hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(ctx, hipMemcpyAsync(a.dist + c0, s_dist, (size_t)nc * 4, hipMemcpyDeviceToHost, ctx->stream));
            if (a.tab) HIP_TRY(ctx, hipMemcpyAsync(a.img + c0, s_img, (size_t)nc * 4, hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        } else {
            if ((rc = r_scan(ctx, d_fcnt, d_foff, nr)) != FM_OK) return rc;
            if (dev) {
                // the chunk's final offsets and lists from the device side: the entries before the chunk are known (every chunk
                // ends in the read-back below), and a row is written only while its list ends within cap -- the final
                // offsets ascend, so the first row that does not fit closes the prefix for this chunk and, through `open`,
                // for every later one
                HIP_TRY(ctx, r_offsets(ctx, d_foff, final_total, nr, offsets + r0));
                HIP_TRY(ctx, r_compact(ctx, a, keys, d_off + r0, c0, d_foff, -final_total, nr, open ? cap : (int64_t)-1, a.img, a.idx, a.dist));
            } else {
                HIP_TRY(ctx, r_compact(ctx, a, keys, d_off + r0, c0, d_foff, (int64_t)0, nr, INT64_MAX, s_img, s_idx, s_dist));
            }
            h_foff.resize((size_t)nr + 1);
            HIP_TRY(ctx, hipMemcpyAsync(h_foff.data(), d_foff, (size_t)(nr + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            int64_t fit = 0;             // rows of the chunk whose whole lists fit in cap
            for (int64_t r = 0; r < nr; ++r) {
                if (!dev) offsets[r0 + r] = final_total + h_foff[r];
                if (open && final_total + h_foff[r + 1] <= cap) fit = r + 1;
            }
            if (!dev && open && fit > 0 && h_foff[fit] > 0) {
                const size_t nb = (size_t)h_foff[fit] * 4;
                HIP_TRY(ctx, hipMemcpyAsync(a.idx + final_total, s_idx, nb, hipMemcpyDeviceToHost, ctx->stream));
                HIP_TRY(ctx, hipMemcpyAsync(a.dist + final_total, s_dist, nb, hipMemcpyDeviceToHost, ctx->stream));
                if (a.tab) HIP_TRY(ctx, hipMemcpyAsync(a.img + final_total, s_img, nb, hipMemcpyDeviceToHost, ctx->stream));
                HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            }
            if (fit < nr) open = false;
            final_total += h_foff[nr];
        }
        r0 = r1;
    }
    if (f32) {
        if (dev) HIP_TRY(ctx, r_offsets(ctx, nullptr, final_total, 1, offsets + nq));
        else offsets[nq] = final_total;
        if (a.n_total) *a.n_total = final_total;
    }
    return done();
}

}  // namespace fm
