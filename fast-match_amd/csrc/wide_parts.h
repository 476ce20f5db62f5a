// K14's device-side parts that more than one translation unit compiles: wide_f32.hip (the bank-pair, SELF and table kernels) and
// wide_masked.hip (the masked bank-pair kernels).  Nothing here is a kernel; every piece is documented where wide_f32.hip's
// file comment describes the part it belongs to.
#pragma once
#include "tile_ops.h"

namespace fm {

typedef _Float16 w_v8h __attribute__((ext_vector_type(8)));
typedef float    w_v4f __attribute__((ext_vector_type(4)));

// ---- part 2: the exact all-pairs kernel --------------------------------------------------------------------------------------
constexpr int kWTile = 64;                 // rows per block step, both sides
constexpr int kWLd   = kWTile + 4;         // padded leading dimension (floats) of the k-major images
constexpr int kWHalf = 128;                // k per staged half of the reduced rows

struct WideExactParams {
    const float* col_rows;    // [ncols_pad][256]
    int          ncols_pad;
    const float* red_rows;    // [nred_pad][256]
    int          nred;        // real rows
    int          nsteps;      // ceil(nred_pad / 64)
    int          nred_pad;
    int          nsplit;
    int          steps_per_split;
    int          ncols_alloc;
    int          kend;        // dim rounded up to 8 (129 .. 256: the second half's length is kend - 128)
    unsigned long long* partial;
    const int*   run_flag;    // null, or: skip the whole launch unless *run_flag != 0
};

// NK4 float4 per row from column k0 of 64 rows into the k-major image img[k - k0][row]; rows from row_end on read as zeros
template <int NK4>
__device__ __forceinline__ void wide_load_kmajor(const float* __restrict__ rows, int row0, int row_end, int k0, float* __restrict__ img, int tid)
{
#pragma unroll
    for (int i = 0; i < NK4 / 4; ++i) {
        const int f4 = tid + 256 * i;              // 0 .. 64 * NK4 - 1
        const int r = f4 / NK4, k4 = (f4 % NK4) * 4;
        const float4 v = (row0 + r < row_end) ? *(const float4*)(rows + (size_t)(row0 + r) * kWideDim + k0 + k4) : float4{0.f, 0.f, 0.f, 0.f};
        img[(k4 + 0) * kWLd + r] = v.x;
        img[(k4 + 1) * kWLd + r] = v.y;
        img[(k4 + 2) * kWLd + r] = v.z;
        img[(k4 + 3) * kWLd + r] = v.w;
    }
}

// ---- part 3: fp16 matrix-core filter + exact rescoring -----------------------------------------------------------------------
constexpr int kWFBlocks = 2;                       // blocks of 16 output rows per wave
constexpr int kWFCols   = 4 * 16 * kWFBlocks;      // output rows per workgroup (4 waves)

struct WideFilterParams {
    const uint16_t* colh;  const float* colnorm;  int ncols;     // output rows: fp16 plane, |scaled row|^2, real rows
    const uint16_t* redh;  const float* redaux;   int nred;      // reduced rows: fp16 plane, -|scaled row|^2 / 2, real rows
    float cscale;          // 2^(kred - kcol): a dot product of the two planes in the reduced bank's scale
    float nscale;          // 2^(2 (kred - kcol)): the output rows' norms in the reduced bank's scale
    float red_nm_max;
    int   ntiles, tiles_per_split, nsplit;
    uint2* list; float* lscore; unsigned cap; unsigned long long* cnt;    // records (output row, reduced row), their scores, the count
    unsigned* gbound;      // [ncols_pad] the best bound any wave reached per output row, as ordered bits (wide_fbits)
};

// float -> unsigned whose order is the floats' (atomicMax on it; 0 lies below every float)
__device__ __forceinline__ unsigned wide_fbits(float f)
{
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float wide_bits_f(unsigned k)
{
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
__device__ __forceinline__ float wide_margin(float colnorm, float nscale, float red_nm_max)
{
    return 1.25f * 0.0009765625f * (colnorm * nscale + red_nm_max);
}

// The list is handed out in chunks of 64 slots, one atomic per chunk and wave: an atomic per push on the one counter would
// serialise the whole sweep.  base / used: the wave's current chunk (wave uniform; base kWNoChunk = none yet).  A chunk that
// cannot take a push is padded with empty records (output row kWNoRecord) and a new one reserved; *cnt counts reserved slots,
// every one of which below cap is written.  The overflow is STICKY: *cnt is a 64-bit word (2^58 reservations before it could
// wrap), and a wave whose reservation starts at or beyond cap stops recording for good (base kWFull) -- the call is redone by
// the exact kernel anyway -- so the count only ever says "more than cap" once it has.
constexpr unsigned kWNoChunk = 0xffffffffu, kWFull = 0xfffffffeu, kWNoRecord = 0xffffffffu;

__device__ __forceinline__ void wide_pad_chunk(unsigned base, unsigned used, const WideFilterParams& p)
{
    const unsigned lane = threadIdx.x & 63;
    if (base < kWFull && lane >= used && base + lane < p.cap) p.list[base + lane] = make_uint2(kWNoRecord, 0u);
}

// one record per set lane of `pred`
__device__ __forceinline__ void wide_push(bool pred, int col, int row, float score, const WideFilterParams& p, unsigned& base, unsigned& used)
{
    const unsigned long long m = __builtin_amdgcn_ballot_w64(pred);
    if (m == 0ull || base == kWFull) return;
    const unsigned lane = threadIdx.x & 63;
    const unsigned n = (unsigned)__builtin_popcountll(m);
    if (base == kWNoChunk || used + n > 64u) {
        wide_pad_chunk(base, used, p);
        unsigned nb = 0;
        if (lane == 0) {
            const unsigned long long r = atomicAdd(p.cnt, 64ull);
            nb = r >= p.cap ? kWFull : (unsigned)r;             // (cap is a multiple of 64 and at most 2^28: a slot below it fits 32 bits)
        }
        base = (unsigned)__builtin_amdgcn_readfirstlane((int)nb);
        used = 0;
        if (base == kWFull) return;
    }
    const unsigned at = base + used + (unsigned)__builtin_popcountll(m & ((1ull << lane) - 1ull));
    if (pred && at < p.cap) { p.list[at] = make_uint2((unsigned)col, (unsigned)row); p.lscore[at] = score; }
    used += n;
}

}  // namespace fm
