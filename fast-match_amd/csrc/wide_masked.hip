// K14 under a mask -- knnMatch(q, t, k, mask) for wide float banks (FM_BANK_F32W, 129 .. 256 values per row): fm_wide_knn_masked,
// fm_wide_knn_masked_dev.  gfx950 only.
//
// The contract is K13's (masked.hip) with K14's distance (wide_f32.hip): row i's list is fm_knn's list for the wide pair computed
// over the train rows the mask permits for row i only -- dist = sqrtf(s), s = fmaf(v_k, v_k, s), k ascending over the real dim --
// ascending by (float32 bits of the distance, train row), strictly; -1 / +inf where fewer than k rows are permitted; k = 1, 2.
// The mask is K13's fm_mask: bit b of word w of row i = (query row i, train row 64 w + b) is permitted, [nq][n_pad / 64] words
// over the PADDED train rows -- a wide bank's n_pad is pad128(n) like every bank's (bank_create_wide), so fm_mask_create's
// geometry is the bank's -- and the bits of padding rows are 0, always.  Wide banks do not grow by appends: there is no
// Bank::real to AND in.
//
// wide_masked_filter_kernel<KS, KTOP> + wide_rescore_kernel<KTOP> (wide_f32.hip's, through launch_wide_rescore): K14's filter
// (part 3 of wide_f32.hip: two blocks of 16 output rows per wave as the B operand of v_mfma_f32_16x16x32_f16, KS = ceil(dim / 32)
// K steps, the train rows' fp16 plane streamed one 16-row tile ahead) with the mask in front of its tail.
//   The mask read.  Lane (lr = lane & 15, lg = lane >> 4) owns, per block, ONE output row (c0 + 16 b + lr) and the 4 reduced rows
//   16 t + 4 lg + r of tile t.  The 16 rows of a tile are 16 bits of ONE word of that output row's mask row -- word t >> 2, bits
//   16 (t & 3) .. + 15 -- and the lane's four are the nibble at 16 (t & 3) + 4 lg.  An 8-byte word covers four tiles: a lane
//   loads one word per block and FOUR tiles, one word ahead (the next word is in flight while the current four tiles run).
//   A forbidden pair leaves by INDEX -- before best[], before the bound and before wide_push -- which is how the SELF form's
//   diagonal leaves: a forbidden near row that reached the bound would shut the permitted neighbours out.
//   Margin.  The margin derivation in wide_f32.hip then holds unchanged.  Every bound is the KTOP-th best score of permitted rows
//   of that output row.  A row x of the exact top-KTOP over the PERMITTED rows has s_real(x) >= s_real of the KTOP-th best of any
//   KTOP permitted rows, so s_fp16(x) >= B - 2 E >= B - M, and x is permitted, so it reaches the test: it is recorded.  The
//   rescoring's second look compares against gbound, the maximum of such bounds: the same argument.
//   The tile skip.  A wave skips the MFMAs and the tail of a (block, tile) in which none of its 16 x 16 pairs is permitted -- one
//   ballot over the lanes' nibbles, so the branch is uniform over the wave -- and does not fetch the operand tile of a tile in
//   which neither block has a permitted pair (the prefetch of tile t + 1 is issued under the ballot of tile t + 1's nibbles,
//   which the words in registers already hold).  A window or band mask costs the words it reads and little else.
//   Only permitted pairs are ever recorded, so wide_rescore_kernel needs no mask.
// wide_masked_exact_kernel<KTOP>: wide_exact_body's tiling (part 2 of wide_f32.hip: 64 x 64 rows per step, 4 x 4 patch per
// thread) with one mask bit tested per candidate.  A step's 64 reduced rows are ONE mask word per output row; thread (tn, tm)
// loads the words of its 4 output rows and tests bit 4 tm + j.  A workgroup skips a step in which none of its 64 x 64 pairs is
// permitted.  For "f32_filter" 0, small calls, banks the filter cannot take (a value that is not finite, scales more than 2^8
// apart) and as the conditional fallback behind run_flag when the record list overflowed.
// Both write keys (float32 distance bits << 32 | train row, ~0 = none) to partial[(split * nq + q) * KTOP + i], ascending in i:
// K9's key format and layout, so knnk_merge_kernel<K> (knn_k.hip) merges the splits and writes [nq][k].
// The route (wide_masked_device) is wide_route's (api_match.hip): option "f32_filter" 0 / 1 / 2, the 4e6 threshold,
// wide_filter_usable, the list-capacity pre-check, the same carving of ws_partial (partial | records | scores | bounds | count).
#include "ctx_internal.h"
#include "wide_parts.h"

#include <algorithm>

namespace fm {

struct WideMaskedFilterParams {
    WideFilterParams f;
    const unsigned long long* mask;   // [f.ncols][mwords]
    int64_t mwords;                   // = f.ntiles / 4
};

// the lane's four bits of tile t in its output row's word w (the word of the four tiles t & ~3 .. t | 3)
__device__ __forceinline__ unsigned wm_nibble(unsigned long long w, int t, int lg)
{
    return (unsigned)(w >> (16 * (t & 3) + 4 * lg)) & 0xFu;
}

template <int KS, int KTOP>
__global__ __launch_bounds__(256)
void wide_masked_filter_kernel(WideMaskedFilterParams mp)
{
    const WideFilterParams& p = mp.f;
    const int blk = (int)(blockIdx.x / p.nsplit), split = (int)(blockIdx.x % p.nsplit);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lr = lane & 15, lg = lane >> 4;
    const int c0 = blk * kWFCols + wave * 16 * kWFBlocks;

    w_v8h bq[kWFBlocks][KS];
    float marg[kWFBlocks], bnd[kWFBlocks], best[kWFBlocks][KTOP];
    const unsigned long long* mrow[kWFBlocks];                  // the output row's mask words (null: a padding row, nothing permitted)
#pragma unroll
    for (int b = 0; b < kWFBlocks; ++b) {
        const int col = c0 + 16 * b + lr;                       // (< the bank's n_pad: a multiple of 128 = kWFCols)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) bq[b][ks] = *(const w_v8h*)(p.colh + (size_t)col * kWideDim + 32 * ks + 8 * lg);
        marg[b] = wide_margin(p.colnorm[col], p.nscale, p.red_nm_max);
        bnd[b] = -INFINITY;
#pragma unroll
        for (int k = 0; k < KTOP; ++k) best[b][k] = -INFINITY;
        mrow[b] = col < p.ncols ? mp.mask + (size_t)col * mp.mwords : nullptr;
    }

    const int t0 = split * p.tiles_per_split;
    const int t1 = min(t0 + p.tiles_per_split, p.ntiles);
    unsigned lbase = kWNoChunk, lused = 0;
    // mw: the word of tile t's group of four; mwn: the next group's, loaded when mw is taken over (4 (w + 1) < t1 <= ntiles: the
    // word exists, ntiles = 4 mwords)
    unsigned long long mw[kWFBlocks] = {}, mwn[kWFBlocks] = {};
    if (t0 < t1) {
#pragma unroll
        for (int b = 0; b < kWFBlocks; ++b) {
            mw[b] = mrow[b] ? mrow[b][t0 >> 2] : 0ull;
            if (4 * ((t0 >> 2) + 1) < t1) mwn[b] = mrow[b] ? mrow[b][(t0 >> 2) + 1] : 0ull;
        }
    }
    w_v8h an[KS];
    bool pre = false;                                           // (wave uniform) an[] holds the current tile
    for (int t = t0; t < t1; ++t) {
        if ((t & 3) == 0 && t != t0) {
#pragma unroll
            for (int b = 0; b < kWFBlocks; ++b) {
                mw[b] = mwn[b];
                if (4 * ((t >> 2) + 1) < t1) mwn[b] = mrow[b] ? mrow[b][(t >> 2) + 1] : 0ull;
            }
        }
        unsigned nib[kWFBlocks];
        bool any[kWFBlocks];
#pragma unroll
        for (int b = 0; b < kWFBlocks; ++b) {
            nib[b] = wm_nibble(mw[b], t, lg);
            any[b] = __builtin_amdgcn_ballot_w64(nib[b] != 0u) != 0ull;
        }
        const bool run = any[0] || any[1];
        w_v8h a[KS];
        if (run) {
            if (pre) {
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) a[ks] = an[ks];
            } else {                                            // (the split's first tile with a permitted pair)
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) a[ks] = *(const w_v8h*)(p.redh + (size_t)(t * 16 + lr) * kWideDim + 32 * ks + 8 * lg);
            }
        }
        pre = false;
        if (t + 1 < t1) {
            // tile t + 1's nibbles: its word is mw, or mwn where t + 1 starts a group
            unsigned nn = 0;
#pragma unroll
            for (int b = 0; b < kWFBlocks; ++b) nn |= wm_nibble(((t + 1) & 3) == 0 ? mwn[b] : mw[b], t + 1, lg);
            pre = __builtin_amdgcn_ballot_w64(nn != 0u) != 0ull;
            if (pre) {
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) an[ks] = *(const w_v8h*)(p.redh + (size_t)((t + 1) * 16 + lr) * kWideDim + 32 * ks + 8 * lg);
            }
        }
        if (!run) continue;
        const int r0 = t * 16 + 4 * lg;                         // this lane's 4 reduced rows
        const float4 ax4 = *(const float4*)(p.redaux + r0);
        const float ax[4] = {ax4.x, ax4.y, ax4.z, ax4.w};
#pragma unroll
        for (int b = 0; b < kWFBlocks; ++b) {
            if (!any[b]) continue;                              // (wave uniform: the MFMAs run with every lane or not at all)
            w_v4f acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[ks], bq[b][ks], acc, 0, 0, 0);
            const int col = c0 + 16 * b + lr;
            float sc[4];
            bool ok[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                sc[r] = __builtin_fmaf(acc[r], p.cscale, ax[r]);
                // bit clear: forbidden, or a padding row (the mask's bits there are 0; the index test costs nothing and keeps the
                // records inside the banks whatever a mask holds), or no such output row (its word is 0)
                ok[r] = ((nib[b] >> r) & 1u) && r0 + r < p.nred;
                if (ok[r]) {
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
            for (int r = 0; r < 4; ++r) wide_push(ok[r] && sc[r] >= bnd[b] - marg[b], col, r0 + r, sc[r], p, lbase, lused);
        }
    }
    wide_pad_chunk(lbase, lused, p);
    // the bound this wave ended with, for the rescoring's second look at the records
    if (lg == 0) {
#pragma unroll
        for (int b = 0; b < kWFBlocks; ++b)
            if (bnd[b] > -INFINITY) atomicMax(p.gbound + c0 + 16 * b + lr, wide_fbits(bnd[b]));
    }
}

struct WideMaskedExactParams {
    WideExactParams e;                // (ncols_alloc: the rows per split of `partial` = the query bank's real rows)
    const unsigned long long* mask;   // [ncols_alloc][mwords]
    int64_t mwords;                   // = e.nred_pad / 64: one word per step
};

template <int KTOP>
__global__ __launch_bounds__(256)
void wide_masked_exact_kernel(WideMaskedExactParams mp)
{
    __shared__ __attribute__((aligned(16))) float colimg[kWideDim * kWLd];
    __shared__ __attribute__((aligned(16))) float redimg[kWHalf * kWLd];

    const WideExactParams& p = mp.e;
    if (p.run_flag) {
        if (*p.run_flag == 0) return;                 // the filter's result stands
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd((int*)p.run_flag + 2, 1);
    }
    const int chunk = (int)(blockIdx.x / p.nsplit), split = (int)(blockIdx.x % p.nsplit);
    const int tid = threadIdx.x;
    const int tn = tid & 15, tm = tid >> 4;
    const int c0 = chunk * kWTile;

    if (c0 < p.ncols_pad) wide_load_kmajor<64>(p.col_rows, c0, p.ncols_pad, 0, colimg, tid);

    float bd[4][KTOP];
    int   bi[4][KTOP];
    float thr[4];
    const unsigned long long* mrow[4];                // the mask words of this thread's 4 output rows (null: no such query row)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        thr[i] = INFINITY;
#pragma unroll
        for (int k = 0; k < KTOP; ++k) { bd[i][k] = INFINITY; bi[i][k] = -1; }
        const int n = c0 + 4 * tn + i;
        mrow[i] = n < p.ncols_alloc ? mp.mask + (size_t)n * mp.mwords : nullptr;
    }

    const int s0 = split * p.steps_per_split;
    const int s1 = min(s0 + p.steps_per_split, p.nsteps);
    for (int st = s0; st < s1; ++st) {
        // the step's 64 reduced rows are word st of every mask row (st < nsteps = mwords); this thread's candidates: bits 4 tm + j
        unsigned nb[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) nb[i] = mrow[i] ? (unsigned)(mrow[i][st] >> (4 * tm)) & 0xFu : 0u;
        // (uniform over the workgroup: every thread passes the same barriers; the barrier also ends the previous step's reads)
        if (!__syncthreads_or((nb[0] | nb[1] | nb[2] | nb[3]) != 0u)) continue;
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
            if (nb[i] == 0u) continue;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int idx = m0 + j;
                // (NaN fails the compare; +inf passes it and fails d < bd: neither is ever listed)
                if (((nb[i] >> j) & 1u) && idx < p.nred && s[i][j] <= thr[i]) {
                    const float d = sqrtf(s[i][j]);
                    if (d < bd[i][KTOP - 1]) {                // strict: earlier row wins ties
                        if constexpr (KTOP == 2) {
                            if (d < bd[i][0]) { bd[i][1] = bd[i][0]; bi[i][1] = bi[i][0]; bd[i][0] = d; bi[i][0] = idx; }
                            else              { bd[i][1] = d; bi[i][1] = idx; }
                        } else {
                            bd[i][0] = d; bi[i][0] = idx;
                        }
                        const float B = bd[i][KTOP - 1];
                        thr[i] = (B * B) * 1.00000024f;        // d2 > thr  =>  sqrtf(d2) >= B
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
                out[k] = ri[k] >= 0 ? (((unsigned long long)__float_as_uint(rd[k]) << 32) | (unsigned)ri[k]) : ~0ull;
        }
    }
}

template <int KS>
static void wide_masked_filter_launch(const WideMaskedFilterParams& mp, int ktop, int grid, hipStream_t stream)
{
    if (ktop == 1) hipLaunchKernelGGL((wide_masked_filter_kernel<KS, 1>), dim3(grid), dim3(256), 0, stream, mp);
    else           hipLaunchKernelGGL((wide_masked_filter_kernel<KS, 2>), dim3(grid), dim3(256), 0, stream, mp);
}

hipError_t launch_wide_masked_filter(const Bank& q, const Bank& t, int ktop, const WideFilterPlan& plan, const unsigned long long* mask,
                                     int64_t mwords, uint2* list, float* lscore, unsigned* gbound, unsigned long long* cnt, int* flag,
                                     unsigned long long* partial, hipStream_t stream)
{
    const int ks = (q.dim + 31) / 32;
    // (the kernel indexes the mask by tile: its words must cover exactly the train bank's padded rows)
    if ((ktop != 1 && ktop != 2) || ks < 5 || ks > 8 || !mask || mwords * 64 != t.n_pad || plan.ntiles != t.n_pad / 16) return hipErrorInvalidValue;
    WideMaskedFilterParams mp;
    WideFilterParams& p = mp.f;
    p.colh = q.wrowsh; p.colnorm = q.normf; p.ncols = (int)q.n;
    p.redh = t.wrowsh; p.redaux = t.auxf; p.nred = (int)t.n;
    const int dk = t.kscale - q.kscale;
    p.cscale = ldexpf(1.f, dk);
    p.nscale = ldexpf(1.f, 2 * dk);
    p.red_nm_max = t.nm_max;
    p.ntiles = plan.ntiles; p.tiles_per_split = plan.tiles_per_split; p.nsplit = plan.nsplit;
    p.list = list; p.lscore = lscore; p.cap = plan.cap; p.cnt = cnt; p.gbound = gbound;
    mp.mask = mask; mp.mwords = mwords;
    const int grid = plan.nchunks * plan.nsplit;
    switch (ks) {
        case 5: wide_masked_filter_launch<5>(mp, ktop, grid, stream); break;
        case 6: wide_masked_filter_launch<6>(mp, ktop, grid, stream); break;
        case 7: wide_masked_filter_launch<7>(mp, ktop, grid, stream); break;
        default: wide_masked_filter_launch<8>(mp, ktop, grid, stream); break;
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_wide_rescore(q, t, ktop, plan.cap, list, lscore, gbound, cnt, flag, partial, stream);
}

hipError_t launch_wide_masked_exact(const Bank& q, const Bank& t, int ktop, const RowReducePlan& plan, const unsigned long long* mask,
                                    int64_t mwords, unsigned long long* partial, const int* run_flag, hipStream_t stream)
{
    if ((ktop != 1 && ktop != 2) || !mask || mwords * 64 != t.n_pad || q.n <= 0) return hipErrorInvalidValue;
    WideMaskedExactParams mp;
    WideExactParams& p = mp.e;
    p.run_flag = run_flag;
    p.col_rows = q.wrows;
    p.ncols_pad = (int)q.n_pad;
    p.red_rows = t.wrows;
    p.nred = (int)t.n;
    p.nsteps = (int)(t.n_pad / kWTile);
    p.nred_pad = (int)t.n_pad;
    p.nsplit = plan.nsplit;
    p.steps_per_split = plan.stages_per_split;
    p.ncols_alloc = (int)q.n;
    p.kend = (q.dim + 7) & ~7;
    p.partial = partial;
    mp.mask = mask; mp.mwords = mwords;
    const int grid = (int)((q.n + kWTile - 1) / kWTile) * plan.nsplit;
    if (ktop == 1) hipLaunchKernelGGL((wide_masked_exact_kernel<1>), dim3(grid), dim3(256), 0, stream, mp);
    else           hipLaunchKernelGGL((wide_masked_exact_kernel<2>), dim3(grid), dim3(256), 0, stream, mp);
    return hipGetLastError();
}

// ---- host side ----------------------------------------------------------------------------------------------------------
// The masked lists of q over t on the context's stream into d_idx / d_dist [q.n][k] (device memory).  q.n > 0; arguments
// checked by the entry points.  wide_route's rule and workspace layout (api_match.hip), with partial = [nsplit][q.n][k].
static int wide_masked_device(fm_ctx* ctx, const Bank& q, const Bank& t, const fm_mask* m, int k, int32_t* d_idx, float* d_dist)
{
    const int64_t nq = q.n;
    int rc;
    if (t.n == 0) {                        // no train rows: the merge of no lists, -1 / +inf
        if ((rc = ws_ensure(ctx, &ctx->ws_partial, &ctx->ws_partial_bytes, 64)) != FM_OK) return rc;
        HIP_TRY(ctx, launch_knnk_merge((const unsigned long long*)ctx->ws_partial, 0, (int)nq, k, d_idx, d_dist, ctx->stream));
        return FM_OK;
    }
    if (m->words * 64 != t.n_pad) return fail(ctx, FM_EINVAL, "fm_wide_knn_masked: the mask's padded rows are not the train bank's");
    const RowReducePlan pl = plan_rowreduce_f32(q.n_pad, t.n_pad, ctx->tune.nsplit);
    const WideFilterPlan fp = plan_wide_filter(q.n_pad, q.n, t.n_pad, ctx->tune);
    const size_t part = (size_t)pl.nsplit * (size_t)nq * (size_t)k * 8;
    const bool filter = ctx->tune.f32_filter != 0 && ctx->d_counters && wide_filter_usable(q, t) &&
                        (ctx->tune.f32_filter >= 2 || (double)q.n * (double)t.n >= 4.0e6) &&
                        q.n * std::min<int64_t>(16, t.n) <= (int64_t)fp.cap;
    unsigned long long* d_part;
    if (!filter) {
        if ((rc = ws_ensure(ctx, &ctx->ws_partial, &ctx->ws_partial_bytes, part + 64)) != FM_OK) return rc;
        d_part = (unsigned long long*)ctx->ws_partial;
        HIP_TRY(ctx, launch_wide_masked_exact(q, t, k, pl, m->bits, m->words, d_part, nullptr, ctx->stream));
    } else {
        size_t off = 0;
        const size_t o_part = carve(off, part), o_list = carve(off, fp.list_bytes()), o_score = carve(off, fp.list_bytes() / 2),
                     o_bound = carve(off, (size_t)q.n_pad * 4), o_cnt = carve(off, 16);
        if ((rc = ws_ensure(ctx, &ctx->ws_partial, &ctx->ws_partial_bytes, off + 64)) != FM_OK) return rc;
        d_part = (unsigned long long*)((char*)ctx->ws_partial + o_part);
        unsigned long long* d_cnt = (unsigned long long*)((char*)ctx->ws_partial + o_cnt);
        HIP_TRY(ctx, hipMemsetAsync(d_part, 0xff, part, ctx->stream));
        // (the bounds and the count are neighbours: one fill)
        HIP_TRY(ctx, hipMemsetAsync((char*)ctx->ws_partial + o_bound, 0, o_cnt + 16 - o_bound, ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(ctx->d_counters, 0, 8, ctx->stream));
        HIP_TRY(ctx, launch_wide_masked_filter(q, t, k, fp, m->bits, m->words, (uint2*)((char*)ctx->ws_partial + o_list),
                                               (float*)((char*)ctx->ws_partial + o_score), (unsigned*)((char*)ctx->ws_partial + o_bound), d_cnt,
                                               ctx->d_counters, d_part, ctx->stream));
        HIP_TRY(ctx, launch_wide_masked_exact(q, t, k, pl, m->bits, m->words, d_part, ctx->d_counters, ctx->stream));
        ctx->filter_launches += 1;
    }
    HIP_TRY(ctx, launch_knnk_merge(d_part, pl.nsplit, (int)nq, k, d_idx, d_dist, ctx->stream));
    return FM_OK;
}

// Steps 1 .. 4 of the error order (the header): handles, the banks' kind and dims, k, the mask's geometry.
static int wide_masked_check(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, const fm_mask* m, int32_t k, const char* who)
{
    if (!ctx) return fail(nullptr, FM_EINVAL, std::string(who) + ": ctx is NULL");
    if (!q || !t) return fail(ctx, FM_EINVAL, std::string(who) + ": bank is NULL");
    if (!m) return fail(ctx, FM_EINVAL, std::string(who) + ": mask is NULL");
    for (const fm_bank* b : {q, t})
        if (int rc = refuse_bin2(ctx, b, who)) return rc;
    for (const fm_bank* b : {q, t})
        if (b->kind != FM_BANK_F32W)
            return fail(ctx, FM_EINVAL, std::string(who) + ": both banks must be wide float (FM_BANK_F32W: fm_bank_create_f32 with 129 .. 256 "
                                        "values per row); fm_knn_masked is the call that serves the other kinds");
    if (q->dim != t->dim) return fail(ctx, FM_EINVAL, std::string(who) + ": query/train dim mismatch");
    if (k < 1) return fail(ctx, FM_EINVAL, std::string(who) + ": k must be at least 1");
    if (k > 2) return fail(ctx, FM_EUNSUPPORTED, std::string(who) + ": k >= 3 is not built for wide float banks (fm_knn serves them with k <= 2 too)");
    int rc = mask_check(ctx, m, who);
    if (rc != FM_OK) return rc;
    if (m->coll) return fail(ctx, FM_EINVAL, std::string(who) + ": the mask was made for a collection (fm_mask_create_coll); a bank pair takes fm_mask_create's");
    if (m->nq != q->n)
        return fail(ctx, FM_EINVAL, std::string(who) + ": the mask has " + std::to_string(m->nq) + " query rows, the query bank " + std::to_string(q->n));
    if (m->nt != t->n)
        return fail(ctx, FM_EINVAL, std::string(who) + ": the mask has " + std::to_string(m->nt) + " train rows, the train bank " + std::to_string(t->n));
    return FM_OK;
}

}  // namespace fm

using namespace fm;

extern "C" int fm_wide_knn_masked(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, const fm_mask* mask, int32_t k, int32_t* idx, float* dist)
{
    int rc = wide_masked_check(ctx, q, t, mask, k, "fm_wide_knn_masked");
    if (rc != FM_OK) return rc;
    const int64_t nq = q->n;
    if (nq > 0 && (!idx || !dist)) return fail(ctx, FM_EINVAL, "fm_wide_knn_masked: output pointer is NULL");
    if (nq == 0) return FM_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t ob = align256((size_t)nq * (size_t)k * 4);
    if ((rc = ws_ensure(ctx, &ctx->ws_out, &ctx->ws_out_bytes, 2 * ob + 64)) != FM_OK) return rc;
    int32_t* d_idx = (int32_t*)ctx->ws_out;
    float* d_dist = (float*)((char*)ctx->ws_out + ob);
    CallScope cs(ctx);
    HIP_TRY(ctx, hipEventRecord(ctx->ev_k0, ctx->stream));
    if ((rc = wide_masked_device(ctx, *q, *t, mask, k, d_idx, d_dist)) != FM_OK) return rc;
    HIP_TRY(ctx, hipEventRecord(ctx->ev_k1, ctx->stream));
    ctx->kernel_timed = true;
    ctx->pending_pairs += nq * t->n;
    ctx->pending_bytes += bank_bytes(q) + bank_bytes(t);
    HIP_TRY(ctx, d2h(ctx, idx, d_idx, (size_t)nq * k * 4));
    HIP_TRY(ctx, d2h(ctx, dist, d_dist, (size_t)nq * k * 4));
    return cs.finish();
}

extern "C" int fm_wide_knn_masked_dev(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, const fm_mask* mask, int32_t k, int32_t* d_idx,
                                      float* d_dist, void* consumer_stream)
{
    const char* who = "fm_wide_knn_masked_dev";
    int rc = wide_masked_check(ctx, q, t, mask, k, who);
    if (rc != FM_OK) return rc;
    const int64_t nq = q->n;
    if (nq == 0) return FM_OK;
    if (!d_idx || !d_dist) return fail(ctx, FM_EINVAL, "fm_wide_knn_masked_dev: output pointer is NULL");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((rc = check_device_ptr(ctx, d_idx, who, "d_idx")) != FM_OK || (rc = check_device_ptr(ctx, d_dist, who, "d_dist")) != FM_OK) return rc;
    // (the sweep and the merge are launched together: the context's stream waits for the consumer's work in front of both)
    if ((rc = wait_for_stream(ctx, consumer_stream)) != FM_OK) return rc;
    if ((rc = wide_masked_device(ctx, *q, *t, mask, k, d_idx, d_dist)) != FM_OK) return rc;
    return results_written(ctx, consumer_stream);
}
