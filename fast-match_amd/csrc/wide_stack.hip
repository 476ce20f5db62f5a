// K14 over a wide collection's stack -- cv2.BFMatcher.add(images) + knnMatch(query, k) against ALL added images at once for wide
// float descriptors (FM_BANK_F32W, 129 .. 256 values per row): the sweeps behind fm_collection_wide_knn(_dev),
// fm_collection_wide_knn2_ratio(_dev) and fm_collection_wide_votes (api_collection.hip).  gfx950 only.
//
// The contract is K14's (wide_f32.hip): dist = sqrtf(s), s = fmaf(v_k, v_k, s), k ascending over the real dim; keys (float32
// distance bits << 32 | PHYSICAL row of the stack, ~0 = none) to partial[(split * ncols_alloc + q) * KTOP + i], ascending in i,
// so coll_merge2_kernel with the collection's CollTab merges the splits and writes (image, row inside the image, distance).
//
// Why the bank-pair kernels cannot take the stack.  A wide collection's stack is a bank with n = n_pad = used (coll_add_wide),
// and every image starts on a 128-row stage: zero-filled padding rows lie behind every image, INSIDE the bank.  K14 excludes
// padding by index at the END of a bank only (idx < nred).  A zero row lies at |q| from query row q -- 1.0 for unit-norm
// descriptors, whose unrelated rows lie at about 1.41 -- so it would enter the top-2, and it would enter the filter's running
// bound and shut the real neighbours out; dropping it at the merge (coll_real) comes too late.  These kernels read the
// collection's stage table instead: reduced row r is real iff (r & 127) < st_real[r >> 7] (coll_tab.h).
//
// wide_stack_filter_kernel<KS, KTOP> + wide_rescore_kernel<KTOP> (wide_f32.hip's, through launch_wide_rescore): K14's filter
// (part 3 of wide_f32.hip: two blocks of 16 output rows per wave as the B operand of v_mfma_f32_16x16x32_f16, KS = ceil(dim / 32)
// K steps, the stack's fp16 plane streamed one 16-row tile ahead, a running bound per row, one record list per call) with the
// stage table in front of its tail.
//   The table read.  A 16-row tile lies inside one stage (128 = 8 tiles) and the tile index is uniform over the wave, so the
//   table word is ONE uniform read per tile: nr = st_real[t >> 3] - 16 (t & 7) is the number of real rows of tile t (<= 0: none),
//   and lane (lr, lg)'s row 4 lg + r of the tile is real iff 4 lg + r < nr.  The word of tile t + 1 is read a tile ahead, with
//   the operand prefetch it decides.
//   A padding row leaves by INDEX -- before best[], before the bound and before wide_push -- as the masked unit's forbidden
//   pairs and the SELF form's diagonal do.
//   The tile skip.  A tile with nr <= 0 runs no matrix instruction and no tail, and the prefetch does not fetch its operand
//   tile: an image of 1 row is followed by 7 such tiles.  A split whose tiles are all padding makes no record and posts no
//   bound (its bound stays -inf).
//   Margin.  Unchanged: M = 1.25 * 2^-10 (|q'|^2 + max |t'|^2) with the STACK's nm_max, an upper bound of every real row's
//   scaled squared norm, and the stack's one scale -- part 4's argument for a view of the stack, taken for all its images at
//   once.  Every bound is the KTOP-th best score of real rows; a row x of the exact top-KTOP over the real rows has s_real(x) >=
//   s_real of the KTOP-th best of any KTOP real rows, so s_fp16(x) >= B - 2 E >= B - M, and x is real, so it reaches the test.
//   Padding enters none of it: it leaves by index.
//   Only real rows are ever recorded (as physical rows), so wide_rescore_kernel serves unchanged with the stack as its
//   reduced bank.
// wide_stack_exact_kernel<KTOP>: wide_exact_body's tiling (part 2 of wide_f32.hip: 64 x 64 rows per step, 4 x 4 patch per
// thread, the query image whole in LDS, the reduced rows in two halves of 128 k) with the same table test in place of
// idx < nred.  A 64-row step lies inside one stage: one table read per step, nr = st_real[st >> 1] - 64 (st & 1); a step with
// nr <= 0 is skipped by the whole workgroup.  For "f32_filter" 0, small calls, a stack or a query with a value that is not
// finite, scales more than 2^8 apart, and as the conditional fallback behind run_flag when the record list overflowed.
#include "ctx_internal.h"
#include "wide_parts.h"

namespace fm {

struct WideStackFilterParams {
    WideFilterParams f;               // (nred is not read: the table says which reduced rows are real)
    const int32_t* st_real;           // [f.ntiles / 8] real rows per 128-row stage
};

template <int KS, int KTOP>
__global__ __launch_bounds__(256)
void wide_stack_filter_kernel(WideStackFilterParams sp)
{
    const WideFilterParams& p = sp.f;
    const int blk = (int)(blockIdx.x / p.nsplit), split = (int)(blockIdx.x % p.nsplit);
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
    // nrn: the real rows of the NEXT tile to run (t0 first), read one tile ahead (t < ntiles = 8 stages' worth: the word exists)
    int nrn = t0 < t1 ? sp.st_real[t0 >> 3] - 16 * (t0 & 7) : 0;
    w_v8h an[KS];
    bool pre = false;                                           // (wave uniform) an[] holds the current tile
    for (int t = t0; t < t1; ++t) {
        const int nr = nrn;                                     // real rows of tile t (wave uniform)
        const bool run = nr > 0;
        w_v8h a[KS];
        if (run) {
            if (pre) {
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) a[ks] = an[ks];
            } else {                                            // (the split's first tile, or the first behind skipped ones)
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) a[ks] = *(const w_v8h*)(p.redh + (size_t)(t * 16 + lr) * kWideDim + 32 * ks + 8 * lg);
            }
        }
        pre = false;
        nrn = 0;
        if (t + 1 < t1) {
            nrn = sp.st_real[(t + 1) >> 3] - 16 * ((t + 1) & 7);
            pre = nrn > 0;
            if (pre) {
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) an[ks] = *(const w_v8h*)(p.redh + (size_t)((t + 1) * 16 + lr) * kWideDim + 32 * ks + 8 * lg);
            }
        }
        if (!run) continue;
        const int r0 = t * 16 + 4 * lg;                         // this lane's 4 reduced rows (physical rows of the stack)
        const float4 ax4 = *(const float4*)(p.redaux + r0);
        const float ax[4] = {ax4.x, ax4.y, ax4.z, ax4.w};
#pragma unroll
        for (int b = 0; b < kWFBlocks; ++b) {
            w_v4f acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[ks], bq[b][ks], acc, 0, 0, 0);
            const int col = c0 + 16 * b + lr;
            float sc[4];
            bool real[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                sc[r] = __builtin_fmaf(acc[r], p.cscale, ax[r]);
                real[r] = 4 * lg + r < nr && col < p.ncols;
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
            for (int r = 0; r < 4; ++r) wide_push(real[r] && sc[r] >= bnd[b] - marg[b], col, r0 + r, sc[r], p, lbase, lused);
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

struct WideStackExactParams {
    WideExactParams e;                // (nred is not read)
    const int32_t* st_real;           // [e.nsteps / 2]
};

template <int KTOP>
__global__ __launch_bounds__(256)
void wide_stack_exact_kernel(WideStackExactParams sp)
{
    __shared__ __attribute__((aligned(16))) float colimg[kWideDim * kWLd];
    __shared__ __attribute__((aligned(16))) float redimg[kWHalf * kWLd];

    const WideExactParams& p = sp.e;
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
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        thr[i] = INFINITY;
#pragma unroll
        for (int k = 0; k < KTOP; ++k) { bd[i][k] = INFINITY; bi[i][k] = -1; }
    }

    const int s0 = split * p.steps_per_split;
    const int s1 = min(s0 + p.steps_per_split, p.nsteps);
    for (int st = s0; st < s1; ++st) {
        // the step's 64 rows are one half of stage st >> 1 (st < nsteps = 2 stages' worth: the word exists); uniform over the
        // workgroup, so every thread passes the same barriers
        const int nr = sp.st_real[st >> 1] - kWTile * (st & 1);
        if (nr <= 0) continue;
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
                    // (NaN fails the compare; +inf passes it and fails d < bd: neither is ever listed)
                    if (4 * tm + j < nr && s[i][j] <= thr[i]) {
                        const int idx = m0 + j;
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

// Top-2 alone is instantiated: the stacked calls' merge (coll_merge2_kernel) takes [..][2] keys, and k = 1 is the first column of
// the top-2 lists, as it is in fm_collection_knn.
constexpr int kWSTop = 2;

template <int KS>
static void wide_stack_filter_launch(const WideStackFilterParams& sp, int grid, hipStream_t stream)
{
    hipLaunchKernelGGL((wide_stack_filter_kernel<KS, kWSTop>), dim3(grid), dim3(256), 0, stream, sp);
}

// (the kernels index the table by tile and by step: the stack must be whole stages, and the plans must be made for all of it)
static bool wide_stack_shape_ok(const Bank& stack, const int32_t* st_real)
{
    return st_real && stack.n > 0 && stack.n == stack.n_pad && stack.n % kStageRows == 0;
}

hipError_t launch_wide_stack_filter(const Bank& q, const Bank& stack, const int32_t* st_real, const WideFilterPlan& plan, uint2* list,
                                    float* lscore, unsigned* gbound, unsigned long long* cnt, int* flag, unsigned long long* partial,
                                    hipStream_t stream)
{
    const int ks = (q.dim + 31) / 32;
    if (!wide_stack_shape_ok(stack, st_real) || ks < 5 || ks > 8 || plan.ntiles != stack.n_pad / 16) return hipErrorInvalidValue;
    WideStackFilterParams sp;
    WideFilterParams& p = sp.f;
    p.colh = q.wrowsh; p.colnorm = q.normf; p.ncols = (int)q.n;
    p.redh = stack.wrowsh; p.redaux = stack.auxf; p.nred = (int)stack.n;
    const int dk = stack.kscale - q.kscale;
    p.cscale = ldexpf(1.f, dk);
    p.nscale = ldexpf(1.f, 2 * dk);
    p.red_nm_max = stack.nm_max;
    p.ntiles = plan.ntiles; p.tiles_per_split = plan.tiles_per_split; p.nsplit = plan.nsplit;
    p.list = list; p.lscore = lscore; p.cap = plan.cap; p.cnt = cnt; p.gbound = gbound;
    sp.st_real = st_real;
    const int grid = plan.nchunks * plan.nsplit;
    switch (ks) {
        case 5: wide_stack_filter_launch<5>(sp, grid, stream); break;
        case 6: wide_stack_filter_launch<6>(sp, grid, stream); break;
        case 7: wide_stack_filter_launch<7>(sp, grid, stream); break;
        default: wide_stack_filter_launch<8>(sp, grid, stream); break;
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_wide_rescore(q, stack, kWSTop, plan.cap, list, lscore, gbound, cnt, flag, partial, stream);
}

hipError_t launch_wide_stack_exact(const Bank& q, const Bank& stack, const int32_t* st_real, const RowReducePlan& plan,
                                   unsigned long long* partial, const int* run_flag, hipStream_t stream)
{
    if (!wide_stack_shape_ok(stack, st_real) || q.n <= 0) return hipErrorInvalidValue;
    WideStackExactParams sp;
    WideExactParams& p = sp.e;
    p.run_flag = run_flag;
    p.col_rows = q.wrows;
    p.ncols_pad = (int)q.n_pad;
    p.red_rows = stack.wrows;
    p.nred = (int)stack.n;
    p.nsteps = (int)(stack.n_pad / kWTile);
    p.nred_pad = (int)stack.n_pad;
    p.nsplit = plan.nsplit;
    p.steps_per_split = plan.stages_per_split;
    p.ncols_alloc = plan.ncols_alloc;
    p.kend = (q.dim + 7) & ~7;
    p.partial = partial;
    sp.st_real = st_real;
    const int grid = plan.nchunks * plan.nsplit;
    hipLaunchKernelGGL((wide_stack_exact_kernel<kWSTop>), dim3(grid), dim3(256), 0, stream, sp);
    return hipGetLastError();
}

}  // namespace fm
