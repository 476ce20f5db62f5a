// C-ABI of libfastmatch_hip.so (include/fastmatch_hip.h), part 2: the matcher entry points and the small kernels
// around K1 --
//   top-2 merge of the split partials for knnMatch(k = 2), Lowe ratio
//   cross-check: election (reverse-NN partials -> 64-bit scatter-min), decode + float64 ratio + threshold,
//   ordered compaction of the accepted matches (host arrays or 12-byte device rows; compact_slot, ctx_internal.h)
//   exact repair of float32-root ties (sqrt_fix_kernel)
// and the pipelines built from them.  One pair's sweep is sweep_pair; the tail behind a reverse top-1 sweep is
//   xcheck_keys_device (fill, sweep, election) -> xcheck1_device (plain decode) | ratio_sync (ratio test, then the delivery
//   its AcceptedSink names) | ratio_enqueue + enqueue_tail (the same on two streams, nothing waits);
// batch_common groups pairs that share distance-kernel launches and calls the same functions; sharded election keys and
// per-round launches (K4) follow.  DESIGN.md section 4 has the table.
// Reference call sites are cited in the header next to each entry point.
#include "ctx_internal.h"

#include <algorithm>

using namespace fm;

// ---------------------------------------------------------------------------------------
// merge / finalise kernels
// ---------------------------------------------------------------------------------------
// knnMatch(k=2): merge nsplit partial top-2 lists per query row (keys are (d2<<32)|idx,
// ascending = cv::batchDistance order) and emit idx / sqrtf(d2).
// Partial keys carry the exact integer d2 (int8 route) or the float32 bits of the distance
// itself (float32 route) in their high word.  The d2 order is OpenCV's (float32 distance, index)
// order as long as the second best d2 stays below kSqrtTieMin (tile_ops.h); output rows beyond that
// are listed in fix[] (fix[0] = count, rows from fix[4] on) and redone by sqrt_fix_kernel<2>.
__device__ __forceinline__ float key_dist(unsigned long long key, int f32)
{
    const unsigned hi = (unsigned)(key >> 32);
    return f32 ? __uint_as_float(hi) : sqrtf((float)hi);
}

__global__ void knn2_merge_kernel(const unsigned long long* __restrict__ partial, int nsplit,
                                  int ncols_alloc, int64_t n, int32_t* __restrict__ idx,
                                  float* __restrict__ dist, int f32, unsigned* __restrict__ fix = nullptr)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    unsigned long long b0 = ~0ull, b1 = ~0ull;
    for (int s = 0; s < nsplit; ++s) {
        const unsigned long long* p = partial + ((size_t)s * ncols_alloc + i) * 2;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const unsigned long long v = p[k];
            if (v < b0) { b1 = b0; b0 = v; }
            else if (v < b1) { b1 = v; }
        }
    }
    idx[2 * i]     = (b0 == ~0ull) ? -1 : (int32_t)(unsigned)b0;
    idx[2 * i + 1] = (b1 == ~0ull) ? -1 : (int32_t)(unsigned)b1;
    dist[2 * i]     = (b0 == ~0ull) ? INFINITY : key_dist(b0, f32);
    dist[2 * i + 1] = (b1 == ~0ull) ? INFINITY : key_dist(b1, f32);
    // The float32 order can differ from the d2 order only if the root class of the best or of the 2nd best d2
    // has a second member (d2 - 1 or d2 + 1 shares its root): only then can a candidate outside this list, or
    // the other list entry, tie with it and win on its index.
    if (fix && b1 != ~0ull && (unsigned)(b1 >> 32) >= kSqrtTieMin) {
        const unsigned e0 = (unsigned)(b0 >> 32), e1 = (unsigned)(b1 >> 32);
        const bool paired1 = sqrt_ties_up(e1) || sqrt_ties_up(e1 - 1u);
        const bool paired0 = e0 >= kSqrtTieMin && (sqrt_ties_up(e0) || sqrt_ties_up(e0 - 1u));
        if (paired0 || paired1) fix[4 + atomicAdd(fix, 1u)] = (unsigned)i;
    }
}

// Exact repair of the output rows listed in fix[] (see knn2_merge_kernel / xcheck_scatter_kernel): one
// workgroup per listed row scans ALL reduced rows with exact integer arithmetic and orders them the way
// cv::batchDistance does, by (float32 bits of sqrtf(d2), index).  KTOP = 2: rewrites the row's 2-NN
// list; KTOP = 1: the row is a train row, the winner is the query row it elects -> scatter-min into
// qbest (the step xcheck_scatter_kernel left out for this row).  Cold: rows whose K-th best d2 is
// >= kSqrtTieMin = 4 197 200 (SIFT descriptors: d2 <= 1.05e6).
template <int KTOP>
__global__ __launch_bounds__(256)
void sqrt_fix_kernel(const unsigned* __restrict__ fix, const int8_t* __restrict__ col_rows,
                     const int32_t* __restrict__ col_norm, const int8_t* __restrict__ red_rows,
                     const int32_t* __restrict__ red_norm, int nred,
                     unsigned long long* __restrict__ qbest, unsigned t_offset,
                     int32_t* __restrict__ idx, float* __restrict__ dist,
                     const unsigned long long* __restrict__ red_real = nullptr)      // a grown reduced bank's real rows (Bank::real)
{
    __shared__ unsigned long long best[2];
    const int tid = threadIdx.x;
    const unsigned n = fix[0];
    for (unsigned e = blockIdx.x; e < n; e += gridDim.x) {
        const unsigned c = fix[4 + e];
        if (tid == 0) { best[0] = ~0ull; best[1] = ~0ull; }
        __syncthreads();
        v4i cr[kDim / 16];
#pragma unroll
        for (int w = 0; w < kDim / 16; ++w) cr[w] = *(const v4i*)(col_rows + (size_t)c * kDim + 16 * w);
        const int cn = col_norm[c];
        unsigned long long k0 = ~0ull, k1 = ~0ull;
        for (int m = tid; m < nred; m += 256) {
            if (red_real && !real_row(red_real, m)) continue;
            int dot = 0;
#pragma unroll
            for (int w = 0; w < kDim / 16; ++w) {
                const v4i y = *(const v4i*)(red_rows + (size_t)m * kDim + 16 * w);
#pragma unroll
                for (int u = 0; u < 4; ++u) dot = __builtin_amdgcn_sdot4(cr[w][u], y[u], dot, false);
            }
            const unsigned d2 = (unsigned)(cn + red_norm[m] - 2 * dot);
            const unsigned long long key = ((unsigned long long)sqrt_bits(d2) << 32) | (unsigned)m;
            if (key < k0) { k1 = k0; k0 = key; }
            else if (key < k1) k1 = key;
        }
        if (k0 != ~0ull) atomicMin(&best[0], k0);
        __syncthreads();
        const unsigned long long g0 = best[0];
        if constexpr (KTOP == 2) {
            const unsigned long long mine = (k0 == g0) ? k1 : k0;
            if (mine != ~0ull) atomicMin(&best[1], mine);
            __syncthreads();
            if (tid == 0) {
                const unsigned long long g1 = best[1];
                idx[2 * (size_t)c]     = (g0 == ~0ull) ? -1 : (int32_t)(unsigned)g0;
                idx[2 * (size_t)c + 1] = (g1 == ~0ull) ? -1 : (int32_t)(unsigned)g1;
                dist[2 * (size_t)c]     = (g0 == ~0ull) ? INFINITY : __uint_as_float((unsigned)(g0 >> 32));
                dist[2 * (size_t)c + 1] = (g1 == ~0ull) ? INFINITY : __uint_as_float((unsigned)(g1 >> 32));
            }
        } else {
            if (tid == 0 && g0 != ~0ull)
                atomicMin(&qbest[(unsigned)g0], (g0 & 0xffffffff00000000ull) | (unsigned long long)(c + t_offset));
        }
        __syncthreads();
    }
}

// Cross-check step 2: train row t elects rq = argmin_q d(q,t)
// (lowest q on ties) = min over the split partials; then scatter-min of (d2<<32 | t)
// into qbest[rq]: q keeps the closest electing train row, lowest t on ties.  64-bit
// atomicMin is order independent, so the result is deterministic.  The key's high word is the float32
// distance (bits of sqrtf(d2); f32: the partial keys carry those bits already): OpenCV compares the
// distances, and above kSqrtTieMin two d2 can share one.  fix != null: a train row whose best d2 shares
// its root with d2 + 1 may elect a LOWER query index that sits at d2 + 1 -- it is listed in fix[] and
// left to sqrt_fix_kernel<1>.
// bound_reset (async calls): the K1 that produced `partial` is complete, so its bound[] array is
// put back to "no bound" here for the next K1 that uses this workspace slot.
__global__ void xcheck_scatter_kernel(const unsigned long long* __restrict__ partial, int nsplit,
                                      int ncols_alloc, int64_t nt,
                                      unsigned long long* __restrict__ qbest, unsigned t_offset, int f32,
                                      int* __restrict__ bound_reset, unsigned* __restrict__ fix)
{
    // four lanes per train row, each takes every 4th split: short independent load chains
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (bound_reset && gid < ncols_alloc) bound_reset[gid] = INT32_MIN;
    const int64_t t = gid >> 2;
    const int part = (int)(gid & 3);
    unsigned long long b = ~0ull;
    if (t < nt) {
        for (int s = part; s < nsplit; s += 4) {
            const unsigned long long v = partial[(size_t)s * ncols_alloc + t];
            b = v < b ? v : b;
        }
    }
    unsigned long long o = __shfl_xor(b, 1);
    b = o < b ? o : b;
    o = __shfl_xor(b, 2);
    b = o < b ? o : b;
    if (t >= nt || part != 0 || b == ~0ull) return;
    const unsigned q = (unsigned)b;
    unsigned hi = (unsigned)(b >> 32);
    if (!f32) {
        if (fix && hi >= kSqrtTieMin && sqrt_ties_up(hi)) { fix[4 + atomicAdd(fix, 1u)] = (unsigned)t; return; }
        hi = sqrt_bits(hi);
    }
    // (t_offset: global index of this bank's first row when the train set is sharded over ranks)
    const unsigned long long key = ((unsigned long long)hi << 32) | (unsigned long long)((unsigned)t + t_offset);
    atomicMin(&qbest[q], key);
}

// A grown train bank in front of the election: its gap rows (padding inside the bank, Bank::real) were output rows of the
// reverse sweep like any other and hold a key -- their nearest query row.  They elect nobody: their keys become "none" in
// every split, which xcheck_scatter_kernel skips (and never lists in fix[]).  One thread per (split, 64-row word of the
// bitmap): only the gap rows are written, a word without gaps costs one load.
__global__ void xcheck_blank_gaps_kernel(unsigned long long* __restrict__ partial, int nsplit, int ncols_alloc, int64_t nt,
                                         const unsigned long long* __restrict__ real)
{
    const int64_t nwords = (nt + 63) >> 6;
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t w = gid % nwords;
    const int64_t s = gid / nwords;
    if (s >= nsplit) return;
    const int64_t rows = nt - 64 * w;                           // rows of this word below nt: 1 .. 64 of them
    unsigned long long gaps = ~real[w] & (rows >= 64 ? ~0ull : ((1ull << rows) - 1ull));
    while (gaps) {
        const int b = __ffsll((long long)gaps) - 1;
        partial[(size_t)s * ncols_alloc + 64 * w + b] = ~0ull;
        gaps &= gaps - 1ull;
    }
}

// Cross-check step 3 + optional R1: decode qbest (high word = float32 distance bits), ratio = (double)dist / selfdist[q] in float64, pass = ratio < tau
// (fastmatch.pyx:124,165; :50,75,82).
__global__ void xcheck_finalize_kernel(const unsigned long long* qbest, int64_t nq,
                                       const double* __restrict__ selfdist, double tau,
                                       int32_t* __restrict__ tidx, float* __restrict__ dist,
                                       double* __restrict__ ratio, uint8_t* __restrict__ pass,
                                       unsigned long long* __restrict__ npass,
                                       int* __restrict__ block_counts,
                                       unsigned long long* qbest_reset = nullptr)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool p = false;
    if (q < nq) {
        const unsigned long long key = qbest[q];
        if (qbest_reset) qbest_reset[q] = ~0ull;     // (async calls: the slot's table is left empty for its next election)
        int32_t ti = -1;
        float d = INFINITY;
        double r = NAN;
        if (key != ~0ull) {
            ti = (int32_t)(unsigned)key;
            d = __uint_as_float((unsigned)(key >> 32));
            if (selfdist) { r = (double)d / selfdist[q]; p = r < tau; }
        }
        tidx[q] = ti;
        dist[q] = d;
        if (ratio) ratio[q] = r;
        if (pass) pass[q] = p ? 1 : 0;
    }
    const unsigned long long m = __ballot(p);
    if (npass && !block_counts) {            // (with block counts the total comes from compact_kernel)
        if ((threadIdx.x & 63) == 0 && m) atomicAdd(npass, (unsigned long long)__popcll(m));
    }
    if (block_counts) emit_block_count(m, block_counts);      // for the ordered compaction (compact_kernel)
}

// Ordered stream compaction of the accepted matches (ascending query index; compact_slot, ctx_internal.h) into the
// caller's four arrays.
__global__ void compact_kernel(const int32_t* __restrict__ tidx, const float* __restrict__ dist,
                               const double* __restrict__ ratio, const uint8_t* __restrict__ pass,
                               const int* __restrict__ block_counts, int64_t nq, int64_t cap,
                               int32_t* __restrict__ o_q, int32_t* __restrict__ o_t,
                               float* __restrict__ o_d, double* __restrict__ o_r,
                               unsigned long long* __restrict__ npass)
{
    int64_t q, total;
    bool p;
    const int64_t dst = compact_slot(block_counts, pass, nq, &q, &p, &total);
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) *npass = (unsigned long long)total;
    if (p && dst < cap) { o_q[dst] = (int32_t)q; o_t[dst] = tidx[q]; o_d[dst] = dist[q]; o_r[dst] = ratio[q]; }
}

// Same ordered compaction, but into the 12-byte rows the multi-GPU result gather ships
// (query index, train index, float32 distance bits) in a caller-supplied DEVICE buffer, with
// the count as a device word next to it (fm_match_accepted_dev): nothing crosses to the host.
__global__ void compact_rows_kernel(const int32_t* __restrict__ tidx, const float* __restrict__ dist,
                                    const uint8_t* __restrict__ pass, const int* __restrict__ block_counts,
                                    int64_t nq, int64_t cap, int32_t* __restrict__ o_rows,
                                    long long* __restrict__ o_count, unsigned long long* __restrict__ h_count)
{
    int64_t q, total;
    bool p;
    const int64_t dst = compact_slot(block_counts, pass, nq, &q, &p, &total);
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
        // the device word counts the rows that are THERE (what a consumer of o_rows may index: the gather ships
        // it next to the rows); the host word keeps the full number of accepted matches
        *o_count = total < cap ? (long long)total : (long long)cap;
        if (h_count) *h_count = (unsigned long long)total;
    }
    if (p && dst < cap) {
        o_rows[3 * dst] = (int32_t)q;
        o_rows[3 * dst + 1] = tidx[q];
        o_rows[3 * dst + 2] = (int32_t)__float_as_uint(dist[q]);
    }
}

__global__ void ratio_filter_kernel(const float* __restrict__ dist, const double* __restrict__ selfdist,
                                    const int32_t* __restrict__ qrows, int64_t n, double tau,
                                    double* __restrict__ ratio, uint8_t* __restrict__ pass,
                                    unsigned long long* __restrict__ npass)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool p = false;
    if (i < n) {
        const int64_t q = qrows ? qrows[i] : i;
        const double r = (double)dist[i] / selfdist[q];
        p = r < tau;
        if (ratio) ratio[i] = r;
        if (pass) pass[i] = p ? 1 : 0;
    }
    const unsigned long long m = __ballot(p);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(npass, (unsigned long long)__popcll(m));
}

// Classic Ratio-Match (Classic Matching.ipynb cell 3): ratio = float64(d1) / float64(d2) of
// the 2-NN list, accepted when ratio < tau (d2 == 0 gives inf / nan: rejected, where the
// notebook's Python division would raise).  Feeds compact_kernel.
__global__ void lowe_kernel(const int32_t* __restrict__ idx2, const float* __restrict__ dist2, int64_t nq,
                            double tau, int32_t* __restrict__ tidx, float* __restrict__ dist,
                            double* __restrict__ ratio, uint8_t* __restrict__ pass,
                            int* __restrict__ block_counts)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool p = false;
    if (q < nq) {
        const float d1 = dist2[2 * q], d2 = dist2[2 * q + 1];
        const double r = (idx2[2 * q + 1] >= 0) ? (double)d1 / (double)d2 : NAN;
        p = r < tau;
        tidx[q] = idx2[2 * q];
        dist[q] = d1;
        ratio[q] = r;
        pass[q] = p ? 1 : 0;
    }
    emit_block_count(__ballot(p), block_counts);
}

// Self distances (cache.pyx:250-252, 271-273: [r[1].distance for r in bf_match(d, d, k = 2)]) from the split partials
// of the masked-diagonal top-1: row i's value is the float32 distance to its nearest OTHER row, as float64; +inf
// for a bank of one row.  Only the value is kept, so the float32-root ties of the integer route need no repair
// (the smallest root is the root of the smallest d2).  Up to kRRBatchMax banks of one shape per launch
// (blockIdx.y); bound_reset: the sweep is complete, its bound[] array goes back to "no bound".
__global__ void selfdist_from_knn_kernel(const float* __restrict__ dist2, int64_t n, double* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (double)dist2[2 * i + 1];
}

// Bank::sdmax: the maximum of the self distances' bit patterns (>= 0 for every value that allows a ratio cut, so the
// unsigned order of the patterns is the order of the values; inf, NaN and sign bits land at or above +inf's pattern,
// which ratio_cut_d2 reads as "no cut").  *out is 0 on entry.
__global__ __launch_bounds__(256)
void selfdist_max_kernel(const double* __restrict__ sd, int64_t n, unsigned long long* __restrict__ out)
{
    unsigned long long m = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const unsigned long long b = (unsigned long long)__double_as_longlong(sd[i]);
        m = b > m ? b : m;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long x = __shfl_xor(m, o);
        m = x > m ? x : m;
    }
    if ((threadIdx.x & 63) == 0 && m != 0) atomicMax(out, m);
}

int fm::enqueue_selfdist_max(fm_ctx* ctx, fm_bank* b, hipStream_t stream)
{
    if (!b->sdmax) return FM_OK;
    HIP_TRY(ctx, hipMemsetAsync(b->sdmax, 0, 8, stream));
    if (b->n > 0) {
        const int64_t blocks = (b->n + 255) / 256;
        hipLaunchKernelGGL(selfdist_max_kernel, dim3((unsigned)(blocks < 256 ? blocks : 256)), dim3(256), 0, stream,
                           (const double*)b->selfdist, b->n, b->sdmax);
        HIP_TRY(ctx, hipGetLastError());
    }
    b->sdmax_rows = b->n;
    return FM_OK;
}

// D* of the ratio test (ratio_cut.h) for the pairs of one K1 launch, from their query banks' largest self distances:
// out[i] for every pair with sdmax[i] != null.
struct CutArgs {
    const unsigned long long* sdmax[kRRBatchMax];
    unsigned* out;
    double tau;
    int n;
};

__global__ void ratio_cut_kernel(CutArgs a)
{
    const int i = threadIdx.x;
    if (i < a.n && a.sdmax[i]) a.out[i] = ratio_cut_d2(__longlong_as_double((long long)*a.sdmax[i]), a.tau);
}

// The accepted-only calls: the cut words of pairs (q[i], -) into the other set of ctx->d_cut than the last call's, enqueued
// on ctx->stream in front of their K1 (which reads them on the same stream) and behind the rescoring that read that set
// last, if it ran beside the stream.  cut[i] = null for a pair without one: a query bank whose self distances were not
// reduced for all of its current rows (a refill to more rows than they were computed for), or no device words.
int enqueue_ratio_cut(fm_ctx* ctx, int n, const fm_bank* const* q, double tau, const unsigned** cut)
{
    CutArgs a{};
    bool any = false;
    ctx->cut_tau_ok = tau == tau;
    const int set = ctx->f6_set ^ 1;
    unsigned* const words = ctx->d_cut ? ctx->d_cut + set * kRRBatchMax : nullptr;
    for (int i = 0; i < n; ++i) {
        const fm_bank* b = q[i];
        const bool ok = words && b->kind == FM_BANK_I8 && b->sdmax && b->sdmax_rows >= b->n;
        a.sdmax[i] = ok ? b->sdmax : nullptr;
        cut[i] = ok ? words + i : nullptr;
        any = any || ok;
    }
    if (!any) return FM_OK;
    ctx->f6_set = set;
    if (ctx->f6_off_stream[set]) {
        HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_f6_done[set], 0));
        ctx->f6_off_stream[set] = false;
    }
    a.out = words;
    a.tau = tau;
    a.n = n;
    hipLaunchKernelGGL(ratio_cut_kernel, dim3(1), dim3(64), 0, ctx->stream, a);
    HIP_TRY(ctx, hipGetLastError());
    return FM_OK;
}

const Filter6Ws* filter6_ws(fm_ctx* ctx, int n)
{
    if (ctx->tune.fp6_filter == 0 || !ctx->cut_tau_ok || n < 1 || n > kRRBatchMax) return nullptr;
    const size_t cap = (size_t)ctx->tune.fp6_cap;
    const int set = ctx->f6_set;             // (the cut words' set: its last rescoring is already waited for)
    // (a larger list is a new allocation: hipFree waits for the launches that still read the old one)
    if (ws_ensure(ctx, &ctx->ws_f6[set], &ctx->ws_f6_bytes[set], 256 + (size_t)n * cap * 8) != FM_OK) { (void)hipGetLastError(); return nullptr; }
    ctx->f6.cnt = (unsigned*)ctx->ws_f6[set];
    ctx->f6.rec = (uint2*)((char*)ctx->ws_f6[set] + 256);
    ctx->f6.cap = (unsigned)cap;
    ctx->f6.nsplit = ctx->tune.fp6_nsplit > 0 ? ctx->tune.fp6_nsplit : ctx->tune.nsplit > 0 ? -1 : 0;
    ctx->f6.resident = ctx->ncu > 0 ? ctx->ncu : 256;
    ctx->f6.side = nullptr;  ctx->f6.ev_sweep = ctx->f6.ev_done = nullptr;
    ctx->f6_last_n = n;
    return &ctx->f6;
}

struct SelfMerge {
    const unsigned long long* partial[kRRBatchMax];
    double* out[kRRBatchMax];
    int*    bound_reset[kRRBatchMax];
};

__global__ void selfdist_merge_kernel(SelfMerge m, int nsplit, int ncols_alloc, int64_t n, int f32)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int b = blockIdx.y;
    if (m.bound_reset[b] && i < ncols_alloc) m.bound_reset[b][i] = INT32_MIN;
    if (i >= n) return;
    const unsigned long long* p = m.partial[b];
    unsigned long long k = ~0ull;
    for (int s = 0; s < nsplit; ++s) {
        const unsigned long long v = p[(size_t)s * ncols_alloc + i];
        k = v < k ? v : k;
    }
    m.out[b][i] = (k == ~0ull) ? (double)INFINITY : (double)key_dist(k, f32);
}

// The triangular self sweep (rowreduce.hip, TRI) leaves, per row, the best hi it has reached as an output row in
// bound[]: d2 = |row|^2 + 1 - bound; a word at or below kTriNoBoundHost met no real row (a bank of one row).
struct TriFinish {
    const int* bound[kRRBatchMax];
    const int32_t* norm[kRRBatchMax];
    double* out[kRRBatchMax];
    int64_t n[kRRBatchMax];
};

__global__ void selfdist_tri_finish_kernel(TriFinish m)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int b = blockIdx.y;
    if (i >= m.n[b]) return;
    const int h = m.bound[b][i];
    m.out[b][i] = (h > kTriNoBoundHost) ? (double)sqrtf((float)(unsigned)(m.norm[b][i] + 1 - h)) : (double)INFINITY;
}

extern "C" int fm_self_dist_plan(int64_t n_pad, int32_t stages, int32_t* table, int64_t cap, int32_t* n_workgroups,
                                 int32_t* n_diag, int32_t* stages_used)
{
    if (n_pad < kStageRows || n_pad % kStageRows != 0 || n_pad > kTriMaxRows || stages < 0 || cap < 0 || (cap > 0 && !table))
        return fail(nullptr, FM_EINVAL, "fm_self_dist_plan: n_pad must be a positive multiple of 128 up to 2^26, stages >= 0");
    try {
        // (the count-only call -- cap 0 -- builds no table: 16 bytes per workgroup, a million of them for a 3M-row bank)
        std::vector<int> tb;
        const TriPlan pl = plan_tri(n_pad, stages, cap > 0 ? &tb : nullptr);
        if (n_workgroups) *n_workgroups = pl.npieces;
        if (n_diag) *n_diag = pl.ndiag;
        if (stages_used) *stages_used = pl.stages;
        const int64_t m = cap < pl.npieces ? cap : pl.npieces;
        for (int64_t i = 0; i < 4 * m; ++i) table[i] = tb[(size_t)i];
    } catch (const std::bad_alloc&) {
        return fail(nullptr, FM_ENOMEM, "fm_self_dist_plan: out of host memory");
    }
    return FM_OK;
}

// The triangular sweep's plan of a bank size: piece length and workgroup counts by arithmetic (plan_tri, api_grid.hip); the
// workgroups themselves follow from (chunks, stages, piece length) in the kernel (tri_entry, rowreduce.hip), so a plan owns
// no device memory (r05, last) and the context keeps plans only to spare the arithmetic of a size it has seen.
static int tri_plan_for(fm_ctx* ctx, int64_t n_pad, TriPlan* out)
{
    const std::pair<int64_t, int> key(n_pad, ctx->tune.tri_stages * 2048 + ctx->tune.bound_every);
    auto it = ctx->tri_plans.find(key);
    if (it != ctx->tri_plans.end()) { *out = it->second; return FM_OK; }
    if (ctx->tri_plans.size() >= 4096) ctx->tri_plans.clear();
    TriPlan pl = plan_tri(n_pad, ctx->tune.tri_stages, nullptr);
    pl.bound_every = 1;
    for (int b = 2; b <= 1024; b <<= 1) if (ctx->tune.bound_every == b) pl.bound_every = b;
    ctx->tri_plans[key] = pl;
    *out = pl;
    return FM_OK;
}

// ---------------------------------------------------------------------------------------
// float32 route: K5 alone, or the fp16 filter (K8) with K5 as its conditional fallback
// ---------------------------------------------------------------------------------------
// Leaves the packed keys in ws_partial in `pl`'s layout (K5's plan) either way.
int rowreduce_f32_route(fm_ctx* ctx, const fm_bank* cols, const fm_bank* red, int ktop, RowReducePlan* pl_out, bool self)
{
    const RowReducePlan pl = plan_rowreduce_f32(cols->n_pad, red->n_pad, ctx->tune.nsplit);
    *pl_out = pl;
    const bool filter = ctx->tune.f32_filter != 0 && filter_usable(*cols, *red) &&
                        (ctx->tune.f32_filter >= 2 || (double)cols->n * (double)red->n >= 4.0e6);
    const size_t part = (pl.partial_bytes(ktop) + 255) & ~(size_t)255;
    if (!filter) {
        int rc = ws_ensure(ctx, &ctx->ws_partial, &ctx->ws_partial_bytes, part);
        if (rc != FM_OK) return rc;
        HIP_TRY(ctx, hipEventRecord(ctx->ev_k0, ctx->stream));
        HIP_TRY(ctx, launch_rowreduce_f32(*cols, *red, ktop, pl, (unsigned long long*)ctx->ws_partial, nullptr, ctx->stream, self));
        HIP_TRY(ctx, hipEventRecord(ctx->ev_k1, ctx->stream));
        return FM_OK;
    }
    const FilterPlan fp = plan_filter(cols->n_pad, red->n_pad, ctx->tune);
    const size_t bnd = (fp.bound_bytes() + 255) & ~(size_t)255;
    int rc = ws_ensure(ctx, &ctx->ws_partial, &ctx->ws_partial_bytes, part + fp.slots_bytes() + bnd + fp.aux_bytes() + 64);
    if (rc != FM_OK) return rc;
    unsigned long long* d_part = (unsigned long long*)ctx->ws_partial;
    unsigned long long* d_slots = (unsigned long long*)((char*)ctx->ws_partial + part);
    int* d_bound = (int*)((char*)d_slots + fp.slots_bytes());
    float* d_aux = (float*)((char*)d_bound + bnd);
    HIP_TRY(ctx, hipMemsetAsync(d_part, 0xff, pl.partial_bytes(ktop), ctx->stream));
    HIP_TRY(ctx, hipMemsetD32Async((hipDeviceptr_t)d_bound, filter_empty_bound(), (size_t)fp.ncols_alloc * 2, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(ctx->d_counters, 0, 8, ctx->stream));
    HIP_TRY(ctx, hipEventRecord(ctx->ev_k0, ctx->stream));
    HIP_TRY(ctx, launch_filter(*cols, *red, ktop, fp, d_slots, d_bound, ctx->d_counters, d_part, ctx->stream, self, d_aux));
    HIP_TRY(ctx, launch_rowreduce_f32(*cols, *red, ktop, pl, d_part, ctx->d_counters, ctx->stream, self));
    HIP_TRY(ctx, hipEventRecord(ctx->ev_k1, ctx->stream));
    ctx->filter_launches += 1;
    return FM_OK;
}

// Wide float banks (K14, wide_f32.hip), the same way: the exact kernel alone, or the fp16 filter with the exact kernel as its
// conditional fallback (a record list that overflowed); "f32_filter" decides as above.  ws_partial: partial | records | their
// scores | per-row bounds | count.  self (cols and red are one bank, ktop 1): the SELF forms of the three kernels, which drop
// the diagonal by index -- fm_wide_self_dist's sweep.
static int wide_route(fm_ctx* ctx, const Bank& cols, const Bank& red, int ktop, RowReducePlan* pl_out, bool self = false)
{
    const RowReducePlan pl = plan_rowreduce_f32(cols.n_pad, red.n_pad, ctx->tune.nsplit);
    *pl_out = pl;
    const WideFilterPlan fp = plan_wide_filter(cols.n_pad, cols.n, red.n_pad, ctx->tune);
    // (a split records its first tile whole -- 16 records per output row, fewer only where the reduced bank is shorter than a
    // tile -- and the list ends at 2^24 records: from 2^20 output rows on it overflows in every call, with one split already,
    // the filter's sweep is wasted and the exact kernel redoes the call.  Such a call goes to the exact kernel at once.)
    const bool filter = ctx->tune.f32_filter != 0 && ctx->d_counters && wide_filter_usable(cols, red) &&
                        (ctx->tune.f32_filter >= 2 || (double)cols.n * (double)red.n >= 4.0e6) &&
                        cols.n * std::min<int64_t>(16, red.n) <= (int64_t)fp.cap;
    unsigned long long* d_part;
    int rc;
    if (!filter) {
        if ((rc = ws_ensure(ctx, &ctx->ws_partial, &ctx->ws_partial_bytes, pl.partial_bytes(ktop) + 64)) != FM_OK) return rc;
        d_part = (unsigned long long*)ctx->ws_partial;
        HIP_TRY(ctx, hipEventRecord(ctx->ev_k0, ctx->stream));
        HIP_TRY(ctx, launch_wide_exact(cols, red, ktop, pl, d_part, nullptr, ctx->stream, self));
        HIP_TRY(ctx, hipEventRecord(ctx->ev_k1, ctx->stream));
        return FM_OK;
    }
    size_t off = 0;
    const size_t o_part = carve(off, pl.partial_bytes(ktop)), o_list = carve(off, fp.list_bytes()), o_score = carve(off, fp.list_bytes() / 2),
                 o_bound = carve(off, (size_t)cols.n_pad * 4), o_cnt = carve(off, 16);
    if ((rc = ws_ensure(ctx, &ctx->ws_partial, &ctx->ws_partial_bytes, off + 64)) != FM_OK) return rc;
    d_part = (unsigned long long*)((char*)ctx->ws_partial + o_part);
    unsigned long long* d_cnt = (unsigned long long*)((char*)ctx->ws_partial + o_cnt);
    HIP_TRY(ctx, hipMemsetAsync(d_part, 0xff, pl.partial_bytes(ktop), ctx->stream));
    // (the bounds and the count are neighbours: one fill)
    HIP_TRY(ctx, hipMemsetAsync((char*)ctx->ws_partial + o_bound, 0, o_cnt + 16 - o_bound, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(ctx->d_counters, 0, 8, ctx->stream));
    HIP_TRY(ctx, hipEventRecord(ctx->ev_k0, ctx->stream));
    HIP_TRY(ctx, launch_wide_filter(cols, red, ktop, fp, (uint2*)((char*)ctx->ws_partial + o_list), (float*)((char*)ctx->ws_partial + o_score),
                                    (unsigned*)((char*)ctx->ws_partial + o_bound), d_cnt, ctx->d_counters, d_part, ctx->stream, self));
    HIP_TRY(ctx, launch_wide_exact(cols, red, ktop, pl, d_part, ctx->d_counters, ctx->stream, self));
    HIP_TRY(ctx, hipEventRecord(ctx->ev_k1, ctx->stream));
    ctx->filter_launches += 1;
    return FM_OK;
}

// ---------------------------------------------------------------------------------------
// one bank pair on the context's stream: every synchronous entry point's sweep (ctx_internal.h)
// ---------------------------------------------------------------------------------------
int sweep_pair_plan(fm_ctx* ctx, const Bank& cols, const Bank& red, int ktop, int64_t fix_rows, PairSweep* out)
{
    PairSweep ps{};
    size_t off = 0;
    if (cols.kind == FM_BANK_BIN || cols.kind == FM_BANK_BIN2) {      // (K11b takes K11's plan)
        ps.ham = plan_hamming(cols.n_pad, red.n_pad);
        ps.nsplit = ps.ham.nsplit; ps.ncols_alloc = ps.ham.ncols_alloc; ps.f32_keys = 1;
        carve(off, ps.ham.partial_bytes(ktop));
    } else {
        ps.rr = plan_rowreduce(cols.n_pad, red.n_pad, ctx->tune);
        ps.nsplit = ps.rr.nsplit; ps.ncols_alloc = ps.rr.ncols_alloc; ps.f32_keys = 0;
        carve(off, ps.rr.partial_bytes(ktop));
    }
    const bool coop = cols.kind == FM_BANK_I8 && ctx->tune.coop != 0 && ps.nsplit > 1;
    const bool ties = cols.kind == FM_BANK_I8 && fix_rows > 0 && sqrt_tie_possible(cols, red);
    const size_t o_bound = coop ? carve(off, ps.rr.bound_bytes()) : 0;
    const size_t o_fix = ties ? carve(off, fix_bytes(fix_rows)) : 0;
    int rc = ws_ensure(ctx, &ctx->ws_partial, &ctx->ws_partial_bytes, off + 64);
    if (rc != FM_OK) return rc;
    ps.partial = (const unsigned long long*)ctx->ws_partial;
    ps.bound = coop ? (int*)((char*)ctx->ws_partial + o_bound) : nullptr;
    ps.fix = ties ? (unsigned*)((char*)ctx->ws_partial + o_fix) : nullptr;
    *out = ps;
    return FM_OK;
}

int sweep_pair_run(fm_ctx* ctx, const Bank& cols, const Bank& red, int ktop, const unsigned* cut, const int* stage_real,
                   unsigned flags, const PairSweep& ps)
{
    const bool events = !(flags & kSweepNoEvents);
    if (events) HIP_TRY(ctx, hipEventRecord(ctx->ev_k0, ctx->stream));
    if (cols.kind == FM_BANK_BIN)
        HIP_TRY(ctx, launch_hamming(cols, red, ktop, ps.ham, (unsigned long long*)ctx->ws_partial, ctx->stream, stage_real));
    else if (cols.kind == FM_BANK_BIN2)
        HIP_TRY(ctx, launch_hamming2(cols, red, ktop, ps.ham, (unsigned long long*)ctx->ws_partial, ctx->stream, stage_real));
    else
        HIP_TRY(ctx, launch_rowreduce(cols, red, ktop, ps.rr, (unsigned long long*)ctx->ws_partial, ps.bound, ctx->tune.glds != 0, ctx->stream, cut,
                                      (cut && ktop == 1) ? filter6_ws(ctx, 1) : nullptr));
    if (events) {
        HIP_TRY(ctx, hipEventRecord(ctx->ev_k1, ctx->stream));
        ctx->kernel_timed = true;
    }
    return FM_OK;
}

int sweep_pair(fm_ctx* ctx, const Bank& cols, const Bank& red, int ktop, int64_t fix_rows, const unsigned* cut,
               const int* stage_real, unsigned flags, PairSweep* out)
{
    int rc;
    if (cols.kind == FM_BANK_F32) {
        // (K5's layout has neither shared bounds nor a tie list behind it, and needs none; the route records ev_k0 / ev_k1 itself)
        RowReducePlan pl;
        if ((rc = rowreduce_f32_route(ctx, static_cast<const fm_bank*>(&cols), static_cast<const fm_bank*>(&red), ktop, &pl)) != FM_OK) return rc;
        *out = PairSweep{};
        out->partial = (const unsigned long long*)ctx->ws_partial;
        out->nsplit = pl.nsplit; out->ncols_alloc = pl.ncols_alloc; out->f32_keys = 1;
        if (!(flags & kSweepNoEvents)) ctx->kernel_timed = true;
    } else if (cols.kind == FM_BANK_F32W) {
        RowReducePlan pl;
        if ((rc = wide_route(ctx, cols, red, ktop, &pl)) != FM_OK) return rc;
        *out = PairSweep{};
        out->partial = (const unsigned long long*)ctx->ws_partial;
        out->nsplit = pl.nsplit; out->ncols_alloc = pl.ncols_alloc; out->f32_keys = 1;
        if (!(flags & kSweepNoEvents)) ctx->kernel_timed = true;
    } else {
        if ((rc = sweep_pair_plan(ctx, cols, red, ktop, fix_rows, out)) != FM_OK) return rc;
        if (out->bound && !ablate_keep_bounds())
            HIP_TRY(ctx, hipMemsetD32Async((hipDeviceptr_t)out->bound, (int)0x80000000, (size_t)ktop * out->ncols_alloc, ctx->stream));
        if (out->fix) HIP_TRY(ctx, hipMemsetAsync(out->fix, 0, 16, ctx->stream));
        if ((rc = sweep_pair_run(ctx, cols, red, ktop, cut, stage_real, flags, *out)) != FM_OK) return rc;
    }
    if (!(flags & kSweepNoCount)) {
        ctx->pending_pairs += cols.n * red.n;
        ctx->pending_bytes += bank_bytes(&cols) + bank_bytes(&red);
    }
    return FM_OK;
}

// ---------------------------------------------------------------------------------------
// float32-root ties of the integer route (tile_ops.h: kSqrtTieMin)
// ---------------------------------------------------------------------------------------
// Election of the cross-check on stream s: per train row the minimum over the sweep's split partials ([nsplit][ncols_alloc]
// top-1 keys; f32_keys: PairSweep's), scatter-min into qbest; the rows the scatter lists in fix are then redone exactly.
// fix: zeroed tie list of nt rows for an integer-route pair whose norms allow d2 >= kSqrtTieMin, else null.
// `partial` is the sweep's workspace and read-only here with one exception: for a GROWN train bank (t->real) the election
// first overwrites the keys of the bank's gap rows with "none" in place (xcheck_blank_gaps_kernel) -- the partials are
// consumed by this election and nothing reads them afterwards.
static int enqueue_election(fm_ctx* ctx, hipStream_t s, const fm_bank* q, const fm_bank* t,
                            const unsigned long long* partial, int nsplit, int ncols_alloc, int f32_keys,
                            unsigned long long* qbest, unsigned t_offset, int* bound_reset, unsigned* fix)
{
    const int64_t nt = t->n;
    if (t->real && nt > 0 && nsplit > 0) {          // (a grown train bank only: one more small launch, nothing for any other bank)
        hipLaunchKernelGGL(xcheck_blank_gaps_kernel, dim3((unsigned)((((nt + 63) >> 6) * nsplit + 255) / 256)), dim3(256), 0, s,
                           const_cast<unsigned long long*>(partial), nsplit, ncols_alloc, nt, (const unsigned long long*)t->real);
        HIP_TRY(ctx, hipGetLastError());
    }
    const int64_t sthreads = (bound_reset && (int64_t)ncols_alloc > nt * 4) ? (int64_t)ncols_alloc : nt * 4;
    hipLaunchKernelGGL(xcheck_scatter_kernel, dim3((unsigned)((sthreads + 255) / 256)), dim3(256), 0, s,
                       partial, nsplit, ncols_alloc, nt, qbest, t_offset, f32_keys, bound_reset, fix);
    HIP_TRY(ctx, hipGetLastError());
    if (fix) {
        hipLaunchKernelGGL(sqrt_fix_kernel<1>, dim3(kFixGrid), dim3(256), 0, s, (const unsigned*)fix,
                           (const int8_t*)t->rows8, (const int32_t*)t->norm, (const int8_t*)q->rows8, (const int32_t*)q->norm,
                           (int)q->n, qbest, t_offset, (int32_t*)nullptr, (float*)nullptr, (const unsigned long long*)q->real);
        HIP_TRY(ctx, hipGetLastError());
    }
    return FM_OK;
}

// ---------------------------------------------------------------------------------------
// K7's delegated cross-check: one expansion round's X1 on the whole GPU
// ---------------------------------------------------------------------------------------
// The rows rows[0 .. nq) of bank q gathered into a bank image of their own (rows, norms, aux words in the layout
// bank_prep_kernel writes; slots past nq are padding rows).  One 256-thread block per 32-row tile.
__global__ __launch_bounds__(256)
void gather_rows_kernel(const int32_t* __restrict__ rows, int64_t nq, const int8_t* __restrict__ src8, const int32_t* __restrict__ srcnorm,
                        int8_t* __restrict__ dst8, int32_t* __restrict__ dstnorm, int32_t* __restrict__ dstaux,
                        unsigned long long* __restrict__ qbest, int* __restrict__ bound, int64_t nbound)
{
    const int tid = threadIdx.x, r = tid >> 3, c = tid & 7;
    const int64_t tile = blockIdx.x, slot = tile * kTileRows + r;
    // (the two fills the round's other kernels want, here instead of two fill launches of their own: the election's table
    // and K1's shared bounds)
    if (c == 1 && slot < nq) qbest[slot] = ~0ull;
    if (bound)
        for (int64_t i = (int64_t)blockIdx.x * 256 + tid; i < nbound; i += (int64_t)gridDim.x * 256) bound[i] = (int)0x80000000;
    uint4 w = make_uint4(0, 0, 0, 0);
    int nm = 0;
    if (slot < nq) {
        const int64_t qi = rows[slot];
        w = *(const uint4*)(src8 + qi * kDim + 16 * c);
        nm = srcnorm[qi];
    }
    *(uint4*)(dst8 + slot * kDim + 16 * c) = w;
    if (c == 0) {
        const int sub = r >> 4, rr = r & 15, id = 4 * sub + (rr & 3);
        int32_t* a = dstaux + tile * kAuxPerTile + 32 * sub;
        if (slot < nq) { dstnorm[slot] = nm; a[rr] = -(nm >> 1); a[16 + rr] = ((1 - (nm & 1)) << 4) | (15 - id); }
        else           { dstnorm[slot] = 0;  a[rr] = kPadCinit;  a[16 + rr] = 15 - id; }
    }
}

// The same for a float32 bank: float32 rows, fp16 filter rows, scaled norms and accumulator inits, in the layout
// bank_copy_f32_kernel / bank_prep_f16_kernel write (padding slots: zero rows, init -3.4e38).  16 rows per 256-thread block.
__global__ __launch_bounds__(256)
void gather_rows_f32_kernel(const int32_t* __restrict__ rows, int64_t nq, const float* __restrict__ srcf, const uint16_t* __restrict__ srch,
                            const float* __restrict__ srcnorm, const float* __restrict__ srcaux, float* __restrict__ dstf,
                            uint16_t* __restrict__ dsth, float* __restrict__ dstnorm, float* __restrict__ dstaux,
                            unsigned long long* __restrict__ qbest)
{
    const int r = threadIdx.x >> 4, c = threadIdx.x & 15;
    const int64_t slot = (int64_t)blockIdx.x * 16 + r;
    float4 f0 = make_float4(0.f, 0.f, 0.f, 0.f), f1 = f0;
    uint4 h = make_uint4(0, 0, 0, 0);
    float nm = 0.f, ax = -3.4e38f;
    if (slot < nq) {
        const int64_t qi = rows[slot];
        f0 = *(const float4*)(srcf + qi * kDim + 8 * c);
        f1 = *(const float4*)(srcf + qi * kDim + 8 * c + 4);
        h = *(const uint4*)(srch + qi * kDim + 8 * c);
        nm = srcnorm[qi];
        ax = srcaux[qi];
        if (c == 1) qbest[slot] = ~0ull;
    }
    *(float4*)(dstf + slot * kDim + 8 * c) = f0;
    *(float4*)(dstf + slot * kDim + 8 * c + 4) = f1;
    *(uint4*)(dsth + slot * kDim + 8 * c) = h;
    if (c == 0) { dstnorm[slot] = nm; dstaux[slot] = ax; }
}

// Cross-checked 1-NN of the query subset d_rows[0 .. nq) of bank q against the train rows [t0, t0 + nt) of bank t, the
// way fm_xcheck1 does it on gathered banks (reverse NN by K1 with the train rows as output rows, election by
// scatter-min), into d_qbest[slot] = (float32 distance bits << 32 | local train row), ~0 = unmatched.  Enqueued on the
// context's stream; the workspaces are the context's (ws_out: the gathered bank, ws_partial: K1's partials).  For
// integer-route pairs outside the float32-root tie range (the caller checks).
int fm::round_xcheck_dense(fm_ctx* ctx, const Bank& q, const int32_t* d_rows, int64_t nq, const Bank& t, int64_t t0, int64_t nt,
                           unsigned long long* d_qbest)
{
    if (nq <= 0 || nt <= 0) return FM_OK;
    const int64_t nq_pad = pad128(nq);
    // the gathered rows as a bank in ws_out, and the cell's rows as a bank of their own: a view into the target bank (rows
    // past nt are other cells' rows or padding; what the sweep computes for them is never looked at).  The view is the
    // output side: its aux words are not read, and t0 need not sit on a tile.
    Bank gq, tv = bank_rows_view(t, t0, nt);
    tv.aux = nullptr;
    gq.kind = q.kind; gq.n = nq; gq.dim = q.dim; gq.n_pad = gq.cap_pad = nq_pad;
    size_t off = 0;
    int rc;
    PairSweep ps;
    if (q.kind == FM_BANK_F32) {
        // float32 banks: the gathered rows in the float32 layout, then the float32 route's own cross-check (fp16 filter +
        // exact rescoring, or all pairs for small rounds: rowreduce_f32_route) with the cell's rows as output rows
        const size_t o_f = carve(off, (size_t)nq_pad * kDim * 4), o_h = carve(off, (size_t)nq_pad * kDim * 2),
                     o_n = carve(off, (size_t)nq_pad * 4), o_a = carve(off, (size_t)nq_pad * 4);
        if ((rc = ws_ensure(ctx, &ctx->ws_out, &ctx->ws_out_bytes, off + 64)) != FM_OK) return rc;
        char* b = (char*)ctx->ws_out;
        gq.rowsf = (float*)(b + o_f); gq.rowsh = (uint16_t*)(b + o_h); gq.normf = (float*)(b + o_n); gq.auxf = (float*)(b + o_a);
        gq.nm_max = q.nm_max; gq.kscale = q.kscale; gq.filt_ok = q.filt_ok;
        hipLaunchKernelGGL(gather_rows_f32_kernel, dim3((unsigned)(nq_pad / 16)), dim3(256), 0, ctx->stream, d_rows, nq,
                           (const float*)q.rowsf, (const uint16_t*)q.rowsh, (const float*)q.normf, (const float*)q.auxf,
                           gq.rowsf, gq.rowsh, gq.normf, gq.auxf, d_qbest);
        HIP_TRY(ctx, hipGetLastError());
        if ((rc = sweep_pair(ctx, tv, gq, 1, 0, nullptr, nullptr, kSweepNoEvents | kSweepNoCount, &ps)) != FM_OK) return rc;
    } else {
        const size_t o_rows = carve(off, (size_t)nq_pad * kDim), o_norm = carve(off, (size_t)nq_pad * 4),
                     o_aux = carve(off, (size_t)(nq_pad / kTileRows) * kAuxPerTile * 4);
        if ((rc = ws_ensure(ctx, &ctx->ws_out, &ctx->ws_out_bytes, off + 64)) != FM_OK) return rc;
        char* b = (char*)ctx->ws_out;
        gq.rows8 = (int8_t*)(b + o_rows); gq.norm = (int32_t*)(b + o_norm); gq.aux = (int32_t*)(b + o_aux);
        // (the gather re-arms K1's shared bounds itself: the sweep in its two halves around it)
        if ((rc = sweep_pair_plan(ctx, tv, gq, 1, 0, &ps)) != FM_OK) return rc;
        hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)(nq_pad / kTileRows)), dim3(256), 0, ctx->stream, d_rows, nq,
                           (const int8_t*)q.rows8, (const int32_t*)q.norm, gq.rows8, gq.norm, gq.aux, d_qbest, ps.bound, (int64_t)ps.ncols_alloc);
        HIP_TRY(ctx, hipGetLastError());
        if ((rc = sweep_pair_run(ctx, tv, gq, 1, nullptr, nullptr, kSweepNoEvents, ps)) != FM_OK) return rc;
    }
    hipLaunchKernelGGL(xcheck_scatter_kernel, dim3((unsigned)((nt * 4 + 255) / 256)), dim3(256), 0, ctx->stream,
                       ps.partial, ps.nsplit, ps.ncols_alloc, nt, d_qbest, 0u, ps.f32_keys, (int*)nullptr, (unsigned*)nullptr);
    HIP_TRY(ctx, hipGetLastError());
    return FM_OK;
}

// ---------------------------------------------------------------------------------------
// K2 entry points
// ---------------------------------------------------------------------------------------
// Device-side knn2 into d_idx/d_dist (device pointers): the top-2 sweep of the pair's route (K2, K8 / K5, K11 on the FP4
// matrix cores -- its keys carry the float32 bits of the integer Hamming distance: exact, no root ties), merged by
// knn2_merge_kernel.  consumer (fm_knn_dev: d_idx / d_dist are the caller's arrays): the stream whose work so far the merge
// -- the first kernel that writes them -- waits for, behind the sweep.
static int knn2_device(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, int32_t* d_idx, float* d_dist, void* consumer = FM_NO_STREAM)
{
    const int64_t nq = q->n;
    if (nq == 0) return FM_OK;
    PairSweep ps{};                                      // (no train rows: no partials, every slot is (-1, +inf))
    ps.f32_keys = q->kind == FM_BANK_F32 || q->kind == FM_BANK_F32W;
    int rc;
    // (output rows whose second best d2 reaches kSqrtTieMin are listed in ps.fix and redone in OpenCV's float32 order)
    if (t->n > 0 && (rc = sweep_pair(ctx, *q, *t, 2, nq, nullptr, nullptr, 0, &ps)) != FM_OK) return rc;
    if ((rc = wait_for_stream(ctx, consumer)) != FM_OK) return rc;
    hipLaunchKernelGGL(knn2_merge_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, ctx->stream,
                       ps.partial, ps.nsplit, ps.ncols_alloc, nq, d_idx, d_dist, ps.f32_keys, ps.fix);
    HIP_TRY(ctx, hipGetLastError());
    if (ps.fix) {
        hipLaunchKernelGGL(sqrt_fix_kernel<2>, dim3(kFixGrid), dim3(256), 0, ctx->stream, (const unsigned*)ps.fix,
                           (const int8_t*)q->rows8, (const int32_t*)q->norm, (const int8_t*)t->rows8, (const int32_t*)t->norm,
                           (int)t->n, (unsigned long long*)nullptr, 0u, d_idx, d_dist, (const unsigned long long*)t->real);
        HIP_TRY(ctx, hipGetLastError());
    }
    return FM_OK;
}

extern "C" int fm_knn2(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, int32_t* idx, float* dist)
{
    int rc = check_pair(ctx, q, t, "fm_knn2", true, true);
    if (rc != FM_OK) return rc;
    const int64_t nq = q->n;
    if (nq > 0 && (!idx || !dist)) return fail(ctx, FM_EINVAL, "fm_knn2: output pointer is NULL");
    if (nq == 0) return FM_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((rc = ws_ensure(ctx, &ctx->ws_out, &ctx->ws_out_bytes, (size_t)nq * 16 + 64)) != FM_OK) return rc;
    int32_t* d_idx = (int32_t*)ctx->ws_out;
    float* d_dist = (float*)((char*)ctx->ws_out + (size_t)nq * 8);
    CallScope cs(ctx);
    if ((rc = knn2_device(ctx, q, t, d_idx, d_dist)) != FM_OK) return rc;
    HIP_TRY(ctx, d2h(ctx, idx, d_idx, (size_t)nq * 8));
    HIP_TRY(ctx, d2h(ctx, dist, d_dist, (size_t)nq * 8));
    return cs.finish();
}

// knnMatch(dt1, dt2, k) for any k the signature of the reference's bf_match / flann_match admits (matchutil.py:39-43, 46-67).
extern "C" int fm_knn(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, int32_t k, int32_t* idx, float* dist)
{
    int rc = check_pair(ctx, q, t, "fm_knn", true, true);
    if (rc != FM_OK) return rc;
    if (k < 1) return fail(ctx, FM_EINVAL, "fm_knn: k must be at least 1");
    if (k > 8) return fail(ctx, FM_EUNSUPPORTED, "fm_knn: k above 8 is not built (cv2.BFMatcher.knnMatch takes any k; the reference calls it with 1 and 2)");
    if (k > 2 && q->kind == FM_BANK_F32W) return refuse_bin(ctx, q, "fm_knn with k >= 3");
    const int64_t nq = q->n;
    if (nq > 0 && (!idx || !dist)) return fail(ctx, FM_EINVAL, "fm_knn: output pointer is NULL");
    if (nq == 0) return FM_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // idx [nq][max(k, 2)] | dist [nq][max(k, 2)] | (k = 1) first columns idx1 [nq], dist1 [nq]
    const size_t out_bytes = (((size_t)nq * (size_t)(k < 2 ? 2 : k) * 4) + 255) & ~(size_t)255;
    const size_t col_bytes = (((size_t)nq * 4) + 255) & ~(size_t)255;
    if ((rc = ws_ensure(ctx, &ctx->ws_out, &ctx->ws_out_bytes, 2 * out_bytes + 2 * col_bytes + 64)) != FM_OK) return rc;
    int32_t* d_idx = (int32_t*)ctx->ws_out;
    float* d_dist = (float*)((char*)ctx->ws_out + out_bytes);
    int32_t* d_idx1 = (int32_t*)((char*)ctx->ws_out + 2 * out_bytes);
    float* d_dist1 = (float*)((char*)ctx->ws_out + 2 * out_bytes + col_bytes);
    CallScope cs(ctx);
    if (k <= 2) {
        // the matrix-core path; k = 1 is the first column of the 2-NN lists
        if ((rc = knn2_device(ctx, q, t, d_idx, d_dist)) != FM_OK) return rc;
        if (k == 2) {
            HIP_TRY(ctx, d2h(ctx, idx, d_idx, (size_t)nq * 8));
            HIP_TRY(ctx, d2h(ctx, dist, d_dist, (size_t)nq * 8));
        } else {
            HIP_TRY(ctx, hipMemcpy2DAsync(d_idx1, 4, d_idx, 8, 4, (size_t)nq, hipMemcpyDeviceToDevice, ctx->stream));
            HIP_TRY(ctx, hipMemcpy2DAsync(d_dist1, 4, d_dist, 8, 4, (size_t)nq, hipMemcpyDeviceToDevice, ctx->stream));
            HIP_TRY(ctx, d2h(ctx, idx, d_idx1, (size_t)nq * 4));
            HIP_TRY(ctx, d2h(ctx, dist, d_dist1, (size_t)nq * 4));
        }
        return cs.finish();
    }
    if ((rc = ws_ensure(ctx, &ctx->ws_partial, &ctx->ws_partial_bytes, knnk_partial_bytes(nq, t->n, k) + 64)) != FM_OK) return rc;
    HIP_TRY(ctx, hipEventRecord(ctx->ev_k0, ctx->stream));
    if (q->kind == FM_BANK_BIN)
        HIP_TRY(ctx, launch_hamming_knnk(*q, *t, k, (unsigned long long*)ctx->ws_partial, d_idx, d_dist, ctx->stream));
    else if (q->kind == FM_BANK_BIN2)
        HIP_TRY(ctx, launch_hamming2_knnk(*q, *t, k, (unsigned long long*)ctx->ws_partial, d_idx, d_dist, ctx->stream));
    else
        HIP_TRY(ctx, launch_knnk(*q, *t, k, (unsigned long long*)ctx->ws_partial, d_idx, d_dist, ctx->stream));
    HIP_TRY(ctx, hipEventRecord(ctx->ev_k1, ctx->stream));
    ctx->kernel_timed = true;
    ctx->pending_pairs += nq * t->n;
    ctx->pending_bytes += bank_bytes(q) + bank_bytes(t);
    HIP_TRY(ctx, d2h(ctx, idx, d_idx, (size_t)nq * k * 4));
    HIP_TRY(ctx, d2h(ctx, dist, d_dist, (size_t)nq * k * 4));
    return cs.finish();
}

// radiusMatch(q, t, maxDistance) (K10, radius.hip): cv2.BFMatcher(NORM_L2).radiusMatch with compactResult = False.
extern "C" int fm_radius_match(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, const float* radius, float radius_all, int64_t cap,
                               int64_t* offsets, int32_t* idx, float* dist, int64_t* n_total)
{
    int rc = check_pair(ctx, q, t, "fm_radius_match");
    if (rc != FM_OK) return rc;
    if (cap < 0) return fail(ctx, FM_EINVAL, "fm_radius_match: cap is negative");
    if (!offsets) return fail(ctx, FM_EINVAL, "fm_radius_match: offsets is NULL");
    if (cap > 0 && (!idx || !dist)) return fail(ctx, FM_EINVAL, "fm_radius_match: idx / dist is NULL with cap > 0");
    if (q->n > 0 && t->n > 0 && q->kind != t->kind) return fail(ctx, FM_EINVAL, "fm_radius_match: query/train kind mismatch");
    const RadiusArgs a{"fm_radius_match", radius, radius_all, cap, offsets, nullptr, idx, dist, n_total, false, FM_NO_STREAM, nullptr, 0};
    return radius_match(ctx, *q, *t, a);
}

// fm_radius_match with the radii read from, and the offsets and lists written to, the caller's device memory (radius.hip).
extern "C" int fm_radius_match_dev(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, const float* d_radius, float radius_all, int64_t cap,
                                   int64_t* d_offsets, int32_t* d_idx, float* d_dist, int64_t* n_total, void* consumer_stream)
{
    const char* who = "fm_radius_match_dev";
    int rc = check_pair(ctx, q, t, who);
    if (rc != FM_OK) return rc;
    if (cap < 0) return fail(ctx, FM_EINVAL, "fm_radius_match_dev: cap is negative");
    if (!d_offsets) return fail(ctx, FM_EINVAL, "fm_radius_match_dev: d_offsets is NULL");
    if (cap > 0 && (!d_idx || !d_dist)) return fail(ctx, FM_EINVAL, "fm_radius_match_dev: d_idx / d_dist is NULL with cap > 0");
    if (q->n > 0 && t->n > 0 && q->kind != t->kind) return fail(ctx, FM_EINVAL, "fm_radius_match_dev: query/train kind mismatch");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (d_radius && (rc = check_device_ptr(ctx, d_radius, who, "d_radius")) != FM_OK) return rc;
    if ((rc = check_device_ptr(ctx, d_offsets, who, "d_offsets")) != FM_OK) return rc;
    if (d_idx && (rc = check_device_ptr(ctx, d_idx, who, "d_idx")) != FM_OK) return rc;
    if (d_dist && (rc = check_device_ptr(ctx, d_dist, who, "d_dist")) != FM_OK) return rc;
    const RadiusArgs a{who, d_radius, radius_all, cap, d_offsets, nullptr, d_idx, d_dist, n_total, true, consumer_stream, nullptr, 0};
    return radius_match(ctx, *q, *t, a);
}

// Hamming radiusMatch (radius.hip, the Hamming route): fm_radius_match's contract with dist = (float)popcount(q XOR t) on two
// binary banks.  The L2-named calls above keep refusing binary banks; these are the entry points that serve them.
static int ham_radius_check(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, int64_t cap, const void* offsets, const void* idx, const void* dist,
                            const char* who, const char* pre)
{
    int rc = check_pair(ctx, q, t, who, true, true);
    if (rc != FM_OK) return rc;
    // (a NORM_HAMMING2 pair -- check_pair has refused one such bank beside any other kind -- takes the radius against h2)
    if (!(q->kind == FM_BANK_BIN2 && t->kind == FM_BANK_BIN2) && (q->kind != FM_BANK_BIN || t->kind != FM_BANK_BIN))
        return fail(ctx, FM_EINVAL, std::string(who) + ": both banks must be binary (FM_BANK_BIN, fm_bank_create_bin); fm_radius_match is the L2 call");
    if (q->dim != t->dim) return fail(ctx, FM_EINVAL, std::string(who) + ": query/train width mismatch");       // (check_pair's, restated)
    if (cap < 0) return fail(ctx, FM_EINVAL, std::string(who) + ": cap is negative");
    if (!offsets) return fail(ctx, FM_EINVAL, std::string(who) + ": " + pre + "offsets is NULL");
    if (cap > 0 && (!idx || !dist)) return fail(ctx, FM_EINVAL, std::string(who) + ": " + pre + "idx / " + pre + "dist is NULL with cap > 0");
    return FM_OK;
}

extern "C" int fm_hamming_radius_match(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, const float* radius, float radius_all, int64_t cap,
                                       int64_t* offsets, int32_t* idx, float* dist, int64_t* n_total)
{
    const char* who = "fm_hamming_radius_match";
    int rc = ham_radius_check(ctx, q, t, cap, offsets, idx, dist, who, "");
    if (rc != FM_OK) return rc;
    const RadiusArgs a{who, radius, radius_all, cap, offsets, nullptr, idx, dist, n_total, false, FM_NO_STREAM, nullptr, 0};
    return radius_match(ctx, *q, *t, a);
}

extern "C" int fm_hamming_radius_match_dev(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, const float* d_radius, float radius_all,
                                           int64_t cap, int64_t* d_offsets, int32_t* d_idx, float* d_dist, int64_t* n_total,
                                           void* consumer_stream)
{
    const char* who = "fm_hamming_radius_match_dev";
    int rc = ham_radius_check(ctx, q, t, cap, d_offsets, d_idx, d_dist, who, "d_");
    if (rc != FM_OK) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (d_radius && (rc = check_device_ptr(ctx, d_radius, who, "d_radius")) != FM_OK) return rc;
    if ((rc = check_device_ptr(ctx, d_offsets, who, "d_offsets")) != FM_OK) return rc;
    if (d_idx && (rc = check_device_ptr(ctx, d_idx, who, "d_idx")) != FM_OK) return rc;
    if (d_dist && (rc = check_device_ptr(ctx, d_dist, who, "d_dist")) != FM_OK) return rc;
    const RadiusArgs a{who, d_radius, radius_all, cap, d_offsets, nullptr, d_idx, d_dist, n_total, true, consumer_stream, nullptr, 0};
    return radius_match(ctx, *q, *t, a);
}

// Wide radiusMatch (radius.hip, the wide route): fm_radius_match's contract with K14's distance on two wide float banks.  The
// L2-named calls above keep refusing wide banks; these are the entry points that serve them.  Checks in the header's order:
// handles, the kinds (even of an empty bank), the dims, cap and the output pointers.
static int wide_radius_check(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, int64_t cap, const void* offsets, const void* idx, const void* dist,
                             const char* who, const char* pre)
{
    if (!ctx) return fail(nullptr, FM_EINVAL, std::string(who) + ": ctx is NULL");
    if (!q || !t) return fail(ctx, FM_EINVAL, std::string(who) + ": bank is NULL");
    for (const fm_bank* b : {q, t})
        if (int rc = refuse_bin2(ctx, b, who)) return rc;
    for (const fm_bank* b : {q, t})
        if (b->kind != FM_BANK_F32W)
            return fail(ctx, FM_EINVAL, std::string(who) + ": both banks must be wide float (FM_BANK_F32W: fm_bank_create_f32 with 129 .. 256 "
                                        "values per row); " + (b->kind == FM_BANK_BIN ? "fm_hamming_radius_match is the Hamming call"
                                                                                      : "fm_radius_match is the L2 call"));
    if (q->dim != t->dim) return fail(ctx, FM_EINVAL, std::string(who) + ": query/train dim mismatch");
    if (cap < 0) return fail(ctx, FM_EINVAL, std::string(who) + ": cap is negative");
    if (!offsets) return fail(ctx, FM_EINVAL, std::string(who) + ": " + pre + "offsets is NULL");
    if (cap > 0 && (!idx || !dist)) return fail(ctx, FM_EINVAL, std::string(who) + ": " + pre + "idx / " + pre + "dist is NULL with cap > 0");
    return FM_OK;
}

extern "C" int fm_wide_radius_match(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, const float* radius, float radius_all, int64_t cap,
                                    int64_t* offsets, int32_t* idx, float* dist, int64_t* n_total)
{
    const char* who = "fm_wide_radius_match";
    int rc = wide_radius_check(ctx, q, t, cap, offsets, idx, dist, who, "");
    if (rc != FM_OK) return rc;
    const RadiusArgs a{who, radius, radius_all, cap, offsets, nullptr, idx, dist, n_total, false, FM_NO_STREAM, nullptr, 0};
    return radius_match(ctx, *q, *t, a);
}

extern "C" int fm_wide_radius_match_dev(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, const float* d_radius, float radius_all,
                                        int64_t cap, int64_t* d_offsets, int32_t* d_idx, float* d_dist, int64_t* n_total,
                                        void* consumer_stream)
{
    const char* who = "fm_wide_radius_match_dev";
    int rc = wide_radius_check(ctx, q, t, cap, d_offsets, d_idx, d_dist, who, "d_");
    if (rc != FM_OK) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (d_radius && (rc = check_device_ptr(ctx, d_radius, who, "d_radius")) != FM_OK) return rc;
    if ((rc = check_device_ptr(ctx, d_offsets, who, "d_offsets")) != FM_OK) return rc;
    if (d_idx && (rc = check_device_ptr(ctx, d_idx, who, "d_idx")) != FM_OK) return rc;
    if (d_dist && (rc = check_device_ptr(ctx, d_dist, who, "d_dist")) != FM_OK) return rc;
    const RadiusArgs a{who, d_radius, radius_all, cap, d_offsets, nullptr, d_idx, d_dist, n_total, true, consumer_stream, nullptr, 0};
    return radius_match(ctx, *q, *t, a);
}

// Masked radiusMatch on a bank pair (radius.hip: the masked instantiations of the four sweeps).  One name for every kind of
// pair -- integer, float32 route, binary (fm_hamming_radius_match's distance and radius rules), wide float
// (fm_wide_radius_match's) -- chosen by the banks' kind as radius_match chooses its route.  Checks in the header's order:
// handles, the pair (check_pair, which takes a binary or a wide pair here), the mask, cap and the outputs.
static int radius_masked_check(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, const fm_mask* m, int64_t cap, const void* offsets,
                               const void* idx, const void* dist, const char* who, const char* pre)
{
    if (!ctx) return fail(nullptr, FM_EINVAL, std::string(who) + ": ctx is NULL");
    if (!q || !t) return fail(ctx, FM_EINVAL, std::string(who) + ": bank is NULL");
    if (!m) return fail(ctx, FM_EINVAL, std::string(who) + ": mask is NULL");
    int rc = check_pair(ctx, q, t, who, true);
    if (rc != FM_OK) return rc;
    if ((rc = mask_check(ctx, m, who)) != FM_OK) return rc;
    if (m->coll) return fail(ctx, FM_EINVAL, std::string(who) + ": the mask was made for a collection (fm_mask_create_coll); a bank pair takes fm_mask_create's");
    if (m->nq != q->n)
        return fail(ctx, FM_EINVAL, std::string(who) + ": the mask has " + std::to_string(m->nq) + " query rows, the query bank " + std::to_string(q->n));
    if (m->nt != t->n)
        return fail(ctx, FM_EINVAL, std::string(who) + ": the mask has " + std::to_string(m->nt) + " train rows, the train bank " + std::to_string(t->n));
    if (cap < 0) return fail(ctx, FM_EINVAL, std::string(who) + ": cap is negative");
    if (!offsets) return fail(ctx, FM_EINVAL, std::string(who) + ": " + pre + "offsets is NULL");
    if (cap > 0 && (!idx || !dist)) return fail(ctx, FM_EINVAL, std::string(who) + ": " + pre + "idx / " + pre + "dist is NULL with cap > 0");
    return FM_OK;
}

extern "C" int fm_radius_match_masked(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, const fm_mask* mask, const float* radius,
                                      float radius_all, int64_t cap, int64_t* offsets, int32_t* idx, float* dist, int64_t* n_total)
{
    const char* who = "fm_radius_match_masked";
    int rc = radius_masked_check(ctx, q, t, mask, cap, offsets, idx, dist, who, "");
    if (rc != FM_OK) return rc;
    const RadiusArgs a{who, radius, radius_all, cap, offsets, nullptr, idx, dist, n_total, false, FM_NO_STREAM, nullptr, 0, mask->bits, mask->words};
    return radius_match(ctx, *q, *t, a);
}

extern "C" int fm_radius_match_masked_dev(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, const fm_mask* mask, const float* d_radius,
                                          float radius_all, int64_t cap, int64_t* d_offsets, int32_t* d_idx, float* d_dist,
                                          int64_t* n_total, void* consumer_stream)
{
    const char* who = "fm_radius_match_masked_dev";
    int rc = radius_masked_check(ctx, q, t, mask, cap, d_offsets, d_idx, d_dist, who, "d_");
    if (rc != FM_OK) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (d_radius && (rc = check_device_ptr(ctx, d_radius, who, "d_radius")) != FM_OK) return rc;
    if ((rc = check_device_ptr(ctx, d_offsets, who, "d_offsets")) != FM_OK) return rc;
    if (d_idx && (rc = check_device_ptr(ctx, d_idx, who, "d_idx")) != FM_OK) return rc;
    if (d_dist && (rc = check_device_ptr(ctx, d_dist, who, "d_dist")) != FM_OK) return rc;
    const RadiusArgs a{who, d_radius, radius_all, cap, d_offsets, nullptr, d_idx, d_dist, n_total, true, consumer_stream, nullptr, 0,
                       mask->bits, mask->words};
    return radius_match(ctx, *q, *t, a);
}

// Classic Ratio-Match up to the compaction, in ws_out: 2-NN lists | per-q tidx, dist, ratio, pass | block counts, count word |
// `extra` bytes of the caller's own (16-byte aligned, at `rest`).  knn2_device, then lowe_kernel.
struct LoweWs {
    int32_t* tidx; float* dist; double* ratio; uint8_t* pass; int* bc;
    unsigned long long* cnt;
    char* rest;
    int nblk;
};

static int knn2_lowe_device(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, double tau, size_t extra, LoweWs* w)
{
    const int64_t nq = q->n;
    w->nblk = (int)((nq + 255) / 256);
    size_t off = 0;
    const size_t o_i2 = carve(off, (size_t)nq * 8, 16), o_d2 = carve(off, (size_t)nq * 8, 16), o_ti = carve(off, (size_t)nq * 4, 16), o_di = carve(off, (size_t)nq * 4, 16);
    const size_t o_ra = carve(off, (size_t)nq * 8, 16), o_pa = carve(off, (size_t)nq, 16), o_bc = carve(off, (size_t)w->nblk * 4, 16), o_cnt = carve(off, 16, 16);
    int rc;
    if ((rc = ws_ensure(ctx, &ctx->ws_out, &ctx->ws_out_bytes, off + extra + 64)) != FM_OK) return rc;
    char* b = (char*)ctx->ws_out;
    w->tidx = (int32_t*)(b + o_ti); w->dist = (float*)(b + o_di); w->ratio = (double*)(b + o_ra); w->pass = (uint8_t*)(b + o_pa);
    w->bc = (int*)(b + o_bc); w->cnt = (unsigned long long*)(b + o_cnt); w->rest = b + off;
    if ((rc = knn2_device(ctx, q, t, (int32_t*)(b + o_i2), (float*)(b + o_d2))) != FM_OK) return rc;
    hipLaunchKernelGGL(lowe_kernel, dim3((unsigned)w->nblk), dim3(256), 0, ctx->stream, (const int32_t*)(b + o_i2),
                       (const float*)(b + o_d2), nq, tau, w->tidx, w->dist, w->ratio, w->pass, w->bc);
    HIP_TRY(ctx, hipGetLastError());
    return FM_OK;
}

extern "C" int fm_knn2_ratio(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, double tau, int64_t cap,
                             int32_t* qidx, int32_t* tidx, float* dist, double* ratio, int64_t* n_accepted)
{
    int rc = check_pair(ctx, q, t, "fm_knn2_ratio", true, true);
    if (rc != FM_OK) return rc;
    if (n_accepted) *n_accepted = 0;
    const int64_t nq = q->n;
    if (nq == 0) return FM_OK;
    if (cap < 0 || !qidx || !tidx || !dist || !ratio) return fail(ctx, FM_EINVAL, "fm_knn2_ratio: bad output arguments");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int64_t ccap = cap < nq ? cap : nq;
    size_t off = 0;         // the compacted outputs
    const size_t o_cq = carve(off, (size_t)ccap * 4, 16), o_ct = carve(off, (size_t)ccap * 4, 16), o_cd = carve(off, (size_t)ccap * 4, 16), o_cr = carve(off, (size_t)ccap * 8, 16);
    CallScope cs(ctx);
    LoweWs w;
    if ((rc = knn2_lowe_device(ctx, q, t, tau, off, &w)) != FM_OK) return rc;
    char* b = w.rest;
    hipLaunchKernelGGL(compact_kernel, dim3((unsigned)w.nblk), dim3(256), 0, ctx->stream, (const int32_t*)w.tidx, (const float*)w.dist,
                       (const double*)w.ratio, (const uint8_t*)w.pass, (const int*)w.bc, nq, ccap, (int32_t*)(b + o_cq),
                       (int32_t*)(b + o_ct), (float*)(b + o_cd), (double*)(b + o_cr), w.cnt);
    HIP_TRY(ctx, hipGetLastError());
    return cs.finish_rows(w.cnt, ccap, {{qidx, b + o_cq, 4}, {tidx, b + o_ct, 4}, {dist, b + o_cd, 4}, {ratio, b + o_cr, 8}}, n_accepted);
}

static int take_timer(fm_ctx* ctx, fm_ctx::PendingTimer* tm);

// Self distances of n banks on the context's stream, each into d_out[i] (device, [banks[i]->n] float64).
// Integer-valued banks: the triangular sweep (launch_rowreduce_tri: from 32768 padded rows on, and for every run of two or
// more integer banks, of any sizes, up to "batch_group" banks per launch pair) or the masked-diagonal top-1 sweep (K1's top-1
// kernel; launch_rowreduce_self; consecutive banks of one padded size through ONE launch of rowreduce_batch_kernel);
// float32 banks: the float32 route with the diagonal masked (K8 filter + exact rescoring, or K5), one by one.
// Banks with non-finite values keep the literal form (2-NN, second column).  Enqueue only; the split partials
// live in ws_partial, which every user touches on ctx->stream only.  timed: record ev_k0 / ev_k1 around the
// (last) distance-kernel launch.
static int selfdist_device(fm_ctx* ctx, int n, const fm_bank* const* banks, double* const* d_out, bool timed)
{
    const int group_max = ctx->tune.batch_group;
    int i = 0;
    while (i < n) {
        const fm_bank* b = banks[i];
        if (b->n == 0) { ++i; continue; }
        int rc;
        if (b->kind == FM_BANK_F32) {
            SelfMerge m{};
            RowReducePlan pl;
            if (!b->filt_ok) {
                // non-finite values: no shortcut is claimed for them
                if ((rc = ws_ensure(ctx, &ctx->ws_out, &ctx->ws_out_bytes, (size_t)b->n * 16 + 64)) != FM_OK) return rc;
                int32_t* d_idx = (int32_t*)ctx->ws_out;
                float* d_dist = (float*)((char*)ctx->ws_out + (size_t)b->n * 8);
                if ((rc = knn2_device(ctx, b, b, d_idx, d_dist)) != FM_OK) return rc;
                hipLaunchKernelGGL(selfdist_from_knn_kernel, dim3((unsigned)((b->n + 255) / 256)), dim3(256), 0, ctx->stream,
                                   (const float*)d_dist, b->n, d_out[i]);
                HIP_TRY(ctx, hipGetLastError());
                ++i;
                continue;
            }
            // r06: every distance once -- the triangular sweep around the fp16 filter (filter_f16.hip, TRI) from 65536 padded
            // rows on ("self_tri" 1; 2 = always, 0 = never), else the masked full sweep through the filter / K5.  (Measured,
            // profiles/r06e_f32_selfdist_tri.log: x 1.00 of the masked sweep's time at 50k rows, 0.94 at 65k, 0.83 at 100k,
            // 0.76 at 200k -- below ~60k rows the sweep has fewer pieces than the chip holds workgroups, every row's visits
            // happen at once against a stale bound, and the lists overflow into rescans.)
            const bool tri = ctx->tune.f32_filter != 0 && ctx->tune.self_tri != 0 && b->n_pad <= kTriMaxRows &&
                             (ctx->tune.self_tri == 2 || b->n_pad >= 65536) && filter_usable(*b, *b);
            if (tri) {
                pl = plan_rowreduce_f32(b->n_pad, b->n_pad, ctx->tune.nsplit);
                TriPlan tp;
                if ((rc = tri_plan_for(ctx, b->n_pad, &tp)) != FM_OK) return rc;
                const size_t part = (pl.partial_bytes(1) + 255) & ~(size_t)255;
                const size_t bnd = ((size_t)tp.ncols_alloc * 4 + 255) & ~(size_t)255;
                if ((rc = ws_ensure(ctx, &ctx->ws_partial, &ctx->ws_partial_bytes, part + bnd + filter_tri_bytes(tp.ncols_alloc) + 64)) != FM_OK) return rc;
                unsigned long long* d_part = (unsigned long long*)ctx->ws_partial;
                int* d_bound = (int*)((char*)ctx->ws_partial + part);
                void* d_tri = (char*)d_bound + bnd;
                HIP_TRY(ctx, hipMemsetAsync(d_part, 0xff, pl.partial_bytes(1), ctx->stream));
                HIP_TRY(ctx, hipMemsetD32Async((hipDeviceptr_t)d_bound, filter_empty_bound(), (size_t)tp.ncols_alloc, ctx->stream));
                HIP_TRY(ctx, hipMemsetAsync(ctx->d_counters, 0, 8, ctx->stream));
                HIP_TRY(ctx, hipEventRecord(ctx->ev_k0, ctx->stream));
                HIP_TRY(ctx, launch_filter_tri(*b, tp, ctx->tune.f32_bound_every, d_tri, d_bound, ctx->d_counters, d_part, ctx->stream));
                HIP_TRY(ctx, launch_rowreduce_f32(*b, *b, 1, pl, d_part, ctx->d_counters, ctx->stream, true));
                HIP_TRY(ctx, hipEventRecord(ctx->ev_k1, ctx->stream));
                ctx->filter_launches += 1;
            } else if ((rc = rowreduce_f32_route(ctx, b, b, 1, &pl, true)) != FM_OK) return rc;
            ctx->kernel_timed = true;
            ctx->pending_pairs += b->n * b->n;
            ctx->pending_bytes += bank_bytes(b);
            m.partial[0] = (const unsigned long long*)ctx->ws_partial;
            m.out[0] = d_out[i];
            hipLaunchKernelGGL(selfdist_merge_kernel, dim3((unsigned)((b->n + 255) / 256), 1), dim3(256), 0, ctx->stream,
                               m, pl.nsplit, pl.ncols_alloc, b->n, 1);
            HIP_TRY(ctx, hipGetLastError());
            ++i;
            continue;
        }
        // Every distance once: the triangular sweep, up to "batch_group" banks per launch, every bank under the plan of its
        // own size.  Rule ("self_tri" 1): a bank of 32768 padded rows or more, or ANY run of two or more integer banks -- a
        // dataset of small images (r05, last: 64 banks of ~12.5k rows took 65 us each one by one through the full sweep and
        // take 23 us each in batched triangular launches; ~3k rows: 35 -> 9.5 us).
        int g = 1;
        const bool tri_fits = b->n_pad <= kTriMaxRows;
        if (ctx->tune.glds != 0 && ctx->tune.self_tri != 0 && tri_fits)
            while (i + g < n && g < group_max && g < kRRBatchMax && banks[i + g]->kind == FM_BANK_I8 && banks[i + g]->n > 0 &&
                   banks[i + g]->n_pad <= kTriMaxRows) ++g;
        if (ctx->tune.glds != 0 && tri_fits && (ctx->tune.self_tri == 2 || (ctx->tune.self_tri == 1 && (b->n_pad >= 32768 || g >= 2)))) {
            TriPlan tps[kRRBatchMax];
            size_t boff[kRRBatchMax + 1];
            boff[0] = 0;
            for (int j = 0; j < g; ++j) {
                if ((rc = tri_plan_for(ctx, banks[i + j]->n_pad, &tps[j])) != FM_OK) return rc;
                boff[j + 1] = boff[j] + (((size_t)tps[j].ncols_alloc * 4 + 255) & ~(size_t)255);
            }
            if ((rc = ws_ensure(ctx, &ctx->ws_partial, &ctx->ws_partial_bytes, boff[g])) != FM_OK) return rc;
            const Bank* bk[kRRBatchMax];
            int* bnd[kRRBatchMax];
            TriFinish fin{};
            int64_t nmax = 0;
            for (int j = 0; j < g; ++j) {
                bk[j] = banks[i + j];
                bnd[j] = (int*)((char*)ctx->ws_partial + boff[j]);
                fin.bound[j] = bnd[j]; fin.norm[j] = bk[j]->norm; fin.out[j] = d_out[i + j]; fin.n[j] = bk[j]->n;
                nmax = bk[j]->n > nmax ? bk[j]->n : nmax;
                // (each distance is computed once; the pairs a caller asked for are still n x n)
                ctx->pending_pairs += bk[j]->n * bk[j]->n;
                ctx->pending_bytes += bank_bytes(bk[j]);
            }
            HIP_TRY(ctx, hipMemsetD32Async((hipDeviceptr_t)bnd[0], (int)0x80000000, boff[g] / 4, ctx->stream));
            if (timed) HIP_TRY(ctx, hipEventRecord(ctx->ev_k0, ctx->stream));
            HIP_TRY(ctx, launch_rowreduce_tri(g, bk, tps, bnd, ctx->tune.prio != 0, ctx->stream));
            if (timed) HIP_TRY(ctx, hipEventRecord(ctx->ev_k1, ctx->stream));
            ctx->kernel_timed = timed;
            hipLaunchKernelGGL(selfdist_tri_finish_kernel, dim3((unsigned)((nmax + 255) / 256), (unsigned)g), dim3(256), 0, ctx->stream, fin);
            HIP_TRY(ctx, hipGetLastError());
            i += g;
            continue;
        }
        const RowReducePlan pl = plan_rowreduce_self(b->n_pad, ctx->tune);
        g = 1;
        if (pl.nw == 8 && (ctx->tune.glds != 0) && pl.nbuf != 2)
            while (i + g < n && g < group_max && banks[i + g]->kind == FM_BANK_I8 && banks[i + g]->n > 0 && banks[i + g]->n_pad == b->n_pad) ++g;
        const bool coop = (ctx->tune.coop != 0) && pl.nsplit > 1;
        const size_t pbytes = (pl.partial_bytes(1) + 255) & ~(size_t)255, bbytes = ((size_t)pl.ncols_alloc * 4 + 255) & ~(size_t)255;
        if ((rc = ws_ensure(ctx, &ctx->ws_partial, &ctx->ws_partial_bytes, (size_t)g * (pbytes + bbytes))) != FM_OK) return rc;
        SelfMerge m{};
        const Bank* bk[kRRBatchMax];
        unsigned long long* part[kRRBatchMax];
        int* bnd[kRRBatchMax];
        int64_t nmax = 0;
        for (int j = 0; j < g; ++j) {
            bk[j] = banks[i + j];
            // (partials first, then the g bound arrays back to back: one fill re-arms them all)
            part[j] = (unsigned long long*)((char*)ctx->ws_partial + (size_t)j * pbytes);
            bnd[j] = coop ? (int*)((char*)ctx->ws_partial + (size_t)g * pbytes + (size_t)j * bbytes) : nullptr;
            m.partial[j] = part[j];
            m.out[j] = d_out[i + j];
            nmax = bk[j]->n > nmax ? bk[j]->n : nmax;
            ctx->pending_pairs += bk[j]->n * bk[j]->n;
            ctx->pending_bytes += bank_bytes(bk[j]);
        }
        if (coop && !ablate_keep_bounds())
            HIP_TRY(ctx, hipMemsetD32Async((hipDeviceptr_t)bnd[0], (int)0x80000000, (size_t)g * (bbytes / 4), ctx->stream));
        if (timed) HIP_TRY(ctx, hipEventRecord(ctx->ev_k0, ctx->stream));
        if (g > 1) {
            RowReducePlan pls[kRRBatchMax];
            for (int j = 0; j < g; ++j) pls[j] = pl;
            HIP_TRY(ctx, launch_rowreduce_batch(g, bk, bk, pls, part, bnd, ctx->stream, true));
        }
        else       HIP_TRY(ctx, launch_rowreduce_self(*bk[0], pl, part[0], bnd[0], (ctx->tune.glds != 0), ctx->stream));
        if (timed) HIP_TRY(ctx, hipEventRecord(ctx->ev_k1, ctx->stream));
        ctx->kernel_timed = timed;
        // (banks of one padded size may hold different row counts: the merge covers the largest, rows beyond a
        // bank's own n are never written -- its out[] has n entries -- see the guard below)
        for (int j = 0; j < g; ++j) {
            SelfMerge one{};
            one.partial[0] = m.partial[j]; one.out[0] = m.out[j];
            if (bk[j]->n != nmax) {
                hipLaunchKernelGGL(selfdist_merge_kernel, dim3((unsigned)((bk[j]->n + 255) / 256), 1), dim3(256), 0, ctx->stream,
                                   one, pl.nsplit, pl.ncols_alloc, bk[j]->n, 0);
                m.partial[j] = nullptr;
            }
        }
        // the banks that share nmax go through one launch
        SelfMerge same{};
        int ns = 0;
        for (int j = 0; j < g; ++j) if (m.partial[j]) { same.partial[ns] = m.partial[j]; same.out[ns] = m.out[j]; ++ns; }
        if (ns > 0)
            hipLaunchKernelGGL(selfdist_merge_kernel, dim3((unsigned)((nmax + 255) / 256), (unsigned)ns), dim3(256), 0, ctx->stream,
                               same, pl.nsplit, pl.ncols_alloc, nmax, 0);
        HIP_TRY(ctx, hipGetLastError());
        i += g;
    }
    return FM_OK;
}

extern "C" int fm_self_dist(fm_ctx* ctx, const fm_bank* bank, double* selfdist)
{
    int rc = check_pair(ctx, bank, bank, "fm_self_dist");
    if (rc != FM_OK) return rc;
    const int64_t n = bank->n;
    if (n == 0) return FM_OK;
    if (!selfdist) return fail(ctx, FM_EINVAL, "fm_self_dist: output pointer is NULL");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // (ws_in: ws_out is the 2-NN scratch of the non-finite float32 case)
    if ((rc = ws_ensure(ctx, &ctx->ws_in, &ctx->ws_in_bytes, (size_t)n * 8 + 64)) != FM_OK) return rc;
    double* d_sd = (double*)ctx->ws_in;
    CallScope cs(ctx);
    if ((rc = selfdist_device(ctx, 1, &bank, &d_sd, true)) != FM_OK) return rc;
    HIP_TRY(ctx, d2h(ctx, selfdist, d_sd, (size_t)n * 8));
    return cs.finish();
}

extern "C" int fm_self_dist_batch(fm_ctx* ctx, int32_t n, fm_bank* const* banks, double* const* out)
{
    if (!ctx) return fail(nullptr, FM_EINVAL, "fm_self_dist_batch: ctx is NULL");
    if (n < 0) return fail(ctx, FM_EINVAL, "fm_self_dist_batch: n < 0");
    if (n == 0) return FM_OK;
    if (!banks) return fail(ctx, FM_EINVAL, "fm_self_dist_batch: banks is NULL");
    for (int i = 0; i < n; ++i) {
        if (!banks[i]) return fail(ctx, FM_EINVAL, "fm_self_dist_batch: bank is NULL");
        if (int rc = refuse_bin(ctx, banks[i], "fm_self_dist_batch")) return rc;
        for (int j = 0; j < i; ++j) if (banks[j] == banks[i]) return fail(ctx, FM_EINVAL, "fm_self_dist_batch: a bank is listed twice");
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::vector<double*> d_out((size_t)n, nullptr);
    std::vector<const fm_bank*> cb((size_t)n, nullptr);
    bool any_out = false;
    int rc;
    for (int i = 0; i < n; ++i) {
        fm_bank* b = banks[i];
        // (the first attachment allocates; a refilled bank keeps its array: fm_bank_refill_u8_async keeps the capacity)
        if ((rc = bank_selfdist_alloc(ctx, b)) != FM_OK) return rc;
        b->sdmax_rows = -1;           // (until the largest of the new values is known: no ratio cut)
        d_out[(size_t)i] = b->selfdist;
        cb[(size_t)i] = b;
        any_out = any_out || (out && out[i] && b->n > 0);
    }
    // the largest self distance of every bank, behind the sweeps on the same stream
    auto reduce_max = [&]() {
        for (int i = 0; i < n; ++i) if (int e = enqueue_selfdist_max(ctx, banks[i], ctx->stream)) return e;
        return (int)FM_OK;
    };
    if (!any_out) {
        // enqueue only: accounted at the next fm_sync like the other asynchronous calls
        fm_ctx::PendingTimer tm;
        if ((rc = take_timer(ctx, &tm)) != FM_OK) return rc;
        const int64_t before = ctx->pending_pairs, before_b = ctx->pending_bytes;
        ctx->pending_pairs = 0;
        ctx->pending_bytes = 0;
        HIP_TRY(ctx, hipEventRecord(tm.k0, ctx->stream));
        rc = selfdist_device(ctx, n, cb.data(), d_out.data(), false);
        HIP_TRY(ctx, hipEventRecord(tm.k1, ctx->stream));
        if (rc == FM_OK) rc = reduce_max();
        HIP_TRY(ctx, hipEventRecord(tm.c1, ctx->stream));
        tm.timed = rc == FM_OK && ctx->pending_pairs > 0;
        tm.call_timed = true;
        tm.pairs = ctx->pending_pairs;
        tm.bytes = ctx->pending_bytes;
        ctx->pending_pairs = before;
        ctx->pending_bytes = before_b;
        ctx->pending.push_back(tm);
        return rc;
    }
    CallScope cs(ctx);
    if ((rc = selfdist_device(ctx, n, cb.data(), d_out.data(), true)) != FM_OK) return rc;
    if ((rc = reduce_max()) != FM_OK) return rc;
    for (int i = 0; i < n; ++i)
        if (out[i] && banks[i]->n > 0) HIP_TRY(ctx, d2h(ctx, out[i], d_out[(size_t)i], (size_t)banks[i]->n * 8));
    return cs.finish();
}

// ---------------------------------------------------------------------------------------
// Hamming self distances (hamming.hip: ham_self_kernel, ham_self_merge_kernel)
// ---------------------------------------------------------------------------------------
// Self distances of n binary banks on the context's stream, each into d_out[i] (device, [banks[i]->n] float64).  Runs of
// consecutive non-empty banks of one ksteps go through ONE sweep launch and one merge launch, up to "batch_group" banks
// (at most kHamSelfMax); every bank under plan_hamming of its own size.  The workgroup tables of all launches are built first
// and uploaded once (the context's page-locked table buffer), behind the partials in ws_partial, which the launches of the
// call reuse in stream order.  Enqueue only.  timed: ev_k0 / ev_k1 around the (last) sweep launch.
static int ham_selfdist_device(fm_ctx* ctx, int n, const fm_bank* const* banks, double* const* d_out, bool timed)
{
    struct Group { int first, count, wg0, wgs; };
    std::vector<Group> groups;
    std::vector<HamPlan> plans((size_t)n);
    const int group_max = std::max(1, std::min(ctx->tune.batch_group, kHamSelfMax));
    size_t max_part = 0;
    int64_t total_wg = 0;
    for (int i = 0; i < n;) {
        if (banks[i]->n == 0) { ++i; continue; }
        Group g{i, 0, (int)total_wg, 0};
        size_t part = 0;
        while (i < n && g.count < group_max && banks[i]->n > 0 && banks[i]->ksteps == banks[g.first]->ksteps) {
            const HamPlan p = plan_hamming(banks[i]->n_pad, banks[i]->n_pad);
            plans[(size_t)i] = p;
            part += (p.partial_bytes(1) + 255) & ~(size_t)255;
            g.wgs += p.nchunks * p.nsplit;
            ++g.count; ++i;
        }
        total_wg += g.wgs;
        max_part = std::max(max_part, part);
        groups.push_back(g);
    }
    if (groups.empty()) return FM_OK;
    if (total_wg > (int64_t)1 << 26) return fail(ctx, FM_EUNSUPPORTED, "fm_hamming_self_dist: more than 2^26 workgroups in one call");
    const size_t tab_bytes = (size_t)total_wg * 16;
    int rc;
    if ((rc = ws_ensure(ctx, &ctx->ws_partial, &ctx->ws_partial_bytes, max_part + tab_bytes + 64)) != FM_OK) return rc;
    if ((rc = table_host(ctx, tab_bytes)) != FM_OK) return rc;
    int* tab = (int*)ctx->h_tab;
    char* d_tab = (char*)ctx->ws_partial + max_part;
    for (const Group& g : groups) {
        int* e = tab + (size_t)g.wg0 * 4;
        for (int j = 0; j < g.count; ++j) {
            const HamPlan& p = plans[(size_t)(g.first + j)];
            // (a bank's workgroups in launch_hamming's order: the chunks of a split side by side)
            for (int s = 0; s < p.nsplit; ++s)
                for (int c = 0; c < p.nchunks; ++c) { e[0] = j; e[1] = c; e[2] = s; e[3] = 0; e += 4; }
        }
    }
    if ((rc = table_upload(ctx, d_tab, tab_bytes)) != FM_OK) return rc;
    for (const Group& g : groups) {
        HamSelfArgs a{};
        size_t at = 0;
        for (int j = 0; j < g.count; ++j) {
            const fm_bank* b = banks[g.first + j];
            HamSelfBank& s = a.b[j];
            s.rows4 = b->rows4;
            s.partial = (unsigned long long*)((char*)ctx->ws_partial + at);
            s.out = d_out[g.first + j];
            s.n = (int)b->n;
            s.W = 8 * b->dim;
            s.plan = plans[(size_t)(g.first + j)];
            at += (s.plan.partial_bytes(1) + 255) & ~(size_t)255;
            ctx->pending_pairs += b->n * b->n;
            ctx->pending_bytes += bank_bytes(b);
        }
        if (timed) HIP_TRY(ctx, hipEventRecord(ctx->ev_k0, ctx->stream));
        HIP_TRY(ctx, launch_hamming_self(a, g.count, banks[g.first]->ksteps, d_tab + (size_t)g.wg0 * 16, g.wgs, ctx->stream));
        if (timed) HIP_TRY(ctx, hipEventRecord(ctx->ev_k1, ctx->stream));
        ctx->kernel_timed = timed;
        HIP_TRY(ctx, launch_hamming_self_merge(a, g.count, ctx->stream));
    }
    return FM_OK;
}

// ---------------------------------------------------------------------------------------
// Wide self distances (wide_f32.hip: the SELF forms of the filter, the rescoring and the exact kernel)
// ---------------------------------------------------------------------------------------
// Self distances of n wide banks on the context's stream, each into d_out[i] (device, [banks[i]->n] float64): one sweep of
// the bank over itself per bank (wide_route, self), back to back -- separate banks share no stack, so the table forms do not
// apply -- and fm_self_dist's merge over the splits (float32-bit keys; no key: +inf).  Enqueue only.
static int wide_selfdist_device(fm_ctx* ctx, int n, const fm_bank* const* banks, double* const* d_out, bool timed)
{
    for (int i = 0; i < n; ++i) {
        const fm_bank* b = banks[i];
        if (b->n == 0) continue;
        RowReducePlan pl;
        int rc = wide_route(ctx, *b, *b, 1, &pl, true);
        if (rc != FM_OK) return rc;
        ctx->kernel_timed = timed;
        ctx->pending_pairs += b->n * b->n;
        ctx->pending_bytes += bank_bytes(b);
        SelfMerge m{};
        m.partial[0] = (const unsigned long long*)ctx->ws_partial;
        m.out[0] = d_out[i];
        hipLaunchKernelGGL(selfdist_merge_kernel, dim3((unsigned)((b->n + 255) / 256), 1), dim3(256), 0, ctx->stream,
                           m, pl.nsplit, pl.ncols_alloc, b->n, 1);
        HIP_TRY(ctx, hipGetLastError());
    }
    return FM_OK;
}

// The two families of calls under names of their own -- fm_hamming_* on binary banks, fm_wide_* on wide float banks: the kind
// they serve, how a refusal describes it, the family's self-distance sweep and the calls that attach self distances.
struct NamedFamily {
    int kind; const char* one; const char* both;
    int (*selfdist)(fm_ctx*, int, const fm_bank* const*, double* const*, bool);
    const char* attach;
};
static const NamedFamily kHamFamily{FM_BANK_BIN, "the bank must be binary (FM_BANK_BIN, fm_bank_create_bin)",
                                    "both banks must be binary (FM_BANK_BIN, fm_bank_create_bin)", ham_selfdist_device,
                                    "fm_hamming_set_selfdist, fm_hamming_self_dist_batch"};
static const NamedFamily kWideFamily{FM_BANK_F32W, "the bank must be wide float (FM_BANK_F32W: fm_bank_create_f32 with 129 .. 256 values per row)",
                                     "both banks must be wide float (FM_BANK_F32W: fm_bank_create_f32 with 129 .. 256 values per row)",
                                     wide_selfdist_device, "fm_wide_set_selfdist, fm_wide_self_dist_batch"};

// "<l2> is the L2 call", or for the wide family's refusal of a binary bank "<ham> is the Hamming call"
static std::string named_served_by(const fm_bank* b, const char* l2, const char* ham)
{
    if (ham && b->kind == FM_BANK_BIN) return std::string(ham) + " is the Hamming call";
    return std::string(l2) + " is the L2 call";
}

// The checks of a family's self-distance calls: handles, then a bank of the family's kind (l2 / ham: the calls the message names)
static int named_bank_check(fm_ctx* ctx, const fm_bank* b, const NamedFamily& f, const char* who, const char* l2, const char* ham = nullptr)
{
    if (!ctx) return fail(nullptr, FM_EINVAL, std::string(who) + ": ctx is NULL");
    if (!b) return fail(ctx, FM_EINVAL, std::string(who) + ": bank is NULL");
    if (int rc = refuse_bin2(ctx, b, who)) return rc;
    if (b->kind != f.kind) return fail(ctx, FM_EINVAL, std::string(who) + ": " + f.one + "; " + named_served_by(b, l2, ham));
    return FM_OK;
}

static int named_self_dist(fm_ctx* ctx, const fm_bank* bank, double* selfdist, const NamedFamily& f, const char* who, const char* l2, const char* ham = nullptr)
{
    int rc = named_bank_check(ctx, bank, f, who, l2, ham);
    if (rc != FM_OK) return rc;
    const int64_t n = bank->n;
    if (n == 0) return FM_OK;
    if (!selfdist) return fail(ctx, FM_EINVAL, std::string(who) + ": output pointer is NULL");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((rc = ws_ensure(ctx, &ctx->ws_in, &ctx->ws_in_bytes, (size_t)n * 8 + 64)) != FM_OK) return rc;
    double* d_sd = (double*)ctx->ws_in;
    CallScope cs(ctx);
    if ((rc = f.selfdist(ctx, 1, &bank, &d_sd, true)) != FM_OK) return rc;
    HIP_TRY(ctx, d2h(ctx, selfdist, d_sd, (size_t)n * 8));
    return cs.finish();
}

static int named_self_dist_batch(fm_ctx* ctx, int32_t n, fm_bank* const* banks, double* const* out, const NamedFamily& f, const char* who_,
                                 const char* l2, const char* ham = nullptr)
{
    const std::string who(who_);
    if (!ctx) return fail(nullptr, FM_EINVAL, who + ": ctx is NULL");
    if (n < 0) return fail(ctx, FM_EINVAL, who + ": n < 0");
    if (n == 0) return FM_OK;
    if (!banks) return fail(ctx, FM_EINVAL, who + ": banks is NULL");
    for (int i = 0; i < n; ++i) {
        if (int rc = named_bank_check(ctx, banks[i], f, who_, l2, ham)) return rc;
        for (int j = 0; j < i; ++j) if (banks[j] == banks[i]) return fail(ctx, FM_EINVAL, who + ": a bank is listed twice");
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::vector<double*> d_out((size_t)n, nullptr);
    std::vector<const fm_bank*> cb((size_t)n, nullptr);
    bool any_out = false;
    int rc;
    for (int i = 0; i < n; ++i) {
        fm_bank* b = banks[i];
        if ((rc = bank_selfdist_alloc(ctx, b)) != FM_OK) return rc;
        b->sdmax_rows = -1;           // (no ratio cut is built on these self distances)
        d_out[(size_t)i] = b->selfdist;
        cb[(size_t)i] = b;
        any_out = any_out || (out && out[i] && b->n > 0);
    }
    if (!any_out) {
        // enqueue only: accounted at the next fm_sync like the other asynchronous calls (fm_self_dist_batch)
        fm_ctx::PendingTimer tm;
        if ((rc = take_timer(ctx, &tm)) != FM_OK) return rc;
        const int64_t before = ctx->pending_pairs, before_b = ctx->pending_bytes;
        ctx->pending_pairs = 0;
        ctx->pending_bytes = 0;
        HIP_TRY(ctx, hipEventRecord(tm.k0, ctx->stream));
        rc = f.selfdist(ctx, n, cb.data(), d_out.data(), false);
        HIP_TRY(ctx, hipEventRecord(tm.k1, ctx->stream));
        HIP_TRY(ctx, hipEventRecord(tm.c1, ctx->stream));
        tm.timed = rc == FM_OK && ctx->pending_pairs > 0;
        tm.call_timed = true;
        tm.pairs = ctx->pending_pairs;
        tm.bytes = ctx->pending_bytes;
        ctx->pending_pairs = before;
        ctx->pending_bytes = before_b;
        ctx->pending.push_back(tm);
        return rc;
    }
    CallScope cs(ctx);
    if ((rc = f.selfdist(ctx, n, cb.data(), d_out.data(), true)) != FM_OK) return rc;
    for (int i = 0; i < n; ++i)
        if (out[i] && banks[i]->n > 0) HIP_TRY(ctx, d2h(ctx, out[i], d_out[(size_t)i], (size_t)banks[i]->n * 8));
    return cs.finish();
}

static int named_set_selfdist(fm_ctx* ctx, fm_bank* bank, const double* selfdist, const NamedFamily& f, const char* who, const char* l2,
                              const char* ham = nullptr)
{
    int rc = named_bank_check(ctx, bank, f, who, l2, ham);
    if (rc != FM_OK) return rc;
    if (bank->n > 0 && !selfdist) return fail(ctx, FM_EINVAL, std::string(who) + ": selfdist is NULL");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((rc = bank_selfdist_alloc(ctx, bank)) != FM_OK) return rc;
    bank->sdmax_rows = -1;
    if (bank->n > 0) {
        HIP_TRY(ctx, hipMemcpyAsync(bank->selfdist, selfdist, (size_t)bank->n * 8, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    return FM_OK;
}

extern "C" int fm_hamming_self_dist(fm_ctx* ctx, const fm_bank* bank, double* selfdist)
{
    return named_self_dist(ctx, bank, selfdist, kHamFamily, "fm_hamming_self_dist", "fm_self_dist");
}

extern "C" int fm_hamming_self_dist_batch(fm_ctx* ctx, int32_t n, fm_bank* const* banks, double* const* out)
{
    return named_self_dist_batch(ctx, n, banks, out, kHamFamily, "fm_hamming_self_dist_batch", "fm_self_dist_batch");
}

extern "C" int fm_hamming_set_selfdist(fm_ctx* ctx, fm_bank* bank, const double* selfdist)
{
    return named_set_selfdist(ctx, bank, selfdist, kHamFamily, "fm_hamming_set_selfdist", "fm_bank_set_selfdist");
}

extern "C" int fm_wide_self_dist(fm_ctx* ctx, const fm_bank* bank, double* selfdist)
{
    return named_self_dist(ctx, bank, selfdist, kWideFamily, "fm_wide_self_dist", "fm_self_dist", "fm_hamming_self_dist");
}

extern "C" int fm_wide_self_dist_batch(fm_ctx* ctx, int32_t n, fm_bank* const* banks, double* const* out)
{
    return named_self_dist_batch(ctx, n, banks, out, kWideFamily, "fm_wide_self_dist_batch", "fm_self_dist_batch", "fm_hamming_self_dist_batch");
}

extern "C" int fm_wide_set_selfdist(fm_ctx* ctx, fm_bank* bank, const double* selfdist)
{
    return named_set_selfdist(ctx, bank, selfdist, kWideFamily, "fm_wide_set_selfdist", "fm_bank_set_selfdist", "fm_hamming_set_selfdist");
}

// ---------------------------------------------------------------------------------------
// X1 (+R1) entry points
// ---------------------------------------------------------------------------------------
// Workspace of one bank pair in flight (async calls): partial | bound | qbest | tidx | dist | ratio | pass | block counts
// "no consumer stream": NULL is a stream (the null stream, which PyTorch's default stream is)
static const hipStream_t kNoStream = (hipStream_t)FM_NO_STREAM;

struct SlotLayout {
    size_t pbytes, a_qbest, a_tidx, a_dist, a_ratio, a_pass, a_bc, a_fix, a_end;
    int nblk;
};

static SlotLayout slot_layout(int64_t nq, int64_t nt, const RowReducePlan& pl)
{
    SlotLayout L;
    L.nblk = (int)((nq + 255) / 256);
    L.pbytes = (pl.partial_bytes(1) + 15) & ~(size_t)15;
    const size_t bbytes = ((size_t)pl.ncols_alloc * 4 + 15) & ~(size_t)15;
    L.a_qbest = L.pbytes + bbytes; L.a_tidx = L.a_qbest + (size_t)nq * 8; L.a_dist = L.a_tidx + (size_t)nq * 4;
    L.a_ratio = (L.a_dist + (size_t)nq * 4 + 7) & ~(size_t)7; L.a_pass = L.a_ratio + (size_t)nq * 8;
    L.a_bc = (L.a_pass + (size_t)nq + 15) & ~(size_t)15;
    L.a_fix = (L.a_bc + (size_t)L.nblk * 4 + 16 + 15) & ~(size_t)15;       // tie-repair list (enqueue_election)
    L.a_end = L.a_fix + fix_bytes(nt);
    return L;
}

// Make the slot ready for a K1 on stream ks: wait for the slot's previous tail (it reads partial /
// qbest and re-arms bound), (re)allocate and initialise the arrays when the shape changed.
static int slot_prepare(fm_ctx* ctx, fm_ctx::AsyncSlot& sl, const SlotLayout& L, int64_t nq, const RowReducePlan& pl, hipStream_t ks)
{
    if (sl.in_use) HIP_TRY(ctx, hipStreamWaitEvent(ks, sl.tail_done, 0));
    if (L.a_end > sl.bytes || sl.nq != nq || sl.ncols_alloc != pl.ncols_alloc || sl.partial_bytes != (int64_t)L.pbytes) {
        if (sl.in_use) HIP_TRY(ctx, hipEventSynchronize(sl.tail_done));
        if (L.a_end > sl.bytes) {
            if (sl.ws) { HIP_TRY(ctx, hipFree(sl.ws)); sl.ws = nullptr; sl.bytes = 0; }
            HIP_TRY(ctx, hipMalloc(&sl.ws, L.a_end + L.a_end / 4));
            sl.bytes = L.a_end + L.a_end / 4;
        }
        HIP_TRY(ctx, hipMemsetD32Async((hipDeviceptr_t)((char*)sl.ws + L.pbytes), (int)0x80000000, (size_t)pl.ncols_alloc, ks));
        HIP_TRY(ctx, hipMemsetAsync((char*)sl.ws + L.a_qbest, 0xff, (size_t)nq * 8, ks));
        sl.nq = nq; sl.ncols_alloc = pl.ncols_alloc; sl.partial_bytes = (int64_t)L.pbytes;
    }
    return FM_OK;
}

static int take_timer(fm_ctx* ctx, fm_ctx::PendingTimer* tm)
{
    if (!ctx->timer_pool.empty()) { *tm = ctx->timer_pool.back(); ctx->timer_pool.pop_back(); return FM_OK; }
    if (ctx->pending.size() >= 1024) {                 // bound the number of live events
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        for (hipStream_t ts : ctx->tails) if (ts) HIP_TRY(ctx, hipStreamSynchronize(ts));
        drain_pending(ctx);
        *tm = ctx->timer_pool.back(); ctx->timer_pool.pop_back();
        return FM_OK;
    }
    HIP_TRY(ctx, hipEventCreate(&tm->c0)); HIP_TRY(ctx, hipEventCreate(&tm->c1));
    HIP_TRY(ctx, hipEventCreate(&tm->k0)); HIP_TRY(ctx, hipEventCreate(&tm->k1));
    return FM_OK;
}

// ---- the tail behind a reverse top-1 sweep: election, decode (+ ratio test), ordered compaction, delivery ---------------
// Cross-check up to the election on the context's stream, all three bank kinds: d_qbest[q] = (float32 distance bits << 32 |
// t_offset + train row) of the closest train row that elects q, ~0 if none.  Reverse NN: output rows = train rows, reduced
// over the query rows.  cut: launch_rowreduce's (enqueue_ratio_cut) or null.
static int xcheck_keys_device(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, unsigned t_offset, const unsigned* cut,
                              unsigned long long* d_qbest)
{
    HIP_TRY(ctx, hipMemsetAsync(d_qbest, 0xff, (size_t)q->n * 8, ctx->stream));
    if (t->n == 0) return FM_OK;
    PairSweep ps;
    int rc = sweep_pair(ctx, *t, *q, 1, t->n, cut, nullptr, 0, &ps);
    if (rc != FM_OK) return rc;
    return enqueue_election(ctx, ctx->stream, q, t, ps.partial, ps.nsplit, ps.ncols_alloc, ps.f32_keys, d_qbest, t_offset, nullptr, ps.fix);
}

// Device-side cross-checked 1-NN into d_tidx / d_dist (device pointers; d_qbest: nq scratch words): the keys, then the plain
// decode.  consumer (fm_xcheck1_dev: the arrays are the caller's): the stream whose work so far the decode -- the kernel that
// writes them -- waits for, behind the sweep and the election.
static int xcheck1_device(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, unsigned long long* d_qbest, int32_t* d_tidx,
                          float* d_dist, void* consumer)
{
    int rc;
    if ((rc = xcheck_keys_device(ctx, q, t, 0u, nullptr, d_qbest)) != FM_OK) return rc;
    if ((rc = wait_for_stream(ctx, consumer)) != FM_OK) return rc;
    hipLaunchKernelGGL(xcheck_finalize_kernel, dim3((unsigned)((q->n + 255) / 256)), dim3(256), 0, ctx->stream,
                       (const unsigned long long*)d_qbest, q->n, (const double*)nullptr, 0.0, d_tidx, d_dist, (double*)nullptr,
                       (uint8_t*)nullptr, (unsigned long long*)nullptr, (int*)nullptr, (unsigned long long*)nullptr);
    HIP_TRY(ctx, hipGetLastError());
    return FM_OK;
}

// Where the rows of one pair's ratio test go.  Host form: the caller's arrays (cap < 0, fm_match_ratio: one row per query,
// no qidx; cap >= 0: the accepted rows, compacted); device form: 12-byte rows and their count in caller device memory.
// n_host: the host word that receives the full number of accepted rows (optional in the device form).
struct AcceptedSink {
    int32_t* qidx = nullptr; int32_t* tidx = nullptr; float* dist = nullptr; double* ratio = nullptr;
    int32_t* dev_rows = nullptr; long long* dev_count = nullptr;
    int64_t* n_host = nullptr;
    unsigned long long* count = nullptr;   // aliased(): n_host as a kernel writes it
    int64_t cap = -1;
    hipStream_t consumer = kNoStream;      // device form: the stream that reads dev_rows / dev_count

    bool to_device() const { return dev_rows != nullptr; }
    // The same sink as the kernels see it: every host pointer replaced by its page-locked device alias (null: pageable).
    AcceptedSink aliased() const
    {
        AcceptedSink a = *this;
        a.qidx = (int32_t*)pinned_device_alias(qidx); a.tidx = (int32_t*)pinned_device_alias(tidx);
        a.dist = (float*)pinned_device_alias(dist);   a.ratio = (double*)pinned_device_alias(ratio);
        a.count = (unsigned long long*)pinned_device_alias(n_host);
        return a;
    }
    // (of an aliased sink) a compaction can write everything the caller gave: all five host aliases, or, in the device form,
    // the count word if there is one
    bool writable() const { return to_device() ? (!n_host || count) : (qidx && tidx && dist && ratio && count); }
};

// The argument checks the ratio calls share, in the order the header documents; n_host is zeroed on the way.  A pair without
// query rows passes: the caller returns.
// named: a binary or a wide pair that named_pair_check (the fm_hamming_* / fm_wide_* entry points) has passed already --
// handles, kinds, widths and the self distances, in the order the header gives for them.
static int ratio_call_check(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, const AcceptedSink& out, const char* who, bool named = false)
{
    int rc = named ? FM_OK : check_pair(ctx, q, t, who);
    if (rc != FM_OK) return rc;
    if (out.n_host) *out.n_host = 0;
    if (q->n == 0) return FM_OK;
    if (!out.to_device() && (!out.tidx || !out.dist || (out.cap >= 0 && (!out.qidx || !out.ratio))))
        return fail(ctx, FM_EINVAL, std::string(who) + ": output pointer is NULL");
    if (!q->selfdist) return fail(ctx, FM_EINVAL, std::string(who) + ": query bank has no self distances (fm_bank_set_selfdist)");
    return FM_OK;
}

// The small kernels behind a K1 (election, decode + ratio test, ordered compaction), on stream ts,
// which must already wait for that K1.  `al`: the pair's sink, aliased and writable.  Leaves the slot's bound[] / qbest[] clean.
static int enqueue_tail(fm_ctx* ctx, hipStream_t ts, fm_ctx::AsyncSlot& sl, const SlotLayout& L, const fm_bank* q,
                        const fm_bank* t, const RowReducePlan& pl, double tau, const AcceptedSink& al)
{
    const int64_t nq = q->n, nt = t->n;
    char* sb = (char*)sl.ws;
    unsigned long long* s_partial = (unsigned long long*)sb;
    int* s_bound = (int*)(sb + L.pbytes);
    unsigned long long* s_qbest = (unsigned long long*)(sb + L.a_qbest);
    int32_t* s_tidx = (int32_t*)(sb + L.a_tidx);
    float* s_dist = (float*)(sb + L.a_dist);
    double* s_ratio = (double*)(sb + L.a_ratio);
    uint8_t* s_pass = (uint8_t*)(sb + L.a_pass);
    int* s_bc = (int*)(sb + L.a_bc);
    if (nt > 0) {
        unsigned* s_fix = sqrt_tie_possible(*q, *t) ? (unsigned*)(sb + L.a_fix) : nullptr;      // (integer-route pairs only get here)
        if (s_fix) HIP_TRY(ctx, hipMemsetAsync(s_fix, 0, 16, ts));
        int rc = enqueue_election(ctx, ts, q, t, s_partial, pl.nsplit, pl.ncols_alloc, 0, s_qbest, 0u, s_bound, s_fix);
        if (rc != FM_OK) return rc;
    }
    hipLaunchKernelGGL(xcheck_finalize_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, ts,
                       (const unsigned long long*)s_qbest, nq, (const double*)q->selfdist, tau, s_tidx, s_dist, s_ratio,
                       s_pass, (unsigned long long*)nullptr, s_bc, s_qbest);
    if (al.to_device()) {
        // the rows go to the caller's device buffers, which a consumer stream (the result gather)
        // reads: the compaction waits for what that stream has been given so far (the gather that
        // last read these buffers), and the stream waits for the compaction
        if (al.consumer != kNoStream) {
            HIP_TRY(ctx, hipEventRecord(ctx->ev_consumer, al.consumer));
            HIP_TRY(ctx, hipStreamWaitEvent(ts, ctx->ev_consumer, 0));
        }
        hipLaunchKernelGGL(compact_rows_kernel, dim3((unsigned)L.nblk), dim3(256), 0, ts,
                           (const int32_t*)s_tidx, (const float*)s_dist, (const uint8_t*)s_pass,
                           (const int*)s_bc, nq, al.cap, al.dev_rows, al.dev_count, al.count);
    } else {
        hipLaunchKernelGGL(compact_kernel, dim3((unsigned)L.nblk), dim3(256), 0, ts,
                           (const int32_t*)s_tidx, (const float*)s_dist, (const double*)s_ratio, (const uint8_t*)s_pass,
                           (const int*)s_bc, nq, al.cap < nq ? al.cap : nq, al.qidx, al.tidx, al.dist, al.ratio, al.count);
    }
    HIP_TRY(ctx, hipGetLastError());
    return FM_OK;
}

// The synchronous ratio calls (fm_match_ratio, fm_match_accepted, fm_match_accepted_dev, a float32 pair inside a batch): keys,
// decode + ratio test, then by the sink -- every row and its flag (pass: fm_match_ratio's, optional), the compaction into
// page-locked caller arrays directly, the compaction into ws_out and the staged delivery, or the device rows.
static int ratio_sync(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, double tau, const AcceptedSink& out, uint8_t* pass, const char* who,
                      bool named = false)
{
    int rc = ratio_call_check(ctx, q, t, out, who, named);
    if (rc != FM_OK || q->n == 0) return rc;
    const bool compact = out.cap >= 0, to_device = out.to_device();
    const int64_t nq = q->n;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // qbest u64[nq] | tidx i32[nq] | dist f32[nq] | ratio f64[nq] | pass u8[nq] | count u64 | block counts | compacted qidx, tidx, dist, ratio
    const int nblk = (int)((nq + 255) / 256);
    const int64_t ccap = (compact && !to_device) ? (out.cap < nq ? out.cap : nq) : 0;
    size_t off = 0;
    const size_t o_qbest = carve(off, (size_t)nq * 8, 16), o_tidx = carve(off, (size_t)nq * 4, 16), o_dist = carve(off, (size_t)nq * 4, 16);
    const size_t o_ratio = carve(off, (size_t)nq * 8, 16), o_pass = carve(off, (size_t)nq, 16), o_cnt = carve(off, 16, 16), o_bc = carve(off, (size_t)nblk * 4, 16);
    const size_t o_cq = carve(off, (size_t)ccap * 4, 16), o_ct = carve(off, (size_t)ccap * 4, 16), o_cd = carve(off, (size_t)ccap * 4, 16), o_cr = carve(off, (size_t)ccap * 8, 16);
    if ((rc = ws_ensure(ctx, &ctx->ws_out, &ctx->ws_out_bytes, off + 16)) != FM_OK) return rc;
    char* base = (char*)ctx->ws_out;
    unsigned long long* d_qbest = (unsigned long long*)(base + o_qbest);
    int32_t* d_tidx = (int32_t*)(base + o_tidx);
    float* d_dist = (float*)(base + o_dist);
    double* d_ratio = (double*)(base + o_ratio);
    uint8_t* d_pass = (uint8_t*)(base + o_pass);
    unsigned long long* d_cnt = (unsigned long long*)(base + o_cnt);
    int* d_bc = (int*)(base + o_bc);
    CallScope cs(ctx);
    if (!compact) HIP_TRY(ctx, hipMemsetAsync(d_cnt, 0, 8, ctx->stream));      // (a compaction writes the count itself)
    // (accepted-only: only rows that pass the ratio test are reported -- K1 may drop what cannot pass)
    const unsigned* cut = nullptr;
    if (t->n > 0 && q->kind != FM_BANK_F32 && compact && (rc = enqueue_ratio_cut(ctx, 1, &q, tau, &cut)) != FM_OK) return rc;
    if ((rc = xcheck_keys_device(ctx, q, t, 0u, cut, d_qbest)) != FM_OK) return rc;
    hipLaunchKernelGGL(xcheck_finalize_kernel, dim3((unsigned)nblk), dim3(256), 0, ctx->stream, (const unsigned long long*)d_qbest, nq,
                       (const double*)q->selfdist, tau, d_tidx, d_dist, d_ratio, d_pass, d_cnt, compact ? d_bc : (int*)nullptr);
    HIP_TRY(ctx, hipGetLastError());
    if (!compact) {
        unsigned long long cnt = 0;
        HIP_TRY(ctx, d2h(ctx, out.tidx, d_tidx, (size_t)nq * 4));
        HIP_TRY(ctx, d2h(ctx, out.dist, d_dist, (size_t)nq * 4));
        if (out.ratio) HIP_TRY(ctx, d2h(ctx, out.ratio, d_ratio, (size_t)nq * 8));
        if (pass) HIP_TRY(ctx, d2h(ctx, pass, d_pass, (size_t)nq));
        HIP_TRY(ctx, hipMemcpyAsync(&cnt, d_cnt, 8, hipMemcpyDeviceToHost, ctx->stream));
        if ((rc = cs.finish()) != FM_OK) return rc;
        if (out.n_host) *out.n_host = (int64_t)cnt;
        return FM_OK;
    }
    // the count through the context's page-locked word where there is one: no copy, a single synchronisation
    unsigned long long* a_c = (unsigned long long*)pinned_device_alias(ctx->h_scratch);
    if (to_device) {
        // accepted matches stay on the device as packed rows (multi-GPU gather input)
        ctx->rows_stream = ctx->stream;
        unsigned long long cnt = 0;
        hipLaunchKernelGGL(compact_rows_kernel, dim3((unsigned)nblk), dim3(256), 0, ctx->stream, (const int32_t*)d_tidx, (const float*)d_dist,
                           (const uint8_t*)d_pass, (const int*)d_bc, nq, out.cap, out.dev_rows, out.dev_count, a_c);
        HIP_TRY(ctx, hipGetLastError());
        if (!a_c) HIP_TRY(ctx, hipMemcpyAsync(&cnt, out.dev_count, 8, hipMemcpyDeviceToHost, ctx->stream));
        if ((rc = cs.finish()) != FM_OK) return rc;
        if (out.n_host) *out.n_host = a_c ? (int64_t)ctx->h_scratch[0] : (int64_t)cnt;
        return FM_OK;
    }
    const AcceptedSink al = out.aliased();
    if (al.qidx && al.tidx && al.dist && al.ratio && a_c && out.cap <= nq) {
        // caller-owned page-locked outputs: the compaction writes them (and the count) directly, no staging copies
        hipLaunchKernelGGL(compact_kernel, dim3((unsigned)nblk), dim3(256), 0, ctx->stream, (const int32_t*)d_tidx, (const float*)d_dist,
                           (const double*)d_ratio, (const uint8_t*)d_pass, (const int*)d_bc, nq, ccap, al.qidx, al.tidx, al.dist, al.ratio, a_c);
        HIP_TRY(ctx, hipGetLastError());
        if ((rc = cs.finish()) != FM_OK) return rc;
        if (out.n_host) *out.n_host = (int64_t)ctx->h_scratch[0];
        return FM_OK;
    }
    hipLaunchKernelGGL(compact_kernel, dim3((unsigned)nblk), dim3(256), 0, ctx->stream, (const int32_t*)d_tidx, (const float*)d_dist,
                       (const double*)d_ratio, (const uint8_t*)d_pass, (const int*)d_bc, nq, ccap, (int32_t*)(base + o_cq),
                       (int32_t*)(base + o_ct), (float*)(base + o_cd), (double*)(base + o_cr), d_cnt);
    HIP_TRY(ctx, hipGetLastError());
    return cs.finish_rows(d_cnt, ccap, {{out.qidx, base + o_cq, 4}, {out.tidx, base + o_ct, 4}, {out.dist, base + o_cd, 4}, {out.ratio, base + o_cr, 8}},
                          out.n_host);
}

// The enqueue-only form of the accepted call (fm_match_accepted_async, fm_match_accepted_dev_async, an odd pair of a batch):
// K1 on the context's stream into a workspace slot of its own, the tail on stream_tail beside the NEXT call's K1; the
// compaction writes page-locked caller memory or the device rows, the events of the call are read at fm_sync.
static int ratio_enqueue(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, double tau, const AcceptedSink& out, const char* who)
{
    int rc = ratio_call_check(ctx, q, t, out, who);
    if (rc != FM_OK || q->n == 0) return rc;
    const int64_t nq = q->n, nt = t->n;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (q->kind == FM_BANK_F32) return fail(ctx, FM_EINVAL, std::string(who) + ": needs integer-valued banks");
    const AcceptedSink al = out.aliased();
    if (!al.writable()) return fail(ctx, FM_EINVAL, std::string(who) + ": host outputs must be page-locked (fm_host_alloc)");
    // (reverse NN: output rows = train rows, reduced over the query rows; the slot owns the sweep's workspace)
    const RowReducePlan pl = plan_rowreduce(t->n_pad, q->n_pad, ctx->tune);
    fm_ctx::PendingTimer tm;
    if ((rc = take_timer(ctx, &tm)) != FM_OK) return rc;
    tm.pairs = nq * nt;
    tm.bytes = bank_bytes(q) + bank_bytes(t);
    fm_ctx::AsyncSlot& sl = ctx->aslot[ctx->aslot_next];
    ctx->aslot_next ^= 1;
    const SlotLayout L = slot_layout(nq, nt, pl);
    const bool coop = (ctx->tune.coop != 0) && pl.nsplit > 1;
    // Every event record is a packet the K1 launches of consecutive calls queue behind; the
    // start-of-kernel event is therefore taken for every async_time_every-th call only (those
    // calls are the ones fm_get_stats accounts as timed K1 launches; option async_time_every, default 4).
    const int time_every = ctx->tune.async_time_every;
    const bool timed_call = time_every > 0 && (ctx->async_calls++ % time_every) == 0;
    tm.timed = nt > 0 && timed_call;
    tm.call_timed = timed_call;
    const unsigned* cut = nullptr;
    if ((rc = slot_prepare(ctx, sl, L, nq, pl, ctx->stream)) != FM_OK ||
        (nt > 0 && (rc = enqueue_ratio_cut(ctx, 1, &q, tau, &cut)) != FM_OK)) {
        ctx->timer_pool.push_back(tm);          // (no event of the set is recorded yet: it goes back)
        return rc;
    }
    if (timed_call) HIP_TRY(ctx, hipEventRecord(tm.k0, ctx->stream));
    if (nt > 0)
        HIP_TRY(ctx, launch_rowreduce(*t, *q, 1, pl, (unsigned long long*)sl.ws, coop ? (int*)((char*)sl.ws + L.pbytes) : nullptr,
                                      (ctx->tune.glds != 0), ctx->stream, cut, cut ? filter6_ws(ctx, 1) : nullptr));
    // (untimed calls hand over through the slot's own event, created without timing)
    hipEvent_t handover = timed_call ? tm.k1 : sl.k_done;
    HIP_TRY(ctx, hipEventRecord(handover, ctx->stream));
    HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream_tail, handover, 0));
    if ((rc = enqueue_tail(ctx, ctx->stream_tail, sl, L, q, t, pl, tau, al)) != FM_OK) return rc;
    if (timed_call) HIP_TRY(ctx, hipEventRecord(tm.c1, ctx->stream_tail));
    HIP_TRY(ctx, hipEventRecord(sl.tail_done, ctx->stream_tail));
    if (al.to_device() && al.consumer != kNoStream) HIP_TRY(ctx, hipStreamWaitEvent(al.consumer, sl.tail_done, 0));
    ctx->rows_stream = al.to_device() ? ctx->stream_tail : ctx->stream;
    sl.in_use = true;
    ctx->pending.push_back(tm);
    return FM_OK;
}

// X1 up to the election, for a train set sharded over ranks: keys[q] =
// (distance key << 32) | (t_offset + local train row) of the closest train row OF THIS BANK that
// elects q, ~0 if none.  The element-wise minimum of the ranks' key arrays is the key array of
// the unsharded call (the key carries the global index, so ties break as on one GPU).
static int xcheck1_keys_common(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, int64_t t_offset, uint64_t* keys, bool keys_on_device);

extern "C" int fm_xcheck1_keys(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, int64_t t_offset, uint64_t* keys)
{
    return xcheck1_keys_common(ctx, q, t, t_offset, keys, false);
}

extern "C" int fm_xcheck1_keys_dev(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, int64_t t_offset, uint64_t* d_keys)
{
    if (q && t && (bin_or_wide(q) || bin_or_wide(t))) return check_pair(ctx, q, t, "fm_xcheck1_keys_dev");
    if (ctx && d_keys)
        if (int rc = check_device_ptr(ctx, d_keys, "fm_xcheck1_keys_dev", "d_keys", false)) return rc;
    return xcheck1_keys_common(ctx, q, t, t_offset, d_keys, true);
}

static int xcheck1_keys_common(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, int64_t t_offset, uint64_t* keys, bool keys_on_device)
{
    int rc = check_pair(ctx, q, t, "fm_xcheck1_keys");
    if (rc != FM_OK) return rc;
    const int64_t nq = q->n, nt = t->n;
    if (nq == 0) return FM_OK;
    if (!keys) return fail(ctx, FM_EINVAL, "fm_xcheck1_keys: output pointer is NULL");
    if (t_offset < 0 || t_offset + nt > (int64_t)UINT32_MAX) return fail(ctx, FM_EINVAL, "fm_xcheck1_keys: t_offset + rows must fit 32 bits");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((rc = ws_ensure(ctx, &ctx->ws_out, &ctx->ws_out_bytes, (size_t)nq * 8 + 64)) != FM_OK) return rc;
    unsigned long long* d_qbest = (unsigned long long*)ctx->ws_out;
    CallScope cs(ctx);
    if ((rc = xcheck_keys_device(ctx, q, t, (unsigned)t_offset, nullptr, d_qbest)) != FM_OK) return rc;
    if (keys_on_device) HIP_TRY(ctx, hipMemcpyAsync(keys, d_qbest, (size_t)nq * 8, hipMemcpyDeviceToDevice, ctx->stream));
    else HIP_TRY(ctx, d2h(ctx, keys, d_qbest, (size_t)nq * 8));
    return cs.finish();
}

// crossCheck of BFMatcher for all three bank kinds (binary: K11's reverse top-1 sweep on the FP4 matrix cores; its keys are in the
// float32-route layout, high word = float32 bits of h).
extern "C" int fm_xcheck1(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, int32_t* tidx, float* dist)
{
    int rc = check_pair(ctx, q, t, "fm_xcheck1", true, true);
    if (rc != FM_OK) return rc;
    const int64_t nq = q->n;
    if (nq == 0) return FM_OK;
    if (!tidx || !dist) return fail(ctx, FM_EINVAL, "fm_xcheck1: output pointer is NULL");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // qbest u64[nq] | tidx i32[nq] | dist f32[nq]
    if ((rc = ws_ensure(ctx, &ctx->ws_out, &ctx->ws_out_bytes, (size_t)nq * 16 + 64)) != FM_OK) return rc;
    unsigned long long* d_qbest = (unsigned long long*)ctx->ws_out;
    int32_t* d_tidx = (int32_t*)((char*)ctx->ws_out + (size_t)nq * 8);
    float* d_dist = (float*)((char*)ctx->ws_out + (size_t)nq * 12);
    CallScope cs(ctx);
    if ((rc = xcheck1_device(ctx, q, t, d_qbest, d_tidx, d_dist, FM_NO_STREAM)) != FM_OK) return rc;
    HIP_TRY(ctx, d2h(ctx, tidx, d_tidx, (size_t)nq * 4));
    HIP_TRY(ctx, d2h(ctx, dist, d_dist, (size_t)nq * 4));
    return cs.finish();
}

// ---------------------------------------------------------------------------------------
// results left in caller-supplied device memory: fm_knn_dev, fm_xcheck1_dev, fm_knn2_ratio_dev
// ---------------------------------------------------------------------------------------
// The host forms' pipelines on the context's stream, with the merge / finalize / compaction kernels given the caller's
// pointers: nothing is copied to the host and nothing waits for the device.  wait_for_stream(consumer) sits in front of
// the first kernel that writes the caller's arrays (the sweep before it overlaps whatever the consumer stream still does
// with them), results_written() behind the last.  The calls are not accounted in fm_stats (no synchronisation to read the
// events at).
int results_written(fm_ctx* ctx, void* consumer)
{
    if (consumer == FM_NO_STREAM) return FM_OK;
    if (!ctx->ev_results) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_results, hipEventDisableTiming));
    HIP_TRY(ctx, hipEventRecord(ctx->ev_results, ctx->stream));
    HIP_TRY(ctx, hipStreamWaitEvent((hipStream_t)consumer, ctx->ev_results, 0));
    return FM_OK;
}

// k = 1: the first column of the top-2 sweep's [n][2] lists
__global__ void knn_first_col_kernel(const int32_t* __restrict__ idx2, const float* __restrict__ dist2, int64_t n,
                                     int32_t* __restrict__ idx, float* __restrict__ dist)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { idx[i] = idx2[2 * i]; dist[i] = dist2[2 * i]; }
}

extern "C" int fm_knn_dev(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, int32_t k, int32_t* d_idx, float* d_dist, void* consumer_stream)
{
    int rc = check_pair(ctx, q, t, "fm_knn_dev", true, true);
    if (rc != FM_OK) return rc;
    if (k < 1) return fail(ctx, FM_EINVAL, "fm_knn_dev: k must be at least 1");
    if (k > 8) return fail(ctx, FM_EUNSUPPORTED, "fm_knn_dev: k above 8 is not built");
    if (k > 2 && q->kind == FM_BANK_F32W) return refuse_bin(ctx, q, "fm_knn_dev with k >= 3");
    const int64_t nq = q->n;
    if (nq == 0) return FM_OK;
    if (!d_idx || !d_dist) return fail(ctx, FM_EINVAL, "fm_knn_dev: output pointer is NULL");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((rc = check_device_ptr(ctx, d_idx, "fm_knn_dev", "d_idx")) != FM_OK || (rc = check_device_ptr(ctx, d_dist, "fm_knn_dev", "d_dist")) != FM_OK) return rc;
    if (k == 2) {
        if ((rc = knn2_device(ctx, q, t, d_idx, d_dist, consumer_stream)) != FM_OK) return rc;
    } else if (k == 1) {
        if ((rc = ws_ensure(ctx, &ctx->ws_out, &ctx->ws_out_bytes, (size_t)nq * 16 + 64)) != FM_OK) return rc;
        int32_t* d_idx2 = (int32_t*)ctx->ws_out;
        float* d_dist2 = (float*)((char*)ctx->ws_out + (size_t)nq * 8);
        if ((rc = knn2_device(ctx, q, t, d_idx2, d_dist2)) != FM_OK) return rc;
        if ((rc = wait_for_stream(ctx, consumer_stream)) != FM_OK) return rc;
        hipLaunchKernelGGL(knn_first_col_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, ctx->stream,
                           (const int32_t*)d_idx2, (const float*)d_dist2, nq, d_idx, d_dist);
        HIP_TRY(ctx, hipGetLastError());
    } else {
        // K9 / K11's vector-ALU lists: their merge kernel writes [nq][k] as asked for
        if ((rc = ws_ensure(ctx, &ctx->ws_partial, &ctx->ws_partial_bytes, knnk_partial_bytes(nq, t->n, k) + 64)) != FM_OK) return rc;
        if ((rc = wait_for_stream(ctx, consumer_stream)) != FM_OK) return rc;
        if (t->n == 0)      // (an empty bank has no kind of its own for the list kernels to dispatch on: the merge of no lists, -1 / +inf)
            HIP_TRY(ctx, launch_knnk_merge((const unsigned long long*)ctx->ws_partial, 0, (int)nq, k, d_idx, d_dist, ctx->stream));
        else if (q->kind == FM_BANK_BIN)
            HIP_TRY(ctx, launch_hamming_knnk(*q, *t, k, (unsigned long long*)ctx->ws_partial, d_idx, d_dist, ctx->stream));
        else if (q->kind == FM_BANK_BIN2)
            HIP_TRY(ctx, launch_hamming2_knnk(*q, *t, k, (unsigned long long*)ctx->ws_partial, d_idx, d_dist, ctx->stream));
        else
            HIP_TRY(ctx, launch_knnk(*q, *t, k, (unsigned long long*)ctx->ws_partial, d_idx, d_dist, ctx->stream));
    }
    return results_written(ctx, consumer_stream);
}

extern "C" int fm_xcheck1_dev(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, int32_t* d_tidx, float* d_dist, void* consumer_stream)
{
    int rc = check_pair(ctx, q, t, "fm_xcheck1_dev", true, true);
    if (rc != FM_OK) return rc;
    const int64_t nq = q->n;
    if (nq == 0) return FM_OK;
    if (!d_tidx || !d_dist) return fail(ctx, FM_EINVAL, "fm_xcheck1_dev: output pointer is NULL");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((rc = check_device_ptr(ctx, d_tidx, "fm_xcheck1_dev", "d_tidx")) != FM_OK || (rc = check_device_ptr(ctx, d_dist, "fm_xcheck1_dev", "d_dist")) != FM_OK) return rc;
    if ((rc = ws_ensure(ctx, &ctx->ws_out, &ctx->ws_out_bytes, (size_t)nq * 8 + 64)) != FM_OK) return rc;
    if ((rc = xcheck1_device(ctx, q, t, (unsigned long long*)ctx->ws_out, d_tidx, d_dist, consumer_stream)) != FM_OK) return rc;
    return results_written(ctx, consumer_stream);
}

extern "C" int fm_knn2_ratio_dev(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, double tau, int64_t cap, int32_t* d_rows,
                                 int64_t* d_count, int64_t* n_accepted, void* consumer_stream)
{
    int rc = check_pair(ctx, q, t, "fm_knn2_ratio_dev", true, true);
    if (rc != FM_OK) return rc;
    if (n_accepted) *n_accepted = 0;
    if (cap < 0 || !d_count || (cap > 0 && !d_rows)) return fail(ctx, FM_EINVAL, "fm_knn2_ratio_dev: bad output arguments");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((rc = check_device_ptr(ctx, d_count, "fm_knn2_ratio_dev", "d_count")) != FM_OK) return rc;
    if (cap > 0 && (rc = check_device_ptr(ctx, d_rows, "fm_knn2_ratio_dev", "d_rows")) != FM_OK) return rc;
    const int64_t nq = q->n;
    if (nq == 0) {
        if ((rc = wait_for_stream(ctx, consumer_stream)) != FM_OK) return rc;
        HIP_TRY(ctx, hipMemsetAsync(d_count, 0, 8, ctx->stream));
        return results_written(ctx, consumer_stream);
    }
    LoweWs w;
    if ((rc = knn2_lowe_device(ctx, q, t, tau, 0, &w)) != FM_OK) return rc;
    if ((rc = wait_for_stream(ctx, consumer_stream)) != FM_OK) return rc;
    // the ordered compaction of fm_knn2_ratio, into the 12-byte rows of fm_match_accepted_dev; w.cnt: the full count
    hipLaunchKernelGGL(compact_rows_kernel, dim3((unsigned)w.nblk), dim3(256), 0, ctx->stream, (const int32_t*)w.tidx, (const float*)w.dist,
                       (const uint8_t*)w.pass, (const int*)w.bc, nq, cap, d_rows, (long long*)d_count, w.cnt);
    HIP_TRY(ctx, hipGetLastError());
    if ((rc = results_written(ctx, consumer_stream)) != FM_OK) return rc;
    if (n_accepted) {       // (the one host synchronisation of the integer and binary routes: the caller asked for a host number)
        unsigned long long cnt = 0;
        HIP_TRY(ctx, hipMemcpyAsync(&cnt, w.cnt, 8, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        *n_accepted = (int64_t)cnt;
    }
    return FM_OK;
}

// ---------------------------------------------------------------------------------------
// mutual nearest neighbours + ratio test: fm_mutual_ratio, fm_mutual_ratio_dev (and, api_collection.hip, the per-image forms)
// ---------------------------------------------------------------------------------------
// hloc's "NN-ratio + mutual", kornia's match_smnn, cv2's knnMatch(k = 2) + ratio + crossCheck loop.  One full sweep: the
// forward 2-NN lists and Lowe's test as fm_knn2_ratio runs them; only the train rows that are the first neighbour of a
// query row that PASSED are asked for their nearest query rows -- they are gathered into a bank G and fm_knn2(G, q) is a
// sweep of n_cand x nq pairs, not nt x nq.  The candidate count is read back between the two (the call's host wait).
// Entry / block / candidate numbering: ctx_internal.h.
__global__ __launch_bounds__(256)
void lowe_each_kernel(const int32_t* __restrict__ idx2, const float* __restrict__ dist2, int64_t nq, int nblk,
                                 double tau, int32_t* __restrict__ tidx, float* __restrict__ dist,
                                 double* __restrict__ ratio, uint8_t* __restrict__ pass, int* __restrict__ block_counts)
{
    const int64_t q = (int64_t)(blockIdx.x % (unsigned)nblk) * 256 + threadIdx.x;
    const int64_t e = (int64_t)(blockIdx.x / (unsigned)nblk) * nq + q;
    bool p = false;
    if (q < nq) {
        const float d1 = dist2[2 * e], d2 = dist2[2 * e + 1];
        const double r = (idx2[2 * e + 1] >= 0) ? (double)d1 / (double)d2 : NAN;
        p = r < tau;
        tidx[e] = idx2[2 * e];
        dist[e] = d1;
        ratio[e] = r;
        pass[e] = p ? 1 : 0;
    }
    emit_block_count(__ballot(p), block_counts);
}

__global__ __launch_bounds__(256)
void mutual_cand_kernel(const int32_t* __restrict__ tidx, const uint8_t* __restrict__ pass,
                        const int* __restrict__ block_counts, int64_t nq, int nblk,
                        const int32_t* __restrict__ first_row, int32_t* __restrict__ cand_rows,
                        unsigned long long* __restrict__ n_cand)
{
    const int64_t img = blockIdx.x / (unsigned)nblk;
    const int64_t q = (int64_t)(blockIdx.x % (unsigned)nblk) * 256 + threadIdx.x;
    const int64_t e = img * nq + q;
    const bool p = q < nq && pass[e];
    int64_t total;
    const int64_t c = compact_rank(block_counts, (int)blockIdx.x, p, &total);
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) *n_cand = (unsigned long long)total;
    if (p) cand_rows[c] = (first_row ? first_row[img] : 0) + tidx[e];
}

__global__ __launch_bounds__(256)
void mutual_join_kernel(const uint8_t* __restrict__ pass, const int* __restrict__ block_counts, int64_t nq, int nblk,
                        const int32_t* __restrict__ r_idx, const float* __restrict__ r_dist, double tau, int symmetric,
                        double* __restrict__ ratio, uint8_t* __restrict__ pass2, int* __restrict__ block_counts2)
{
    const int64_t q = (int64_t)(blockIdx.x % (unsigned)nblk) * 256 + threadIdx.x;
    const int64_t e = (int64_t)(blockIdx.x / (unsigned)nblk) * nq + q;
    const bool p = q < nq && pass[e];
    int64_t total;
    const int64_t c = compact_rank(block_counts, (int)blockIdx.x, p, &total);
    bool keep = false;
    if (p) {
        keep = r_idx[2 * c] == (int32_t)q;                 // mutual: the train row's nearest query row (lowest index on ties)
        if (keep && symmetric) {
            const double r = (r_idx[2 * c + 1] >= 0) ? (double)r_dist[2 * c] / (double)r_dist[2 * c + 1] : NAN;
            keep = r < tau;
            if (keep && r > ratio[e]) ratio[e] = r;
        }
    }
    if (q < nq) pass2[e] = keep ? 1 : 0;
    emit_block_count(__ballot(keep), block_counts2);
}

// Up to four planes of a bank's rows, moved by 16-byte units (4-byte units for the per-row words); the slots from n up to
// n_pad take the plane's padding word.
struct GatherPlane { const char* src; char* dst; int row_bytes; unsigned pad; };
struct GatherPlanes { GatherPlane p[4]; };

// G's planes from the rows rows[0 .. n) of the source bank's: blockIdx.y = plane, one thread per unit, grid-stride.
__global__ __launch_bounds__(256)
void mutual_gather_kernel(const int32_t* __restrict__ rows, int64_t n, int64_t n_pad, GatherPlanes g)
{
    const GatherPlane pl = g.p[blockIdx.y];
    const int64_t stride = (int64_t)gridDim.x * 256;
    if (pl.row_bytes >= 16) {
        const int upr = pl.row_bytes >> 4;
        for (int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x; u < n_pad * upr; u += stride) {
            const int64_t slot = u / upr;
            const int k = (int)(u - slot * upr);
            uint4 w = make_uint4(pl.pad, pl.pad, pl.pad, pl.pad);
            if (slot < n) w = *(const uint4*)(pl.src + (int64_t)rows[slot] * pl.row_bytes + 16 * k);
            *(uint4*)(pl.dst + slot * pl.row_bytes + 16 * k) = w;
        }
    } else {
        for (int64_t slot = (int64_t)blockIdx.x * 256 + threadIdx.x; slot < n_pad; slot += stride)
            ((unsigned*)pl.dst)[slot] = slot < n ? ((const unsigned*)pl.src)[rows[slot]] : pl.pad;
    }
}

int fm::mutual_reverse_device(fm_ctx* ctx, const Bank& t, const int32_t* cand_rows, int64_t n_cand, const fm_bank* q, size_t budget,
                              int32_t** r_idx, float** r_dist)
{
    int64_t chunk = (int64_t)(budget / mutual_row_bytes(t)) / kStageRows * kStageRows;
    chunk = std::max<int64_t>(kStageRows, std::min<int64_t>(chunk, pad128(n_cand)));
    // ws_in: the reverse lists of all candidates | G's planes for one chunk (padding rows as each route's sweeps expect them:
    // zero rows, norm 0; float32 accumulator init -3.4e38)
    const float pad_aux = -3.4e38f;
    unsigned pad_aux_bits;
    memcpy(&pad_aux_bits, &pad_aux, 4);
    const size_t rb[4][4] = {{(size_t)kDim, 4, 0, 0}, {(size_t)kDim * 4, (size_t)kDim * 2, 4, 4}, {(size_t)t.ksteps * 16, (size_t)fp4_steps(t) * 64, 0, 0},
                             {(size_t)kWideDim * 4, (size_t)kWideDim * 2, 4, 4}};
    const int route = t.kind == FM_BANK_F32 ? 1 : (t.kind == FM_BANK_BIN || t.kind == FM_BANK_BIN2) ? 2 : t.kind == FM_BANK_F32W ? 3 : 0;
    const void* src[4][4] = {{t.rows8, t.norm, nullptr, nullptr}, {t.rowsf, t.rowsh, t.normf, t.auxf}, {t.rowsb, t.rows4, nullptr, nullptr},
                             {t.wrows, t.wrowsh, t.normf, t.auxf}};
    size_t off = 0, o_pl[4] = {0, 0, 0, 0};
    const size_t o_ri = carve(off, (size_t)n_cand * 8), o_rd = carve(off, (size_t)n_cand * 8);
    int npl = 0;
    for (; npl < 4 && rb[route][npl]; ++npl) o_pl[npl] = carve(off, (size_t)chunk * rb[route][npl]);
    int rc;
    if ((rc = ws_ensure(ctx, &ctx->ws_in, &ctx->ws_in_bytes, off + 64)) != FM_OK) return rc;
    char* b = (char*)ctx->ws_in;
    *r_idx = (int32_t*)(b + o_ri);
    *r_dist = (float*)(b + o_rd);
    GatherPlanes gp{};
    for (int i = 0; i < npl; ++i) gp.p[i] = GatherPlane{(const char*)src[route][i], b + o_pl[i], (int)rb[route][i], 0u};
    if (route == 1 || route == 3) gp.p[3].pad = pad_aux_bits;
    fm_bank g;
    static_cast<Bank&>(g) = bank_rows_view(t, 0, 0);      // kind, width and the scale terms: upper bounds for any subset of t's rows
    g.rows8 = nullptr; g.norm = nullptr; g.aux = nullptr; g.rowsf = nullptr; g.rowsh = nullptr; g.normf = nullptr; g.auxf = nullptr;
    g.rowsb = nullptr; g.rows4 = nullptr; g.wrows = nullptr; g.wrowsh = nullptr;
    if (route == 0) { g.rows8 = (int8_t*)gp.p[0].dst; g.norm = (int32_t*)gp.p[1].dst; }
    else if (route == 1) { g.rowsf = (float*)gp.p[0].dst; g.rowsh = (uint16_t*)gp.p[1].dst; g.normf = (float*)gp.p[2].dst; g.auxf = (float*)gp.p[3].dst; }
    else if (route == 3) { g.wrows = (float*)gp.p[0].dst; g.wrowsh = (uint16_t*)gp.p[1].dst; g.normf = (float*)gp.p[2].dst; g.auxf = (float*)gp.p[3].dst; }
    else { g.rowsb = (uint8_t*)gp.p[0].dst; g.rows4 = (uint8_t*)gp.p[1].dst; }
    for (int64_t c0 = 0; c0 < n_cand; c0 += chunk) {
        g.n = std::min<int64_t>(chunk, n_cand - c0);
        g.n_pad = g.cap_pad = pad128(g.n);
        const int64_t units = g.n_pad * (int64_t)(rb[route][0] >> 4);
        hipLaunchKernelGGL(mutual_gather_kernel, dim3((unsigned)std::min<int64_t>((units + 255) / 256, 16384), (unsigned)npl), dim3(256), 0,
                           ctx->stream, cand_rows + c0, g.n, g.n_pad, gp);
        HIP_TRY(ctx, hipGetLastError());
        if ((rc = knn2_device(ctx, &g, q, *r_idx + 2 * c0, *r_dist + 2 * c0)) != FM_OK) return rc;
    }
    return FM_OK;
}

// Where a pair's accepted rows go: the host arrays (through compacted columns in ws_out) or the caller's device rows.
struct MutualSink {
    int32_t* qidx; int32_t* tidx; float* dist; double* ratio;     // host form
    int32_t* d_rows; int64_t* d_count; void* consumer; bool dev;  // device form
    int64_t* n_accepted;
};

static int mutual_ratio_pair(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, double tau, int symmetric, int64_t cap, const MutualSink& s)
{
    const int64_t nq = q->n;
    const int64_t ccap = s.dev ? 0 : (cap < nq ? cap : nq);
    const int nblk = (int)((nq + 255) / 256);
    size_t off = 0;         // behind the forward lists: the candidates' train rows, the join's flags and counts, the compacted outputs
    const size_t o_cand = carve(off, (size_t)nq * 4, 16), o_p2 = carve(off, (size_t)nq, 16), o_bc2 = carve(off, (size_t)nblk * 4, 16), o_cnt2 = carve(off, 16, 16);
    const size_t o_cq = carve(off, (size_t)ccap * 4, 16), o_ct = carve(off, (size_t)ccap * 4, 16), o_cd = carve(off, (size_t)ccap * 4, 16), o_cr = carve(off, (size_t)ccap * 8, 16);
    CallScope cs(ctx);
    LoweWs w;
    int rc;
    if ((rc = knn2_lowe_device(ctx, q, t, tau, off, &w)) != FM_OK) return rc;
    char* b = w.rest;
    int32_t* d_cand = (int32_t*)(b + o_cand);
    const uint8_t* d_pass = w.pass;
    const int* d_bc = w.bc;
    unsigned long long* d_cnt = w.cnt;
    hipLaunchKernelGGL(mutual_cand_kernel, dim3((unsigned)nblk), dim3(256), 0, ctx->stream, (const int32_t*)w.tidx, (const uint8_t*)w.pass,
                       (const int*)w.bc, nq, nblk, (const int32_t*)nullptr, d_cand, w.cnt);
    HIP_TRY(ctx, hipGetLastError());
    unsigned long long n_cand = 0;      // the call's host wait: how many rows the reverse sweep has to answer for
    HIP_TRY(ctx, hipMemcpyAsync(&n_cand, w.cnt, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (n_cand > 0) {
        int32_t* r_idx; float* r_dist;
        if ((rc = mutual_reverse_device(ctx, *t, d_cand, (int64_t)n_cand, q, kMutualGatherBytes, &r_idx, &r_dist)) != FM_OK) return rc;
        hipLaunchKernelGGL(mutual_join_kernel, dim3((unsigned)nblk), dim3(256), 0, ctx->stream, (const uint8_t*)w.pass, (const int*)w.bc, nq, nblk,
                           (const int32_t*)r_idx, (const float*)r_dist, tau, symmetric, w.ratio, (uint8_t*)(b + o_p2), (int*)(b + o_bc2));
        HIP_TRY(ctx, hipGetLastError());
        d_pass = (const uint8_t*)(b + o_p2); d_bc = (const int*)(b + o_bc2); d_cnt = (unsigned long long*)(b + o_cnt2);
    }
    // (no candidates: the forward flags are all clear, the same compaction writes the zero count)
    if (s.dev) {
        if ((rc = wait_for_stream(ctx, s.consumer)) != FM_OK) return rc;
        hipLaunchKernelGGL(compact_rows_kernel, dim3((unsigned)nblk), dim3(256), 0, ctx->stream, (const int32_t*)w.tidx, (const float*)w.dist,
                           d_pass, d_bc, nq, cap, s.d_rows, (long long*)s.d_count, d_cnt);
        HIP_TRY(ctx, hipGetLastError());
        if ((rc = results_written(ctx, s.consumer)) != FM_OK) return rc;
        if (s.n_accepted) {
            unsigned long long cnt = 0;
            HIP_TRY(ctx, hipMemcpyAsync(&cnt, d_cnt, 8, hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            *s.n_accepted = (int64_t)cnt;
        }
        return FM_OK;
    }
    hipLaunchKernelGGL(compact_kernel, dim3((unsigned)nblk), dim3(256), 0, ctx->stream, (const int32_t*)w.tidx, (const float*)w.dist,
                       (const double*)w.ratio, d_pass, d_bc, nq, ccap, (int32_t*)(b + o_cq), (int32_t*)(b + o_ct), (float*)(b + o_cd),
                       (double*)(b + o_cr), d_cnt);
    HIP_TRY(ctx, hipGetLastError());
    return cs.finish_rows(d_cnt, ccap, {{s.qidx, b + o_cq, 4}, {s.tidx, b + o_ct, 4}, {s.dist, b + o_cd, 4}, {s.ratio, b + o_cr, 8}}, s.n_accepted);
}

extern "C" int fm_mutual_ratio(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, double tau, int32_t symmetric, int64_t cap,
                               int32_t* qidx, int32_t* tidx, float* dist, double* ratio, int64_t* n_accepted)
{
    int rc = check_pair(ctx, q, t, "fm_mutual_ratio", true, true);
    if (rc != FM_OK) return rc;
    if (n_accepted) *n_accepted = 0;
    if (q->n == 0) return FM_OK;
    if (cap < 0 || (cap > 0 && (!qidx || !tidx || !dist || !ratio))) return fail(ctx, FM_EINVAL, "fm_mutual_ratio: bad output arguments");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const MutualSink s{qidx, tidx, dist, ratio, nullptr, nullptr, FM_NO_STREAM, false, n_accepted};
    return mutual_ratio_pair(ctx, q, t, tau, symmetric, cap, s);
}

extern "C" int fm_mutual_ratio_dev(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, double tau, int32_t symmetric, int64_t cap,
                                   int32_t* d_rows, int64_t* d_count, int64_t* n_accepted, void* consumer_stream)
{
    int rc = check_pair(ctx, q, t, "fm_mutual_ratio_dev", true, true);
    if (rc != FM_OK) return rc;
    if (n_accepted) *n_accepted = 0;
    if (cap < 0 || !d_count || (cap > 0 && !d_rows)) return fail(ctx, FM_EINVAL, "fm_mutual_ratio_dev: bad output arguments");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((rc = check_device_ptr(ctx, d_count, "fm_mutual_ratio_dev", "d_count")) != FM_OK) return rc;
    if (cap > 0 && (rc = check_device_ptr(ctx, d_rows, "fm_mutual_ratio_dev", "d_rows")) != FM_OK) return rc;
    if (q->n == 0) {
        if ((rc = wait_for_stream(ctx, consumer_stream)) != FM_OK) return rc;
        HIP_TRY(ctx, hipMemsetAsync(d_count, 0, 8, ctx->stream));
        return results_written(ctx, consumer_stream);
    }
    const MutualSink s{nullptr, nullptr, nullptr, nullptr, d_rows, d_count, consumer_stream, true, n_accepted};
    return mutual_ratio_pair(ctx, q, t, tau, symmetric, cap, s);
}

// Host sink of the accepted calls: the four arrays, the count word, the capacity
static AcceptedSink host_sink(int32_t* qidx, int32_t* tidx, float* dist, double* ratio, int64_t* n_host, int64_t cap)
{
    AcceptedSink s;
    s.qidx = qidx; s.tidx = tidx; s.dist = dist; s.ratio = ratio; s.n_host = n_host; s.cap = cap;
    return s;
}

static AcceptedSink device_sink(int32_t* d_rows, int64_t* d_count, int64_t* n_host, int64_t cap, void* consumer)
{
    AcceptedSink s;
    s.dev_rows = d_rows; s.dev_count = (long long*)d_count; s.n_host = n_host; s.cap = cap; s.consumer = (hipStream_t)consumer;
    return s;
}

// d_rows and d_count are device memory, of any device (fm_match_accepted_dev and its async and batch forms)
static int check_device_rows(fm_ctx* ctx, const void* d_rows, const void* d_count, const char* who)
{
    int rc = check_device_ptr(ctx, d_rows, who, "d_rows", false);
    return rc != FM_OK ? rc : check_device_ptr(ctx, d_count, who, "d_count", false);
}

extern "C" int fm_match_ratio(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, double tau, int32_t* tidx,
                              float* dist, double* ratio, uint8_t* pass, int64_t* n_pass)
{
    return ratio_sync(ctx, q, t, tau, host_sink(nullptr, tidx, dist, ratio, n_pass, -1), pass, "fm_match_ratio");
}

extern "C" int fm_match_accepted(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, double tau, int64_t cap,
                                 int32_t* qidx, int32_t* tidx, float* dist, double* ratio, int64_t* n_accepted)
{
    if (cap < 0) return fail(ctx, FM_EINVAL, "fm_match_accepted: cap < 0");
    return ratio_sync(ctx, q, t, tau, host_sink(qidx, tidx, dist, ratio, n_accepted, cap), nullptr, "fm_match_accepted");
}

extern "C" int fm_match_accepted_async(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, double tau, int64_t cap,
                                       int32_t* qidx, int32_t* tidx, float* dist, double* ratio, int64_t* n_accepted)
{
    if (cap < 0) return fail(ctx, FM_EINVAL, "fm_match_accepted_async: cap < 0");
    if (!n_accepted) return fail(ctx, FM_EINVAL, "fm_match_accepted_async: n_accepted is NULL");
    if (q && q->n == 0) { *n_accepted = 0; }
    return ratio_enqueue(ctx, q, t, tau, host_sink(qidx, tidx, dist, ratio, n_accepted, cap), "fm_match_accepted_async");
}

// n image pairs in one call, enqueued like fm_match_accepted_async; runs of consecutive pairs of one
// shape go through K1 TOGETHER (rowreduce_batch_kernel: up to `batch_group` pairs per launch, at most 16), each
// pair's small kernels follow on one of three tail streams beside the next group's K1.
// d_rows != NULL: device outputs (fm_match_accepted_dev_batch): pair i's rows at d_rows + i * cap * 3, its
// count at d_counts + i, optionally also in the page-locked words h_counts[i]; host outputs otherwise.
static int batch_common(fm_ctx* ctx, int32_t n, const fm_bank* const* q, const fm_bank* const* t, double tau,
                        int64_t cap, int32_t* const* qidx, int32_t* const* tidx, float* const* dist,
                        double* const* ratio, int64_t* const* n_accepted,
                        int32_t* d_rows, int64_t* d_counts, int64_t* h_counts, hipStream_t consumer);

extern "C" int fm_match_accepted_batch(fm_ctx* ctx, int32_t n, const fm_bank* const* q, const fm_bank* const* t, double tau,
                                       int64_t cap, int32_t* const* qidx, int32_t* const* tidx, float* const* dist,
                                       double* const* ratio, int64_t* const* n_accepted)
{
    if (!ctx) return fail(nullptr, FM_EINVAL, "fm_match_accepted_batch: ctx is NULL");
    if (n > 0 && (!qidx || !tidx || !dist || !ratio || !n_accepted)) return fail(ctx, FM_EINVAL, "fm_match_accepted_batch: NULL argument");
    for (int i = 0; i < n; ++i) if (!n_accepted[i]) return fail(ctx, FM_EINVAL, "fm_match_accepted_batch: n_accepted is NULL");
    return batch_common(ctx, n, q, t, tau, cap, qidx, tidx, dist, ratio, n_accepted, nullptr, nullptr, nullptr, kNoStream);
}

extern "C" int fm_match_accepted_dev_batch(fm_ctx* ctx, int32_t n, const fm_bank* const* q, const fm_bank* const* t, double tau,
                                           int64_t cap, int32_t* d_rows, int64_t* d_counts, int64_t* h_counts, void* consumer_stream)
{
    if (!ctx) return fail(nullptr, FM_EINVAL, "fm_match_accepted_dev_batch: ctx is NULL");
    for (int i = 0; q && t && i < n; ++i)
        if (q[i] && t[i] && (bin_or_wide(q[i]) || bin_or_wide(t[i]))) return check_pair(ctx, q[i], t[i], "fm_match_accepted_dev_batch");
    if (n > 0) {
        if (!d_rows || !d_counts) return fail(ctx, FM_EINVAL, "fm_match_accepted_dev_batch: device output pointer is NULL");
        if (int rc = check_device_rows(ctx, d_rows, d_counts, "fm_match_accepted_dev_batch")) return rc;
        if (h_counts && !pinned_device_alias(h_counts)) return fail(ctx, FM_EINVAL, "fm_match_accepted_dev_batch: h_counts must be page-locked (fm_host_alloc)");
    }
    return batch_common(ctx, n, q, t, tau, cap, nullptr, nullptr, nullptr, nullptr, nullptr, d_rows, d_counts, h_counts,
                        (hipStream_t)consumer_stream);
}

static int batch_common(fm_ctx* ctx, int32_t n, const fm_bank* const* q, const fm_bank* const* t, double tau,
                        int64_t cap, int32_t* const* qidx, int32_t* const* tidx, float* const* dist,
                        double* const* ratio, int64_t* const* n_accepted,
                        int32_t* d_rows, int64_t* d_counts, int64_t* h_counts, hipStream_t consumer)
{
    const bool to_dev = d_rows != nullptr;
    // pair k's sink (the consumer stream is fanned in and out around the whole batch, below)
    auto sink_of = [&](int k) {
        return to_dev ? device_sink(d_rows + (size_t)k * cap * 3, d_counts + k, h_counts ? h_counts + k : nullptr, cap, FM_NO_STREAM)
                      : host_sink(qidx[k], tidx[k], dist[k], ratio[k], n_accepted[k], cap);
    };
    if (n < 0 || cap < 0) return fail(ctx, FM_EINVAL, "fm_match_accepted_batch: n < 0 or cap < 0");
    if (n == 0) return FM_OK;
    if (!q || !t) return fail(ctx, FM_EINVAL, "fm_match_accepted_batch: NULL argument");
    int rc;
    // every pair is checked BEFORE anything is enqueued: a bad pair in the middle must not leave earlier pairs
    // in flight and outputs half written
    for (int i = 0; i < n; ++i) {
        if ((rc = check_pair(ctx, q[i], t[i], "fm_match_accepted_batch")) != FM_OK) return rc;
        if (q[i]->n > 0 && !q[i]->selfdist)
            return fail(ctx, FM_EINVAL, "fm_match_accepted_batch: a query bank has no self distances (fm_bank_set_selfdist)");
        if (!to_dev && q[i]->n > 0) {
            if (!qidx[i] || !tidx[i] || !dist[i] || !ratio[i]) return fail(ctx, FM_EINVAL, "fm_match_accepted_batch: output pointer is NULL");
            if (!pinned_device_alias(qidx[i]) || !pinned_device_alias(tidx[i]) || !pinned_device_alias(dist[i]) ||
                !pinned_device_alias(ratio[i]) || !pinned_device_alias(n_accepted[i]))
                return fail(ctx, FM_EINVAL, "fm_match_accepted_batch: host outputs must be page-locked (fm_host_alloc)");
        }
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (to_dev && consumer != kNoStream) {
        // the compactions write buffers the consumer stream reads (the previous step's collective): they wait
        // for what that stream has been given so far
        HIP_TRY(ctx, hipEventRecord(ctx->ev_consumer, consumer));
        for (hipStream_t ts : ctx->tails) HIP_TRY(ctx, hipStreamWaitEvent(ts, ctx->ev_consumer, 0));
    }
    // options batch_group: most pairs per launch (default 8); batch_tail: size of the short launch a run ends
    // with (default 2; 0 = none, for callers that enqueue the next batch before they wait for this one:
    // the small kernels of the last launch then overlap the next batch, see fm_mark / fm_wait)
    const int group_max = ctx->tune.batch_group, tail_n = ctx->tune.batch_tail;
    auto batchable = [&](int i) {
        return q[i]->kind != FM_BANK_F32 && q[i]->n > 0 && t[i]->n > 0 && q[i]->selfdist != nullptr;
    };
    static_assert(fm_ctx::kBatchSlots >= 2 * kRRBatchMax, "two full launches must find distinct workspaces");
    if ((int)ctx->bslot.size() < fm_ctx::kBatchSlots) ctx->bslot.resize((size_t)fm_ctx::kBatchSlots);
    int i = 0;
    while (i < n) {
        // run of same-shape pairs from i on, then this launch's share of it: a launch's small kernels overlap
        // the NEXT launch, so only the last launch's are exposed -- the run ends with a short launch (2 pairs)
        // (r05, last: the pairs of a run need not share their padded sizes any more -- every pair brings its own plan, the
        // launch its own block ranges -- only the kernel shape: 4 blocks per wave, 8 waves, three stage buffers)
        // (a SMALL pair -- train bank below 32768 rows -- is planned with 4-wave workgroups when it runs alone, to fill the chip;
        // in a batched launch the other pairs do that, so it is planned again in the batched kernel's shape: 64 pairs of
        // ~12.5k x 12.5k rows 79 -> 44 us per pair, ~3k x 3k 49 -> 28, scripts/gpu_small_pairs.py)
        auto plan_fits = [&](int k, RowReducePlan* out) {
            if (ctx->tune.glds == 0) return false;
            RowReducePlan p = plan_rowreduce(t[k]->n_pad, q[k]->n_pad, ctx->tune);
            if (!(p.nb == 4 && p.nw == 8 && p.nbuf != 2) && ctx->tune.nb == 0 && ctx->tune.nw == 0) {
                Tuning shaped = ctx->tune;
                shaped.nb = 4; shaped.nw = 8;
                p = plan_rowreduce(t[k]->n_pad, q[k]->n_pad, shaped);
            }
            if (out) *out = p;
            return p.nb == 4 && p.nw == 8 && p.nbuf != 2;
        };
        int run = 1;
        if (batchable(i) && plan_fits(i, nullptr))
            while (i + run < n && batchable(i + run) && plan_fits(i + run, nullptr)) ++run;
        int g = run;
        if (run > group_max + tail_n) g = group_max;
        else if (run > 4 && tail_n > 0) g = run - tail_n < group_max ? run - tail_n : group_max;
        if (g > group_max) g = group_max;
        if (g < 1) g = 1;
        RowReducePlan pls[kRRBatchMax];
        for (int j = 0; j < g && g > 1; ++j) (void)plan_fits(i + j, &pls[j]);
        if (g == 1) {                  // an odd pair: the single-pair call (which also reports its errors)
            // float32-route pairs have no enqueue-only form: they run synchronously, in place (their outputs
            // are complete when the batch call returns; the pairs around them stay asynchronous)
            const bool in_place = q[i]->kind == FM_BANK_F32 && q[i]->n > 0;
            const char* who = to_dev ? "fm_match_accepted_dev_batch" : "fm_match_accepted_batch";
            const AcceptedSink out = sink_of(i);
            if (to_dev && q[i]->n == 0) {
                HIP_TRY(ctx, hipMemsetAsync(d_counts + i, 0, 8, ctx->stream_tail));
                if (out.n_host) *out.n_host = 0;
            } else {
                rc = in_place ? ratio_sync(ctx, q[i], t[i], tau, out, nullptr, who) : ratio_enqueue(ctx, q[i], t[i], tau, out, who);
                if (rc != FM_OK) return rc;
            }
            ++i;
            continue;
        }
        AcceptedSink al[kRRBatchMax];
        int slot_of[kRRBatchMax];
        SlotLayout L[kRRBatchMax];
        const Bank* cols[kRRBatchMax]; const Bank* red[kRRBatchMax];
        unsigned long long* part[kRRBatchMax]; int* bnd[kRRBatchMax];
        fm_ctx::PendingTimer tm;
        if ((rc = take_timer(ctx, &tm)) != FM_OK) return rc;
        tm.timed = true; tm.call_timed = true; tm.pairs = 0; tm.bytes = 0;
        for (int j = 0; j < g; ++j) {
            const int k = i + j;
            al[j] = sink_of(k).aliased();
            if (!al[j].writable()) { ctx->timer_pool.push_back(tm); return fail(ctx, FM_EINVAL, "fm_match_accepted_batch: host outputs must be page-locked (fm_host_alloc)"); }
            if (al[j].n_host) *al[j].n_host = 0;
            slot_of[j] = (int)(ctx->bslot_next++ % fm_ctx::kBatchSlots);
            fm_ctx::AsyncSlot& sl = ctx->bslot[(size_t)slot_of[j]];
            if (!sl.tail_done) HIP_TRY(ctx, hipEventCreateWithFlags(&sl.tail_done, hipEventDisableTiming));
            const RowReducePlan& pl = pls[j];
            const bool coop = (ctx->tune.coop != 0) && pl.nsplit > 1;
            L[j] = slot_layout(q[k]->n, t[k]->n, pl);
            if ((rc = slot_prepare(ctx, sl, L[j], q[k]->n, pl, ctx->stream)) != FM_OK) { ctx->timer_pool.push_back(tm); return rc; }
            cols[j] = t[k]; red[j] = q[k];            // reverse NN: output rows = train rows, reduced over the query rows
            part[j] = (unsigned long long*)sl.ws;
            bnd[j] = coop ? (int*)((char*)sl.ws + L[j].pbytes) : nullptr;
            tm.pairs += q[k]->n * t[k]->n;
            tm.bytes += bank_bytes(q[k]) + bank_bytes(t[k]);
        }
        const unsigned* cut[kRRBatchMax];
        if ((rc = enqueue_ratio_cut(ctx, g, q + i, tau, cut)) != FM_OK) { ctx->timer_pool.push_back(tm); return rc; }
        HIP_TRY(ctx, hipEventRecord(tm.k0, ctx->stream));
        // The filter's rescoring and its guarded K1 go to the last tail stream, beside the next launch's sweep; the pairs'
        // tails then follow the guard's event.  tm.k1 stays on the sweep's stream: with the filter, k0 .. k1 is the sweep alone.
        const Filter6Ws* f6 = filter6_ws(ctx, g);
        const int set = ctx->f6_set;
        if (f6) { ctx->f6.side = ctx->tails[fm_ctx::kTails - 1];  ctx->f6.ev_sweep = ctx->ev_f6_sweep[set];  ctx->f6.ev_done = ctx->ev_f6_done[set]; }
        bool moved = false;
        HIP_TRY(ctx, launch_rowreduce_batch(g, cols, red, pls, part, bnd, ctx->stream, false, cut, f6, &moved));
        HIP_TRY(ctx, hipEventRecord(tm.k1, ctx->stream));
        if (moved) ctx->f6_off_stream[set] = true;
        hipEvent_t handover = moved ? ctx->ev_f6_done[set] : tm.k1;
        for (int j = 0; j < g; ++j) {
            const int k = i + j;
            hipStream_t ts = ctx->tails[j % fm_ctx::kTails];
            fm_ctx::AsyncSlot& sl = ctx->bslot[(size_t)slot_of[j]];
            HIP_TRY(ctx, hipStreamWaitEvent(ts, handover, 0));
            if ((rc = enqueue_tail(ctx, ts, sl, L[j], q[k], t[k], pls[j], tau, al[j])) != FM_OK) { ctx->pending.push_back(tm); return rc; }     // (events are in flight: drained at fm_sync)
            HIP_TRY(ctx, hipEventRecord(sl.tail_done, ts));
            sl.in_use = true;
            if (j == g - 1) HIP_TRY(ctx, hipEventRecord(tm.c1, ts));
        }
        ctx->pending.push_back(tm);
        i += g;
    }
    if (to_dev) {
        // everything the tails were given is in front of these records: the consumer waits for all of it
        // (without a consumer stream the first tail stream collects the others: fm_gather_matches follows it)
        for (int u = 0; u < fm_ctx::kTails; ++u) {
            hipStream_t ts = ctx->tails[u];
            HIP_TRY(ctx, hipEventRecord(ctx->ev_tail_end[u], ts));
            if (consumer != kNoStream) HIP_TRY(ctx, hipStreamWaitEvent(consumer, ctx->ev_tail_end[u], 0));
            else if (ts != ctx->stream_tail) HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream_tail, ctx->ev_tail_end[u], 0));
        }
        ctx->rows_stream = ctx->stream_tail;
    }
    return FM_OK;
}

extern "C" int fm_match_accepted_dev(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, double tau, int64_t cap,
                                     int32_t* d_rows, int64_t* d_count, int64_t* n_accepted)
{
    if (!ctx) return fail(nullptr, FM_EINVAL, "fm_match_accepted_dev: ctx is NULL");
    if (q && t && (bin_or_wide(q) || bin_or_wide(t))) return check_pair(ctx, q, t, "fm_match_accepted_dev");
    if (cap < 0) return fail(ctx, FM_EINVAL, "fm_match_accepted_dev: cap < 0");
    if (!d_rows || !d_count) return fail(ctx, FM_EINVAL, "fm_match_accepted_dev: device output pointer is NULL");
    if (int rc = check_device_rows(ctx, d_rows, d_count, "fm_match_accepted_dev")) return rc;
    if (q && q->n == 0) HIP_TRY(ctx, hipMemset(d_count, 0, 8));
    return ratio_sync(ctx, q, t, tau, device_sink(d_rows, d_count, n_accepted, cap, FM_NO_STREAM), nullptr, "fm_match_accepted_dev");
}

// ---- Hamming and wide Fast-Match: the accepted-match test on binary / wide float banks (the header's sections of those names) -
// Steps 1 .. 4 of the documented error order; the entry points add cap and the NULL outputs, then ratio_sync runs the pair with
// the family's reverse top-1 sweep (sweep_pair's binary route: K11; its wide route: K14 with float32-bit keys), the generic
// election and tail, and no ratio cut (an int8-route device).
static int named_pair_check(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, const NamedFamily& f, const char* who, const char* l2,
                            const char* ham = nullptr)
{
    if (!ctx) return fail(nullptr, FM_EINVAL, std::string(who) + ": ctx is NULL");
    if (!q || !t) return fail(ctx, FM_EINVAL, std::string(who) + ": bank is NULL");
    for (const fm_bank* b : {q, t})
        if (int rc = refuse_bin2(ctx, b, who)) return rc;
    if (q->kind != f.kind || t->kind != f.kind)
        return fail(ctx, FM_EINVAL, std::string(who) + ": " + f.both + "; " + named_served_by(q->kind != f.kind ? q : t, l2, ham));
    if (q->dim != t->dim) return fail(ctx, FM_EINVAL, std::string(who) + ": query/train width mismatch");
    if (q->n > 0 && !q->selfdist)
        return fail(ctx, FM_EINVAL, std::string(who) + ": query bank has no self distances (" + f.attach + ")");
    return FM_OK;
}

static int named_match_accepted_dev(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, double tau, int64_t cap, int32_t* d_rows, int64_t* d_count,
                                    int64_t* n_accepted, const NamedFamily& f, const char* who_, const char* l2, const char* ham = nullptr)
{
    const std::string who(who_);
    if (int rc = named_pair_check(ctx, q, t, f, who_, l2, ham)) return rc;
    if (cap < 0) return fail(ctx, FM_EINVAL, who + ": cap < 0");
    if (!d_rows || !d_count) return fail(ctx, FM_EINVAL, who + ": device output pointer is NULL");
    if (int rc = check_device_rows(ctx, d_rows, d_count, who_)) return rc;
    if (q->n == 0) HIP_TRY(ctx, hipMemset(d_count, 0, 8));
    return ratio_sync(ctx, q, t, tau, device_sink(d_rows, d_count, n_accepted, cap, FM_NO_STREAM), nullptr, who_, true);
}

extern "C" int fm_hamming_match_ratio(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, double tau, int32_t* tidx,
                                      float* dist, double* ratio, uint8_t* pass, int64_t* n_pass)
{
    if (int rc = named_pair_check(ctx, q, t, kHamFamily, "fm_hamming_match_ratio", "fm_match_ratio")) return rc;
    return ratio_sync(ctx, q, t, tau, host_sink(nullptr, tidx, dist, ratio, n_pass, -1), pass, "fm_hamming_match_ratio", true);
}

extern "C" int fm_hamming_match_accepted(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, double tau, int64_t cap,
                                         int32_t* qidx, int32_t* tidx, float* dist, double* ratio, int64_t* n_accepted)
{
    if (int rc = named_pair_check(ctx, q, t, kHamFamily, "fm_hamming_match_accepted", "fm_match_accepted")) return rc;
    if (cap < 0) return fail(ctx, FM_EINVAL, "fm_hamming_match_accepted: cap < 0");
    return ratio_sync(ctx, q, t, tau, host_sink(qidx, tidx, dist, ratio, n_accepted, cap), nullptr, "fm_hamming_match_accepted", true);
}

extern "C" int fm_hamming_match_accepted_dev(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, double tau, int64_t cap,
                                             int32_t* d_rows, int64_t* d_count, int64_t* n_accepted)
{
    return named_match_accepted_dev(ctx, q, t, tau, cap, d_rows, d_count, n_accepted, kHamFamily, "fm_hamming_match_accepted_dev",
                                    "fm_match_accepted_dev");
}

extern "C" int fm_wide_match_ratio(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, double tau, int32_t* tidx,
                                   float* dist, double* ratio, uint8_t* pass, int64_t* n_pass)
{
    if (int rc = named_pair_check(ctx, q, t, kWideFamily, "fm_wide_match_ratio", "fm_match_ratio", "fm_hamming_match_ratio")) return rc;
    return ratio_sync(ctx, q, t, tau, host_sink(nullptr, tidx, dist, ratio, n_pass, -1), pass, "fm_wide_match_ratio", true);
}

extern "C" int fm_wide_match_accepted(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, double tau, int64_t cap,
                                      int32_t* qidx, int32_t* tidx, float* dist, double* ratio, int64_t* n_accepted)
{
    if (int rc = named_pair_check(ctx, q, t, kWideFamily, "fm_wide_match_accepted", "fm_match_accepted", "fm_hamming_match_accepted")) return rc;
    if (cap < 0) return fail(ctx, FM_EINVAL, "fm_wide_match_accepted: cap < 0");
    return ratio_sync(ctx, q, t, tau, host_sink(qidx, tidx, dist, ratio, n_accepted, cap), nullptr, "fm_wide_match_accepted", true);
}

extern "C" int fm_wide_match_accepted_dev(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, double tau, int64_t cap,
                                          int32_t* d_rows, int64_t* d_count, int64_t* n_accepted)
{
    return named_match_accepted_dev(ctx, q, t, tau, cap, d_rows, d_count, n_accepted, kWideFamily, "fm_wide_match_accepted_dev",
                                    "fm_match_accepted_dev", "fm_hamming_match_accepted_dev");
}

extern "C" int fm_match_accepted_dev_async(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, double tau, int64_t cap,
                                           int32_t* d_rows, int64_t* d_count, int64_t* h_count, void* consumer_stream)
{
    if (!ctx) return fail(nullptr, FM_EINVAL, "fm_match_accepted_dev_async: ctx is NULL");
    if (q && t && (bin_or_wide(q) || bin_or_wide(t))) return check_pair(ctx, q, t, "fm_match_accepted_dev_async");
    if (cap < 0) return fail(ctx, FM_EINVAL, "fm_match_accepted_dev_async: cap < 0");
    if (!d_rows || !d_count) return fail(ctx, FM_EINVAL, "fm_match_accepted_dev_async: device output pointer is NULL");
    if (int rc = check_device_rows(ctx, d_rows, d_count, "fm_match_accepted_dev_async")) return rc;
    if (q && q->n == 0) {
        HIP_TRY(ctx, hipMemsetAsync(d_count, 0, 8, ctx->stream_tail));
        if (h_count) *h_count = 0;
        if (consumer_stream != FM_NO_STREAM) {
            HIP_TRY(ctx, hipEventRecord(ctx->ev_consumer, ctx->stream_tail));
            HIP_TRY(ctx, hipStreamWaitEvent((hipStream_t)consumer_stream, ctx->ev_consumer, 0));
        }
        ctx->rows_stream = ctx->stream_tail;
    }
    return ratio_enqueue(ctx, q, t, tau, device_sink(d_rows, d_count, h_count, cap, consumer_stream), "fm_match_accepted_dev_async");
}

extern "C" int fm_ratio_filter(fm_ctx* ctx, const float* dist, const double* selfdist, const int32_t* qrows,
                               int64_t n, double tau, double* ratio, uint8_t* pass, int64_t* n_pass)
{
    if (!ctx) return fail(nullptr, FM_EINVAL, "fm_ratio_filter: ctx is NULL");
    if (n_pass) *n_pass = 0;
    if (n < 0) return fail(ctx, FM_EINVAL, "fm_ratio_filter: n < 0");
    if (n == 0) return FM_OK;
    if (!dist || !selfdist) return fail(ctx, FM_EINVAL, "fm_ratio_filter: NULL input");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // selfdist is indexed by qrows (or by i): upload max(qrows)+1 entries
    int64_t nsd = n;
    if (qrows) { nsd = 0; for (int64_t i = 0; i < n; ++i) { if (qrows[i] < 0) return fail(ctx, FM_EINVAL, "fm_ratio_filter: negative qrow"); if (qrows[i] + 1 > nsd) nsd = qrows[i] + 1; } }
    const size_t i_dist = 0, i_sd = ((size_t)n * 4 + 7) & ~(size_t)7, i_qr = i_sd + (size_t)nsd * 8;
    const size_t in_bytes = i_qr + (qrows ? (size_t)n * 4 : 0);
    int rc;
    if ((rc = ws_ensure(ctx, &ctx->ws_in, &ctx->ws_in_bytes, in_bytes + 16)) != FM_OK) return rc;
    const size_t o_ratio = 0, o_pass = (size_t)n * 8, o_cnt = (o_pass + (size_t)n + 15) & ~(size_t)15;
    if ((rc = ws_ensure(ctx, &ctx->ws_out, &ctx->ws_out_bytes, o_cnt + 16)) != FM_OK) return rc;
    char* ib = (char*)ctx->ws_in;
    char* ob = (char*)ctx->ws_out;
    CallScope cs(ctx);
    HIP_TRY(ctx, hipMemcpyAsync(ib + i_dist, dist, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ib + i_sd, selfdist, (size_t)nsd * 8, hipMemcpyHostToDevice, ctx->stream));
    if (qrows) HIP_TRY(ctx, hipMemcpyAsync(ib + i_qr, qrows, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(ob + o_cnt, 0, 8, ctx->stream));
    hipLaunchKernelGGL(ratio_filter_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream,
                       (const float*)(ib + i_dist), (const double*)(ib + i_sd),
                       qrows ? (const int32_t*)(ib + i_qr) : (const int32_t*)nullptr, n, tau,
                       (double*)(ob + o_ratio), (uint8_t*)(ob + o_pass), (unsigned long long*)(ob + o_cnt));
    HIP_TRY(ctx, hipGetLastError());
    unsigned long long cnt = 0;
    if (ratio) HIP_TRY(ctx, d2h(ctx, ratio, ob + o_ratio, (size_t)n * 8));
    if (pass) HIP_TRY(ctx, d2h(ctx, pass, ob + o_pass, (size_t)n));
    HIP_TRY(ctx, hipMemcpyAsync(&cnt, ob + o_cnt, 8, hipMemcpyDeviceToHost, ctx->stream));
    rc = cs.finish();
    if (rc != FM_OK) return rc;
    if (n_pass) *n_pass = (int64_t)cnt;
    return FM_OK;
}

// Planes and scale terms of a (query = reduced, train = output rows) pair of float32 banks for
// x1_round_f32: the same margin / accumulator-init factors launch_filter (filter_f16.hip) uses.
void fm::fill_round_f32(RoundF32* r, const Bank& q, const Bank& t)
{
    const float eps = 1.1f / 1024.0f;
    const int dk = t.kscale - q.kscale;               // acc units are 2^(kt + kq)
    r->q_rowsh = (const char*)q.rowsh; r->q_auxf = q.auxf; r->q_rowsf = q.rowsf;
    r->t_rowsh = (const char*)t.rowsh; r->t_normf = t.normf; r->t_rowsf = t.rowsf;
    r->eps_c = ldexpf(eps, -dk);
    r->eps_nm = ldexpf(eps * q.nm_max, dk);
    r->aux_mul = ldexpf(1.0f, dk);
}

extern "C" int fm_xcheck1_batched(fm_ctx* ctx, const fm_bank* q, const int32_t* q_rows, const int64_t* q_off,
                                  const fm_bank* t, const int64_t* t_off, int64_t n_rounds,
                                  int32_t* tidx, float* dist, double* ratio)
{
    int rc = check_pair(ctx, q, t, "fm_xcheck1_batched");
    if (rc != FM_OK) return rc;
    const bool f32 = q->kind == FM_BANK_F32;
    if (f32 && !filter_usable(*t, *q))
        return fail(ctx, FM_EUNSUPPORTED, "fm_xcheck1_batched: float32 banks without usable fp16 filter planes take the dense path (fm_xcheck1 / fm_match_ratio)");
    if (n_rounds < 0) return fail(ctx, FM_EINVAL, "fm_xcheck1_batched: n_rounds < 0");
    if (n_rounds == 0) return FM_OK;
    if (!q_off || !t_off) return fail(ctx, FM_EINVAL, "fm_xcheck1_batched: NULL offsets");
    if (q_off[0] != 0) return fail(ctx, FM_EINVAL, "fm_xcheck1_batched: q_off[0] must be 0");
    int64_t pairs = 0, rows_read = 0;
    for (int64_t b = 0; b < n_rounds; ++b) {
        const int64_t nq = q_off[b + 1] - q_off[b], nt = t_off[b + 1] - t_off[b];
        if (nq < 0 || nt < 0 || t_off[b] < 0 || t_off[b + 1] > t->n)
            return fail(ctx, FM_EINVAL, "fm_xcheck1_batched: bad round offsets");
        if (nq > round_qcap())
            return fail(ctx, FM_EUNSUPPORTED, "fm_xcheck1_batched: a round has more than 4096 query rows; use fm_xcheck1 on gathered banks");
        pairs += nq * nt;
        rows_read += nq + nt;
    }
    const int64_t tot = q_off[n_rounds];
    if (tot == 0) return FM_OK;
    if (!q_rows || !tidx || !dist) return fail(ctx, FM_EINVAL, "fm_xcheck1_batched: NULL rows/outputs");
    for (int64_t i = 0; i < tot; ++i)
        if (q_rows[i] < 0 || q_rows[i] >= q->n) return fail(ctx, FM_EINVAL, "fm_xcheck1_batched: q_rows index out of range");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t i_qoff = 0, i_toff = (size_t)(n_rounds + 1) * 8, i_rows = i_toff + (size_t)(n_rounds + 1) * 8;
    if ((rc = ws_ensure(ctx, &ctx->ws_in, &ctx->ws_in_bytes, i_rows + (size_t)tot * 4 + 16)) != FM_OK) return rc;
    const size_t o_tidx = 0, o_dist = (size_t)tot * 4, o_ratio = ((size_t)tot * 8 + 7) & ~(size_t)7;
    if ((rc = ws_ensure(ctx, &ctx->ws_out, &ctx->ws_out_bytes, o_ratio + (size_t)tot * 8 + 16)) != FM_OK) return rc;
    char* ib = (char*)ctx->ws_in;
    char* ob = (char*)ctx->ws_out;
    CallScope cs(ctx);
    HIP_TRY(ctx, hipMemcpyAsync(ib + i_qoff, q_off, (size_t)(n_rounds + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ib + i_toff, t_off, (size_t)(n_rounds + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ib + i_rows, q_rows, (size_t)tot * 4, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipEventRecord(ctx->ev_k0, ctx->stream));
    if (f32) {
        RoundF32 rf;
        fill_round_f32(&rf, *q, *t);
        HIP_TRY(ctx, launch_rounds_f32(rf, q->selfdist, (const int32_t*)(ib + i_rows), (const int64_t*)(ib + i_qoff),
                                       (const int64_t*)(ib + i_toff), n_rounds, (int32_t*)(ob + o_tidx),
                                       (float*)(ob + o_dist), (double*)(ob + o_ratio), ctx->stream));
    } else {
        HIP_TRY(ctx, launch_rounds(*q, *t, (const int32_t*)(ib + i_rows), (const int64_t*)(ib + i_qoff),
                                   (const int64_t*)(ib + i_toff), n_rounds, (int32_t*)(ob + o_tidx),
                                   (float*)(ob + o_dist), (double*)(ob + o_ratio), ctx->stream));
    }
    HIP_TRY(ctx, hipEventRecord(ctx->ev_k1, ctx->stream));
    ctx->kernel_timed = true;
    ctx->pending_pairs += pairs;
    ctx->pending_bytes += rows_read * (f32 ? 512 : 128);
    HIP_TRY(ctx, d2h(ctx, tidx, ob + o_tidx, (size_t)tot * 4));
    HIP_TRY(ctx, d2h(ctx, dist, ob + o_dist, (size_t)tot * 4));
    if (ratio) HIP_TRY(ctx, d2h(ctx, ratio, ob + o_ratio, (size_t)tot * 8));
    return cs.finish();
}
