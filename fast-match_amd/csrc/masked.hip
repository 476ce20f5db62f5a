// K13 -- knnMatch under a mask: cv2.BFMatcher.knnMatch(q, t, k, mask) / knnMatch(q, k, masks=[...]).  Row i's list is
// fm_knn's list computed over the train rows the mask permits for row i only: the same distance bits, ascending by
// (float32 bits of the distance, train row), strictly; -1 / +inf where fewer than k rows are permitted.
//
//   the mask              a device-resident bit matrix [nq][n_pad / 64] of 64-bit words over the PADDED rows of the train
//                         operand (fm_mask, ctx_internal.h): bit b of word w of row i = (query row i, train row 64 w + b) is
//                         permitted.  The bits of padding rows are 0, always: mask_pack_kernel and mask_fill_kernel clear
//                         every bit at or beyond an image's real rows.  A collection's mask lies on the physical stack --
//                         an image starts on a 128-row stage, so its bits are whole words (two per stage) and setting one
//                         image touches no other image's words -- and the padding behind EVERY image is forbidden by the
//                         mask itself: the masked kernels need no per-stage real-row table (RSweep::st_real, stage_real).
//                         The one padding a mask cannot know: the gap rows INSIDE a train bank that grew by appends (a pair
//                         mask is made from row counts).  The kernels AND the bank's real-row word (Bank::real, the same
//                         word layout, null for every other bank) into the mask word of each stage.
//   mask_pack_kernel      one wave per word: 64 consecutive bytes of a source row (host rows staged in chunks of at most
//                         64 MiB, or the caller's device memory read in place), nonzero = permitted, packed by ballot.
//   masked_i8_kernel<K>   integer route, k = 1 and 2, on the matrix cores: v_mfma_i32_16x16x64_i8 in radius_i8_kernel's
//                         geometry (radius.hip) -- 4 waves, 4 blocks of 16 query rows per wave held in VGPRs for the whole
//                         sweep, the train rows through LDS 64 at a time, grid = (query groups of 256, splits of the train
//                         range).  Lane (j = lane & 15, g = lane >> 4) holds, for tile tt and accumulator register r, train
//                         row base + 16 tt + 4 g + r of query row qw + 16 b + j, so the 16 bits a lane needs per block and
//                         stage are the four nibbles (w >> (16 tt + 4 g)) & 0xF of the ONE word mask[q][base >> 6]: one
//                         8-byte load per (block, stage), issued ahead of the stage's LDS traffic and MFMAs.  A forbidden
//                         candidate never enters the in-lane list.  A wave whose words of a stage are all zero skips the
//                         stage's MFMAs, and so does a (block, tile) without a permitted pair (wave-uniform branches:
//                         guided matching and per-class masks forbid whole ranges of train rows).
//                         Order inside the kernel: (sqrt_bits(d2), row), knnk_i8_kernel's order (knn_k.hip) -- the test
//                         `d2 <= wd2` runs on the exact integer d2, wd2 being the largest d2 whose root can still reach the
//                         list's last entry.  The lists hold the lower member of d2's float32-root class (m_class: below
//                         4 197 200 that is d2 itself and no root is taken), which orders exactly as the root does; the
//                         root is taken once per list entry when the partial keys are written.  That is OpenCV's order
//                         above d2 = 4 197 200 too (two integers share one float32 root there, tile_ops.h) without a
//                         masked twin of sqrt_fix_kernel, whose rescan knows nothing of masks.
//                         The four lanes of a query row (j, j + 16, j + 32, j + 48) merge their lists by shuffles; lane
//                         g = 0 writes partial[(split * nq + q) * K + i] = (distance bits << 32) | row, ~0 = none -- K9's
//                         key format and layout, so knnk_merge_kernel<K> (knn_k.hip) merges the splits and writes [nq][k].
//   everything else       k = 3 .. 8 on the integer route, every k on the float32 route and for binary rows: the exact
//                         vector-ALU kernels of K9 / K11 in their MASKED instantiations (knn_k.hip, hamming.hip): one thread
//                         per query row reads its mask word once per 64-row stage and tests a bit per candidate.  The
//                         float32 ones run K5's chain: the bits are fm_knn2's.  NOT on the matrix cores.
// The option "masked_mfma" = 0 sends the integer route's k <= 2 to the masked K9 kernel as well (measurements, tests).
#include "ctx_internal.h"
#include "tile_ops.h"

#include <algorithm>

namespace fm {

constexpr int kMStage = 64;                 // train rows per LDS stage = one mask word per query row
constexpr int kMNB = 4;                     // blocks of 16 query rows per wave
constexpr int kMWaves = 4;
constexpr int kMQPerWG = 16 * kMNB * kMWaves;
constexpr int kMRowI8 = kDim + 16;          // LDS row pitch (bytes): 16 bytes of padding against bank conflicts
constexpr size_t kMaskChunkBytes = (size_t)64 << 20;    // host rows of fm_mask_set_u8 staged per chunk

// ---- the mask's words ---------------------------------------------------------------------------------------------------
// One wave per (source row r, word w of the image): bits[(q0 + r)][w0 + w] = ballot(src[r][64 w + lane] != 0), columns at or
// beyond the image's real rows 0.  The image has img_words = pad128(img_rows) / 64 words; all of them are written.
__global__ __launch_bounds__(256)
void mask_pack_kernel(const uint8_t* __restrict__ src, int64_t pitch, int64_t nrows, int64_t img_rows, int64_t img_words,
                      unsigned long long* __restrict__ bits, int64_t words, int64_t q0, int64_t w0)
{
    const int lane = threadIdx.x & 63;
    const int64_t wv = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wv >= nrows * img_words) return;                       // (uniform in a wave)
    const int64_t r = wv / img_words, w = wv % img_words;
    const int64_t col = 64 * w + lane;
    const bool on = col < img_rows && src[r * pitch + col] != 0;
    const unsigned long long word = __ballot(on);
    if (lane == 0) bits[(q0 + r) * words + w0 + w] = word;
}

// Every real row of one image permitted (value != 0) or forbidden, for the query rows [q0, q0 + nrows): one thread per word.
__global__ __launch_bounds__(256)
void mask_fill_kernel(unsigned long long* __restrict__ bits, int64_t words, int64_t q0, int64_t nrows, int64_t w0, int64_t img_words,
                      int64_t img_rows, int value)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nrows * img_words) return;
    const int64_t r = q0 + i / img_words, w = i % img_words;
    const int64_t rem = img_rows - 64 * w;
    const unsigned long long word = (!value || rem <= 0) ? 0ull : rem >= 64 ? ~0ull : ((1ull << rem) - 1ull);
    bits[r * words + w0 + w] = word;
}

// ---- the masked MFMA sweep ----------------------------------------------------------------------------------------------
__device__ __forceinline__ void m_top2(unsigned long long& k0, unsigned long long& k1, unsigned long long v)
{
    // (selects, not branches: stores under a branch invite the compiler to pick the destination by address, which puts the
    // lists into scratch memory)
    const bool lt0 = v < k0, lt1 = v < k1;
    k1 = lt0 ? k0 : (lt1 ? v : k1);
    k0 = lt0 ? v : k0;
}

// Two integers d2 share a float32 root only from kSqrtTieMin on, and then only as pairs {n, n + 1} (tile_ops.h).  The in-lane
// lists keep a d2 as the LOWER member of its root class: ordering by (class, row) IS ordering by (sqrt_bits(d2), row) -- the
// root is monotone in d2 -- and below kSqrtTieMin (every SIFT-range pair) it costs one compare and no square root.
__device__ __forceinline__ unsigned m_class(unsigned d2)
{
    return (d2 > kSqrtTieMin && sqrt_ties_up(d2 - 1u)) ? d2 - 1u : d2;
}

// the largest d2 whose root can still reach a list entry of class c: c itself, or c + 1 where that shares c's root
__device__ __forceinline__ unsigned m_wd2(unsigned c)
{
    return (c >= kSqrtTieMin && sqrt_ties_up(c)) ? c + 1u : c;
}

template <int K>
__global__ __launch_bounds__(256)
void masked_i8_kernel(const int8_t* __restrict__ qrows, const int32_t* __restrict__ qnorm, int nq,
                      const int8_t* __restrict__ trows, const int32_t* __restrict__ tnorm, int nt, int per,
                      const unsigned long long* __restrict__ mask, int64_t mwords, unsigned long long* __restrict__ partial,
                      const unsigned long long* __restrict__ real)
{
    __shared__ __attribute__((aligned(16))) int8_t srow[kMStage * kMRowI8];
    __shared__ __attribute__((aligned(16))) int snorm[kMStage];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
    const int qw = blockIdx.x * kMQPerWG + wave * 16 * kMNB;
    v4i bq[kMNB][2];
    int qn[kMNB];
    unsigned long long k0[kMNB], k1[kMNB];
    unsigned wd2[kMNB];                          // a candidate needs d2 <= wd2 (no list entry yet: every d2)
    const unsigned long long* mrow[kMNB];        // the query row's mask words (null: no such row)
#pragma unroll
    for (int b = 0; b < kMNB; ++b) {
        const int q = qw + 16 * b + j;
        const bool live = q < nq;
#pragma unroll
        for (int h = 0; h < 2; ++h)
            bq[b][h] = live ? *(const v4i*)(qrows + (size_t)q * kDim + 64 * h + 16 * g) : v4i{0, 0, 0, 0};
        qn[b] = live ? qnorm[q] : 0;
        mrow[b] = live ? mask + (size_t)q * mwords : nullptr;
        k0[b] = ~0ull; k1[b] = ~0ull;
        wd2[b] = 0xffffffffu;
    }
    const int t0 = blockIdx.y * per, t1 = min(nt, t0 + per);
    for (int base = t0; base < t1; base += kMStage) {
        // the stage's mask words first: one 8-byte load per block, in flight while the stage is copied
        unsigned long long mw[kMNB];
#pragma unroll
        for (int b = 0; b < kMNB; ++b) mw[b] = mrow[b] ? mrow[b][base >> 6] : 0ull;
        if (real) {         // a grown train bank (Bank::real; uniform): the mask cannot know its gap rows -- forbidden here
            const unsigned long long rw = real[base >> 6];
#pragma unroll
            for (int b = 0; b < kMNB; ++b) mw[b] &= rw;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 2; ++i) {       // 64 rows x 8 pieces of 16 B (rows < n_pad: base % 64 == 0, n_pad % 128 == 0)
            const int piece = tid + 256 * i, r = piece >> 3, c = piece & 7;
            *(v4i*)(srow + r * kMRowI8 + 16 * c) = *(const v4i*)(trows + (size_t)(base + r) * kDim + 16 * c);
        }
        if (tid < kMStage) snorm[tid] = tnorm[base + tid];
        __syncthreads();
        // (both barriers of a stage are passed by every wave; what a wave may skip lies between this one and the next stage's)
        if (!__any((mw[0] | mw[1] | mw[2] | mw[3]) != 0ull)) continue;
        v4i a[4][2], tn[4];
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
#pragma unroll
            for (int h = 0; h < 2; ++h) a[tt][h] = *(const v4i*)(srow + (16 * tt + j) * kMRowI8 + 64 * h + 16 * g);
            tn[tt] = *(const v4i*)(snorm + 16 * tt + 4 * g);
        }
#pragma unroll
        for (int b = 0; b < kMNB; ++b) {
            const unsigned long long mine = mw[b] >> (4 * g);       // tile tt's nibble of this lane: bits 16 tt .. 16 tt + 3
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) {
                const unsigned nib = (unsigned)(mine >> (16 * tt)) & 0xFu;
                if (__any(nib != 0u)) {                             // (wave-uniform: the MFMAs run with every lane or not at all)
                    v4i acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[tt][0], bq[b][0], v4i{0, 0, 0, 0}, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[tt][1], bq[b][1], acc, 0, 0, 0);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const unsigned d2 = (unsigned)(qn[b] + tn[tt][r] - 2 * acc[r]);
                        // bit clear: forbidden (or a padding row, or no such query row)
                        if (((nib >> r) & 1u) && d2 <= wd2[b]) {
                            const unsigned long long key = ((unsigned long long)m_class(d2) << 32) | (unsigned)(base + 16 * tt + 4 * g + r);
                            if constexpr (K == 1) {
                                if (key < k0[b]) { k0[b] = key; wd2[b] = m_wd2((unsigned)(key >> 32)); }
                            } else {
                                if (key < k1[b]) {
                                    m_top2(k0[b], k1[b], key);
                                    if (k1[b] != ~0ull) wd2[b] = m_wd2((unsigned)(k1[b] >> 32));
                                }
                            }
                        }
                    }
                }
            }
        }
    }
    // the four lanes of a query row hold disjoint train rows: after two exchanges each of them holds the row's list
#pragma unroll
    for (int b = 0; b < kMNB; ++b) {
        unsigned long long a0 = k0[b], a1 = k1[b];
#pragma unroll
        for (int x = 0; x < 2; ++x) {
            const unsigned long long o0 = __shfl_xor(a0, 16 << x), o1 = __shfl_xor(a1, 16 << x);
            m_top2(a0, a1, o0);
            m_top2(a0, a1, o1);
        }
        const int q = qw + 16 * b + j;
        if (g == 0 && q < nq) {
            // (the root itself only here: the class's root is the root of both of its members)
            unsigned long long* p = partial + ((size_t)blockIdx.y * nq + q) * K;
            p[0] = a0 == ~0ull ? a0 : (((unsigned long long)sqrt_bits((unsigned)(a0 >> 32)) << 32) | (unsigned)a0);
            if constexpr (K == 2) p[1] = a1 == ~0ull ? a1 : (((unsigned long long)sqrt_bits((unsigned)(a1 >> 32)) << 32) | (unsigned)a1);
        }
    }
}

static int m_splits(int64_t nq, int64_t nt)
{
    // ~2048 workgroups on the chip, a split of at least 1024 train rows (K10's rule)
    const int64_t qg = (nq + kMQPerWG - 1) / kMQPerWG;
    int64_t s = (2048 + qg - 1) / qg;
    if (s > (nt + 1023) / 1024) s = (nt + 1023) / 1024;
    if (s < 1) s = 1;
    if (s > 65535) s = 65535;
    return (int)s;
}

size_t masked_i8_partial_bytes(int64_t nq, int64_t nt, int k) { return (size_t)m_splits(nq, nt) * (size_t)nq * (size_t)k * 8; }

hipError_t launch_masked_i8(const Bank& q, const Bank& t, int k, const unsigned long long* mask, int64_t mwords,
                            unsigned long long* partial, int32_t* d_idx, float* d_dist, hipStream_t stream)
{
    if (k < 1 || k > 2 || q.kind != FM_BANK_I8 || t.kind != FM_BANK_I8 || q.n <= 0 || t.n <= 0 || !mask || mwords * 64 < t.n)
        return hipErrorInvalidValue;
    const int nq = (int)q.n, nt = (int)t.n;
    const int ns = m_splits(q.n, t.n);
    int per = (nt + ns - 1) / ns;
    per = (per + kMStage - 1) / kMStage * kMStage;
    const dim3 grid((unsigned)((nq + kMQPerWG - 1) / kMQPerWG), (unsigned)ns);
    if (k == 1)
        hipLaunchKernelGGL(masked_i8_kernel<1>, grid, dim3(256), 0, stream, (const int8_t*)q.rows8, (const int32_t*)q.norm, nq,
                           (const int8_t*)t.rows8, (const int32_t*)t.norm, nt, per, mask, mwords, partial, (const unsigned long long*)t.real);
    else
        hipLaunchKernelGGL(masked_i8_kernel<2>, grid, dim3(256), 0, stream, (const int8_t*)q.rows8, (const int32_t*)q.norm, nq,
                           (const int8_t*)t.rows8, (const int32_t*)t.norm, nt, per, mask, mwords, partial, (const unsigned long long*)t.real);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_knnk_merge(partial, ns, nq, k, d_idx, d_dist, stream);
}

// ---- host side ----------------------------------------------------------------------------------------------------------
int mask_alloc(fm_ctx* ctx, int64_t nq, const std::vector<int64_t>& rows, const std::vector<int64_t>& phys, int64_t n_pad,
               const char* who, fm_mask** out)
{
    fm_mask* m = new (std::nothrow) fm_mask();
    if (!m) return fail(ctx, FM_ENOMEM, std::string(who) + ": out of host memory");
    m->ctx = ctx; m->nq = nq; m->n_pad = n_pad; m->words = n_pad / 64;
    m->rows = rows; m->phys = phys;
    for (int64_t r : rows) m->nt += r;
    m->bytes = (size_t)nq * (size_t)m->words * 8;
    if (m->bytes > 0) {
        hipError_t e = hipSetDevice(ctx->device);
        if (e == hipSuccess) e = hipMalloc((void**)&m->bits, m->bytes);
        if (e == hipSuccess) e = hipMemsetAsync(m->bits, 0, m->bytes, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            if (m->bits) (void)hipFree(m->bits);
            delete m;
            return fail(ctx, e == hipErrorOutOfMemory ? FM_ENOMEM : FM_EDEVICE, std::string(who) + ": " + hipGetErrorString(e));
        }
    }
    *out = m;
    return FM_OK;
}

int mask_check(fm_ctx* ctx, const fm_mask* m, const char* who)
{
    if (m->ctx != ctx) return fail(ctx, FM_EINVAL, std::string(who) + ": the mask belongs to another context");
    return FM_OK;
}

// Query rows per launch of the pack / fill kernels.  A launch may hold fewer than 2^32 work-items in x; the pack kernel
// spends 64 per word, so a launch takes at most 2^26 - 4 words (the option "mask_pack_words", which tests lower so that
// small masks take several launches), and always at least one row (an image has at most 2^25 words: 2^31 work-items).
static int64_t mask_rows_per_launch(const fm_ctx* ctx, int64_t iw)
{
    return std::max<int64_t>(1, (int64_t)ctx->tune.mask_pack_words / iw);
}

static hipError_t pack_rows(fm_ctx* ctx, const fm_mask* m, int img, const uint8_t* d_src, int64_t pitch, int64_t q0, int64_t n)
{
    const int64_t R = m->rows[(size_t)img], iw = pad128(R) / 64, w0 = m->phys[(size_t)img] / 64;
    const int64_t step = mask_rows_per_launch(ctx, iw);
    for (int64_t r0 = 0; r0 < n; r0 += step) {
        const int64_t nr = std::min(step, n - r0);
        hipLaunchKernelGGL(mask_pack_kernel, dim3((unsigned)((nr * iw + 3) / 4)), dim3(256), 0, ctx->stream,
                           d_src + (size_t)r0 * pitch, pitch, nr, R, iw, m->bits, m->words, q0 + r0, w0);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// The common part of fm_mask_set_u8 / fm_mask_set_dev.
static int mask_set(fm_ctx* ctx, fm_mask* m, int32_t img, const uint8_t* rows, int64_t pitch, bool dev, void* producer, const char* who)
{
    if (!ctx) return fail(nullptr, FM_EINVAL, std::string(who) + ": ctx is NULL");
    if (!m) return fail(ctx, FM_EINVAL, std::string(who) + ": mask is NULL");
    int rc = mask_check(ctx, m, who);
    if (rc != FM_OK) return rc;
    if (img < 0 || (size_t)img >= m->rows.size())
        return fail(ctx, FM_EINVAL, std::string(who) + ": image " + std::to_string(img) + " is outside the mask (" + std::to_string(m->rows.size()) + " images)");
    const int64_t R = m->rows[(size_t)img];
    if (pitch == 0) pitch = R;
    if (pitch < R) return fail(ctx, FM_EINVAL, std::string(who) + ": pitch " + std::to_string(pitch) + " is below the row width " + std::to_string(R));
    if (m->nq == 0 || R == 0) return FM_OK;
    if (!rows) return fail(ctx, FM_EINVAL, std::string(who) + ": the source rows are NULL");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (dev) {
        if ((rc = check_device_ptr(ctx, rows, who, "d_rows")) != FM_OK) return rc;
        if ((rc = wait_for_stream(ctx, producer)) != FM_OK) return rc;
        HIP_TRY(ctx, pack_rows(ctx, m, img, rows, pitch, 0, m->nq));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));          // (the source is not read after the call, as in fm_bank_create_dev)
        return FM_OK;
    }
    // chunks of query rows through the bounded workspace: dense [rows][R] bytes
    const int64_t cr = std::max<int64_t>(1, std::min<int64_t>(m->nq, (int64_t)(kMaskChunkBytes / (size_t)R)));
    if ((rc = ws_ensure(ctx, &ctx->ws_in, &ctx->ws_in_bytes, (size_t)cr * (size_t)R + 64)) != FM_OK) return rc;
    for (int64_t q0 = 0; q0 < m->nq; q0 += cr) {
        const int64_t n = std::min(cr, m->nq - q0);
        HIP_TRY(ctx, hipMemcpy2DAsync(ctx->ws_in, (size_t)R, rows + (size_t)q0 * pitch, (size_t)pitch, (size_t)R, (size_t)n,
                                      hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, pack_rows(ctx, m, img, (const uint8_t*)ctx->ws_in, R, q0, n));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));          // (the workspace is re-used by the next chunk; the caller's rows are free on return)
    }
    return FM_OK;
}

int knn_masked_device(fm_ctx* ctx, const Bank& q, const Bank& t, const fm_mask* m, int k, int32_t* d_idx, float* d_dist)
{
    const int64_t nq = q.n;
    int rc;
    if (t.n == 0 || m->nt == 0) {          // no train rows: the merge of no lists, -1 / +inf
        if ((rc = ws_ensure(ctx, &ctx->ws_partial, &ctx->ws_partial_bytes, 64)) != FM_OK) return rc;
        HIP_TRY(ctx, launch_knnk_merge((const unsigned long long*)ctx->ws_partial, 0, (int)nq, k, d_idx, d_dist, ctx->stream));
        return FM_OK;
    }
    const bool mfma = q.kind == FM_BANK_I8 && k <= 2 && ctx->tune.masked_mfma != 0;
    const size_t need = mfma ? masked_i8_partial_bytes(nq, t.n, k) : knnk_partial_bytes(nq, t.n, k);
    if ((rc = ws_ensure(ctx, &ctx->ws_partial, &ctx->ws_partial_bytes, need + 64)) != FM_OK) return rc;
    unsigned long long* partial = (unsigned long long*)ctx->ws_partial;
    if (mfma)
        HIP_TRY(ctx, launch_masked_i8(q, t, k, m->bits, m->words, partial, d_idx, d_dist, ctx->stream));
    else if (q.kind == FM_BANK_BIN)
        HIP_TRY(ctx, launch_hamming_knnk(q, t, k, partial, d_idx, d_dist, ctx->stream, nullptr, m->bits, m->words));
    else
        HIP_TRY(ctx, launch_knnk_masked(q, t, k, partial, d_idx, d_dist, ctx->stream, m->bits, m->words));
    return FM_OK;
}

// Steps 1 .. 4 of the pair forms' error order (the header): handles, check_pair, k, the mask's geometry.
static int pair_masked_check(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, const fm_mask* m, int32_t k, const char* who)
{
    if (!ctx) return fail(nullptr, FM_EINVAL, std::string(who) + ": ctx is NULL");
    if (!q || !t) return fail(ctx, FM_EINVAL, std::string(who) + ": bank is NULL");
    if (!m) return fail(ctx, FM_EINVAL, std::string(who) + ": mask is NULL");
    int rc = check_pair(ctx, q, t, who, true);
    if (rc == FM_OK) rc = refuse_wide(ctx, q, who);
    if (rc != FM_OK) return rc;
    if (k < 1) return fail(ctx, FM_EINVAL, std::string(who) + ": k must be at least 1");
    if (k > 8) return fail(ctx, FM_EUNSUPPORTED, std::string(who) + ": k above 8 is not built");
    if ((rc = mask_check(ctx, m, who)) != FM_OK) return rc;
    if (m->coll) return fail(ctx, FM_EINVAL, std::string(who) + ": the mask was made for a collection (fm_mask_create_coll); a bank pair takes fm_mask_create's");
    if (m->nq != q->n)
        return fail(ctx, FM_EINVAL, std::string(who) + ": the mask has " + std::to_string(m->nq) + " query rows, the query bank " + std::to_string(q->n));
    if (m->nt != t->n)
        return fail(ctx, FM_EINVAL, std::string(who) + ": the mask has " + std::to_string(m->nt) + " train rows, the train bank " + std::to_string(t->n));
    return FM_OK;
}

}  // namespace fm

using namespace fm;

extern "C" int fm_mask_create(fm_ctx* ctx, int64_t nq, int64_t nt, fm_mask** mask)
{
    if (!ctx) return fail(nullptr, FM_EINVAL, "fm_mask_create: ctx is NULL");
    if (!mask) return fail(ctx, FM_EINVAL, "fm_mask_create: mask out pointer is NULL");
    *mask = nullptr;
    if (nq < 0 || nt < 0) return fail(ctx, FM_EINVAL, "fm_mask_create: bad nq / nt");
    if (nq > 0x7fffffff || nt > 0x7fffffff - 2 * kStageRows) return fail(ctx, FM_EUNSUPPORTED, "fm_mask_create: more than 2^31 - 1 rows");
    return mask_alloc(ctx, nq, std::vector<int64_t>{nt}, std::vector<int64_t>{0}, pad128(nt), "fm_mask_create", mask);
}

extern "C" int fm_mask_set_u8(fm_ctx* ctx, fm_mask* mask, int32_t img, const uint8_t* rows, int64_t pitch)
{
    return mask_set(ctx, mask, img, rows, pitch, false, FM_NO_STREAM, "fm_mask_set_u8");
}

extern "C" int fm_mask_set_dev(fm_ctx* ctx, fm_mask* mask, int32_t img, const void* d_rows, int64_t pitch, void* producer_stream)
{
    return mask_set(ctx, mask, img, (const uint8_t*)d_rows, pitch, true, producer_stream, "fm_mask_set_dev");
}

extern "C" int fm_mask_set_all(fm_ctx* ctx, fm_mask* mask, int32_t img, int32_t value)
{
    if (!ctx) return fail(nullptr, FM_EINVAL, "fm_mask_set_all: ctx is NULL");
    if (!mask) return fail(ctx, FM_EINVAL, "fm_mask_set_all: mask is NULL");
    int rc = mask_check(ctx, mask, "fm_mask_set_all");
    if (rc != FM_OK) return rc;
    if (img < 0 || (size_t)img >= mask->rows.size())
        return fail(ctx, FM_EINVAL, "fm_mask_set_all: image " + std::to_string(img) + " is outside the mask (" + std::to_string(mask->rows.size()) + " images)");
    const int64_t R = mask->rows[(size_t)img], iw = pad128(R) / 64;
    if (mask->nq == 0 || R == 0) return FM_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int64_t step = mask_rows_per_launch(ctx, iw);
    for (int64_t q0 = 0; q0 < mask->nq; q0 += step) {
        const int64_t nr = std::min(step, mask->nq - q0);
        hipLaunchKernelGGL(mask_fill_kernel, dim3((unsigned)((nr * iw + 255) / 256)), dim3(256), 0, ctx->stream, mask->bits, mask->words,
                           q0, nr, mask->phys[(size_t)img] / 64, iw, R, (int)value);
        HIP_TRY(ctx, hipGetLastError());
    }
    return FM_OK;
}

extern "C" int fm_mask_destroy(fm_ctx* ctx, fm_mask* mask)
{
    if (!mask) return FM_OK;
    if (ctx) sync_all_streams(ctx);
    if (mask->bits) (void)hipFree(mask->bits);
    delete mask;
    return FM_OK;
}

extern "C" int fm_mask_info(const fm_mask* mask, int64_t* nq, int64_t* nt, int32_t* n_images, int64_t* bytes)
{
    if (!mask) return fail(nullptr, FM_EINVAL, "fm_mask_info: mask is NULL");
    if (nq) *nq = mask->nq;
    if (nt) *nt = mask->nt;
    if (n_images) *n_images = mask->coll ? (int32_t)mask->rows.size() : 0;
    if (bytes) *bytes = (int64_t)mask->bytes;
    return FM_OK;
}

extern "C" int fm_knn_masked(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, const fm_mask* mask, int32_t k, int32_t* idx, float* dist)
{
    int rc = pair_masked_check(ctx, q, t, mask, k, "fm_knn_masked");
    if (rc != FM_OK) return rc;
    const int64_t nq = q->n;
    if (nq > 0 && (!idx || !dist)) return fail(ctx, FM_EINVAL, "fm_knn_masked: output pointer is NULL");
    if (nq == 0) return FM_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t ob = align256((size_t)nq * (size_t)k * 4);
    if ((rc = ws_ensure(ctx, &ctx->ws_out, &ctx->ws_out_bytes, 2 * ob + 64)) != FM_OK) return rc;
    int32_t* d_idx = (int32_t*)ctx->ws_out;
    float* d_dist = (float*)((char*)ctx->ws_out + ob);
    CallScope cs(ctx);
    HIP_TRY(ctx, hipEventRecord(ctx->ev_k0, ctx->stream));
    if ((rc = knn_masked_device(ctx, *q, *t, mask, k, d_idx, d_dist)) != FM_OK) return rc;
    HIP_TRY(ctx, hipEventRecord(ctx->ev_k1, ctx->stream));
    ctx->kernel_timed = true;
    ctx->pending_pairs += nq * t->n;
    ctx->pending_bytes += bank_bytes(q) + bank_bytes(t);
    HIP_TRY(ctx, d2h(ctx, idx, d_idx, (size_t)nq * k * 4));
    HIP_TRY(ctx, d2h(ctx, dist, d_dist, (size_t)nq * k * 4));
    return cs.finish();
}

extern "C" int fm_knn_masked_dev(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, const fm_mask* mask, int32_t k, int32_t* d_idx,
                                 float* d_dist, void* consumer_stream)
{
    const char* who = "fm_knn_masked_dev";
    int rc = pair_masked_check(ctx, q, t, mask, k, who);
    if (rc != FM_OK) return rc;
    const int64_t nq = q->n;
    if (nq == 0) return FM_OK;
    if (!d_idx || !d_dist) return fail(ctx, FM_EINVAL, "fm_knn_masked_dev: output pointer is NULL");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((rc = check_device_ptr(ctx, d_idx, who, "d_idx")) != FM_OK || (rc = check_device_ptr(ctx, d_dist, who, "d_dist")) != FM_OK) return rc;
    // (the sweep and the merge are launched together: the context's stream waits for the consumer's work in front of both)
    if ((rc = wait_for_stream(ctx, consumer_stream)) != FM_OK) return rc;
    if ((rc = knn_masked_device(ctx, *q, *t, mask, k, d_idx, d_dist)) != FM_OK) return rc;
    return results_written(ctx, consumer_stream);
}
