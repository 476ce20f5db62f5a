// C-ABI of libfastmatch_hip.so (include/fastmatch_hip.h), part 2b: train collections -- cv2.BFMatcher.add / train / clear and
// match / knnMatch against all added images (DMatch.imgIdx).
//
// Layout.  One integer-route bank (`stack`: rows8 / norm / aux) holds every image; a non-empty image starts on a 128-row
// stage and its last stage ends in padding rows prepared like any bank's tail (cinit = kPadCinit: the matrix-core sweeps
// never prefer them to a real row), so
//   * rows [phys[i], phys[i] + pad128(rows[i])) ARE a bank: the reduced operand of the top-2 sweep for image i alone
//     (fm_collection_knn2_each), and
//   * the used part of the allocation is one bank of n = n_pad = `used` rows for the stacked sweep (fm_collection_knn,
//     _knn2_ratio, _votes mode 0).
// The kernels that read rows and norms instead of the aux words (K9's vector-ALU lists, the float32-root repair) see a
// padding row through its norm: a collection writes 2^26 there (a plain bank: 0), which puts the row at d^2 >= 2^26,
// beyond every real pair (<= 128 * 255^2), with room left in int32.  A padding row can therefore enter a list only
// where fewer than k real rows exist, always behind them, and the lookup (physical row -> image, row) turns it into
// -1 / -1 / +inf.  Lookup tables on the device, per 128-row stage: its image and its number of real rows; per image: its
// first physical row.  Physical order = logical (image, row) order, so keys (distance, physical row) order ties the way
// OpenCV's per-image insertion does: the earlier image, then the earlier row.
// fm_collection_match_accepted_each (further down) is the first caller that makes the stack the OUTPUT operand of a
// sweep; what the padding rows do there is written down in front of it.
// The match graph -- image pairs inside a collection, and a wide query bank image by image -- is a unit of its own,
// api_pairs.hip; coll_internal.h holds the collection object and what that unit calls here.
#include "coll_internal.h"

#include <algorithm>
#include <atomic>

using namespace fm;

// The three kinds.  Integer route: as above.  Float32 route (the first float32 image with a value that is not an integer in
// 0 .. 255 REBUILDS a collection of integer-valued float32 images on the float32 route, on the device, from the int8 rows:
// nothing is uploaded again): rowsf / rowsh / normf / auxf, the fp16 planes of ALL images on the ONE power-of-two scale
// chosen at the rebuild (an image that leaves fp16's range under it switches the filter off for the collection: K5
// alone, same results); a padding row is a padding row of the fp16 planes (auxf = -3.4e38) and holds kCollPadF32 in every
// float32 dimension, so the exact chain -- K8's rescoring and rescan, K5, K9 -- puts it at >= 9.7e18, behind every real
// row (<= 3.3e18) as long as no finite magnitude exceeds kCollF32Max, which add and the match calls enforce: masked by
// value, no kernel changed.  Binary: rowsb / rows4; an all-zero FP4 row is at W / 2 from everything, so K11
// masks by INDEX: its sweep and its vector-ALU kernel take the per-stage real-row table (stage_real).
// A fourth kind, wide (FM_BANK_F32W, fm_collection_add_wide: coll_add_wide below), masks by INDEX as well and serves the
// match graph (fm_collection_pairs_mutual_ratio) and, under names of their own, a wide query bank image by image
// (fm_collection_wide_mutual_ratio_each, fm_collection_wide_knn2_each: api_pairs.hip; fm_collection_wide_match_accepted_each:
// coll_elect_each's wide form below); every other call that takes a query bank refuses it (coll_refuse_wide).  (kCollPadNorm, kCollPadF32, kCollF32Max: coll_internal.h.)
static uint64_t coll_next_gen()
{
    static std::atomic<uint64_t> g{0};
    return ++g;
}

// ---------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------
__global__ void coll_pad_norm_kernel(int32_t* __restrict__ norm, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) norm[i] = kCollPadNorm;
}

// (CollTab, coll_lookup, coll_real: coll_tab.h -- K10's compaction shares them)

// One (query bank, reduced bank) slot of a merge launch: the stacked sweep (tab set, one slot) or one image of
// fm_collection_knn2_each (tab null: rows are the image's own).
struct CollSlot {
    const unsigned long long* partial;    // null: the image is empty, every entry -1 / +inf
    int nsplit, ncols_alloc;
    unsigned* fix;                        // rows for the float32-root repair (fix[0] = count, rows from fix[4]) or null
    int64_t out;                          // first output entry of the slot (in units of 2 entries per query row)
};
struct CollMerge { CollSlot s[kRRBatchMax]; };

// Top-2 merge of K2's split partials (keys (d2 << 32) | row) as knn2_merge_kernel, with the row lookup fused in;
// blockIdx.y = slot.  img may be null (per-image lists).
__global__ __launch_bounds__(256)
void coll_merge2_kernel(CollMerge m, CollTab tab, int64_t nq, int32_t* __restrict__ img, int32_t* __restrict__ idx,
                        float* __restrict__ dist, int f32)
{
    const CollSlot& sl = m.s[blockIdx.y];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nq) return;
    unsigned long long b0 = ~0ull, b1 = ~0ull;
    for (int s = 0; s < sl.nsplit; ++s) {
        const unsigned long long* p = sl.partial + ((size_t)s * sl.ncols_alloc + i) * 2;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            unsigned long long v = p[k];
            if (tab.st_img && !coll_real(tab, v)) v = ~0ull;
            if (v < b0) { b1 = b0; b0 = v; }
            else if (v < b1) { b1 = v; }
        }
    }
    const int64_t o = 2 * (sl.out + i);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const unsigned long long b = k ? b1 : b0;
        int32_t im = -1, lo = -1;
        if (b != ~0ull) {
            if (tab.st_img) (void)coll_lookup(tab, (unsigned)b, im, lo);
            else { im = 0; lo = (int32_t)(unsigned)b; }
        }
        if (img) img[o + k] = im;
        idx[o + k] = lo;
        const unsigned hi = (unsigned)(b >> 32);         // integer route: d2; float32 route and binary: the distance's bits
        dist[o + k] = (b == ~0ull) ? INFINITY : (f32 ? __uint_as_float(hi) : sqrtf((float)hi));
    }
    // (the float32 order can differ from the d2 order: see knn2_merge_kernel)
    if (sl.fix && b1 != ~0ull && (unsigned)(b1 >> 32) >= kSqrtTieMin) {
        const unsigned e0 = (unsigned)(b0 >> 32), e1 = (unsigned)(b1 >> 32);
        const bool paired1 = sqrt_ties_up(e1) || sqrt_ties_up(e1 - 1u);
        const bool paired0 = e0 >= kSqrtTieMin && (sqrt_ties_up(e0) || sqrt_ties_up(e0 - 1u));
        if (paired0 || paired1) sl.fix[4 + atomicAdd(sl.fix, 1u)] = (unsigned)i;
    }
}

// sqrt_fix_kernel<2> (api_match.hip) for a collection: exact rescan of the listed query rows over the reduced rows
// [0, nred) in OpenCV's (float32 root, row) order; padding rows sit at d2 >= 2^26 behind every real row and are
// dropped by the lookup.  out = first output entry of the slot, as CollSlot::out.
__global__ __launch_bounds__(256)
void coll_sqrt_fix_kernel(const unsigned* __restrict__ fix, const int8_t* __restrict__ col_rows,
                          const int32_t* __restrict__ col_norm, const int8_t* __restrict__ red_rows,
                          const int32_t* __restrict__ red_norm, int nred, CollTab tab, int64_t out,
                          int32_t* __restrict__ img, int32_t* __restrict__ idx, float* __restrict__ dist)
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
        const unsigned long long mine = (k0 == g0) ? k1 : k0;
        if (mine != ~0ull) atomicMin(&best[1], mine);
        __syncthreads();
        if (tid == 0) {
            const int64_t o = 2 * (out + (int64_t)c);
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const unsigned long long g = best[k];
                int32_t im = -1, lo = -1;
                bool has = g != ~0ull;
                if (has) {
                    if (tab.st_img) has = coll_lookup(tab, (unsigned)g, im, lo);
                    else { im = 0; lo = (int32_t)(unsigned)g; }
                }
                if (img) img[o + k] = has ? im : -1;
                idx[o + k] = has ? lo : -1;
                dist[o + k] = has ? __uint_as_float((unsigned)(g >> 32)) : INFINITY;
            }
        }
        __syncthreads();
    }
}

hipError_t launch_coll_sqrt_fix(const unsigned* fix, const int8_t* col_rows, const int32_t* col_norm, const int8_t* red_rows,
                                const int32_t* red_norm, int nred, CollTab tab, int64_t out, int32_t* img, int32_t* idx, float* dist,
                                hipStream_t stream)
{
    hipLaunchKernelGGL(coll_sqrt_fix_kernel, dim3(kFixGrid), dim3(256), 0, stream, fix, col_rows, col_norm, red_rows, red_norm, nred, tab, out,
                       img, idx, dist);
    return hipGetLastError();
}

// k = 3 .. 8: K9 wrote physical rows; one thread per entry looks its (image, row) up.  A padding row (fewer than k real
// rows in the collection; it sorts behind them) becomes -1 / -1 / +inf.
__global__ void coll_translate_kernel(CollTab tab, int64_t n, int32_t* __restrict__ img, int32_t* __restrict__ idx,
                                      float* __restrict__ dist)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t p = idx[i];
    int32_t im = -1, lo = -1;
    const bool has = p >= 0 && coll_lookup(tab, (unsigned)p, im, lo);
    img[i] = has ? im : -1;
    idx[i] = has ? lo : -1;
    if (!has) dist[i] = INFINITY;
}

// first column of [n][2] lists
__global__ void coll_col0_kernel(const int32_t* __restrict__ a2, const float* __restrict__ d2, const int32_t* __restrict__ b2,
                                 int64_t n, int32_t* __restrict__ a, float* __restrict__ d, int32_t* __restrict__ b)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    a[i] = a2[2 * i];  d[i] = d2[2 * i];  b[i] = b2[2 * i];
}

// Rebuild on the float32 route: an image's int8 rows (value XOR 0x80 = the uint8 value) as float32, dims from `dim` on 0.
__global__ void coll_i8_to_f32_kernel(const int8_t* __restrict__ rows8, int64_t n, int dim, float* __restrict__ rowsf)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * kDim) return;
    const int k = (int)(i % kDim);
    rowsf[i] = k < dim ? (float)((int)rows8[i] + 128) : 0.f;
}

__global__ void coll_fill_f32_kernel(float* __restrict__ p, int64_t n, float v)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

// Ordered compaction of the accepted rows: compact_kernel (api_match.hip) with the image column.
__global__ __launch_bounds__(256)
void coll_compact_kernel(const int32_t* __restrict__ img2, const int32_t* __restrict__ tidx, const float* __restrict__ dist,
                         const double* __restrict__ ratio, const uint8_t* __restrict__ pass, const int* __restrict__ block_counts,
                         int64_t nq, int64_t cap, int32_t* __restrict__ o_q, int32_t* __restrict__ o_m, int32_t* __restrict__ o_t,
                         float* __restrict__ o_d, double* __restrict__ o_r, unsigned long long* __restrict__ npass)
{
    int64_t q, total;
    bool p;
    const int64_t dst = compact_slot(block_counts, pass, nq, &q, &p, &total);
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) *npass = (unsigned long long)total;
    if (p && dst < cap) { o_q[dst] = (int32_t)q; o_m[dst] = img2[2 * q]; o_t[dst] = tidx[q]; o_d[dst] = dist[q]; o_r[dst] = ratio[q]; }
}

// The same ordered compaction into 16-byte rows {query, image, row inside the image, float32 distance bits} in the caller's
// device memory (fm_collection_knn2_ratio_dev): compact_rows_kernel (api_match.hip) with the image column.
__global__ __launch_bounds__(256)
void coll_compact_rows_kernel(const int32_t* __restrict__ img2, const int32_t* __restrict__ tidx, const float* __restrict__ dist,
                              const uint8_t* __restrict__ pass, const int* __restrict__ block_counts, int64_t nq, int64_t cap,
                              int32_t* __restrict__ o_rows, long long* __restrict__ o_count, unsigned long long* __restrict__ full)
{
    int64_t q, total;
    bool p;
    const int64_t dst = compact_slot(block_counts, pass, nq, &q, &p, &total);
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
        *o_count = total < cap ? (long long)total : (long long)cap;       // the rows that are THERE; `full` keeps the number accepted
        *full = (unsigned long long)total;
    }
    if (p && dst < cap) {
        o_rows[4 * dst] = (int32_t)q;
        o_rows[4 * dst + 1] = img2[2 * q];
        o_rows[4 * dst + 2] = tidx[q];
        o_rows[4 * dst + 3] = (int32_t)__float_as_uint(dist[q]);
    }
}

// Votes: query rows whose 2-NN list passes d0 / d1 < tau (float64; a missing or zero second distance fails, as
// lowe_kernel) counted per image.  Stacked lists (img != null, one list per query row): at the image of the first
// neighbour; per-image lists [n_images][nq][2] (img null): at the list's own image, blockIdx.y.  Integer atomics: the
// totals do not depend on the order of the additions.
__global__ __launch_bounds__(256)
void coll_votes_kernel(const int32_t* __restrict__ img, const int32_t* __restrict__ idx, const float* __restrict__ dist,
                       int64_t nq, double tau, unsigned long long* __restrict__ votes)
{
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t e = 2 * ((int64_t)blockIdx.y * nq + q);
    bool p = false;
    int im = (int)blockIdx.y;
    if (q < nq) {
        const double r = (idx[e + 1] >= 0) ? (double)dist[e] / (double)dist[e + 1] : NAN;
        p = r < tau;
        if (img) im = img[e];
    }
    if (img) {
        if (p) atomicAdd(votes + im, 1ull);
    } else {
        const unsigned long long mk = __ballot(p);
        if ((threadIdx.x & 63) == 0 && mk) atomicAdd(votes + im, (unsigned long long)__popcll(mk));
    }
}

hipError_t launch_coll_votes(const int32_t* img, const int32_t* idx, const float* dist, int64_t nq, int64_t ny, double tau,
                             unsigned long long* votes, hipStream_t stream)
{
    hipLaunchKernelGGL(coll_votes_kernel, dim3((unsigned)((nq + 255) / 256), (unsigned)ny), dim3(256), 0, stream, img, idx, dist, nq, tau, votes);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// storage
// ---------------------------------------------------------------------------------------
// the device arrays of a kind and their bytes per row
struct CollPlane { void** p; size_t row_bytes; };
static int coll_planes(fm::Bank& b, CollPlane* pl)
{
    int n = 0;
    if (b.kind == FM_BANK_F32) {
        pl[n++] = {(void**)&b.rowsf, (size_t)kDim * 4}; pl[n++] = {(void**)&b.rowsh, (size_t)kDim * 2};
        pl[n++] = {(void**)&b.normf, 4}; pl[n++] = {(void**)&b.auxf, 4};
    } else if (b.kind == FM_BANK_F32W) {
        pl[n++] = {(void**)&b.wrows, (size_t)kWideDim * 4}; pl[n++] = {(void**)&b.wrowsh, (size_t)kWideDim * 2};
        pl[n++] = {(void**)&b.normf, 4}; pl[n++] = {(void**)&b.auxf, 4};
    } else if (b.kind == FM_BANK_BIN) {
        pl[n++] = {(void**)&b.rowsb, (size_t)b.ksteps * 16}; pl[n++] = {(void**)&b.rows4, (size_t)b.ksteps * 64};
    } else {
        pl[n++] = {(void**)&b.rows8, (size_t)kDim}; pl[n++] = {(void**)&b.norm, 4};
        pl[n++] = {(void**)&b.aux, (size_t)kAuxPerTile * 4 / kTileRows};
    }
    return n;
}

static void coll_free_planes(fm::Bank& b)
{
    void** all[] = {(void**)&b.rows8, (void**)&b.norm, (void**)&b.aux, (void**)&b.rowsf, (void**)&b.rowsh, (void**)&b.normf,
                    (void**)&b.auxf, (void**)&b.rowsb, (void**)&b.rows4, (void**)&b.wrows, (void**)&b.wrowsh};
    for (void** p : all) { if (*p) (void)hipFree(*p); *p = nullptr; }
    b.cap_pad = 0;
}

static void coll_free(fm_collection* c)
{
    coll_free_planes(c->stack);
    if (c->d_tab) (void)hipFree(c->d_tab);
    c->d_tab = nullptr;
    c->tab_bytes = 0;
}

static void coll_reset(fm_collection* c)
{
    c->dim = 0; c->src = 0; c->used = 0; c->total = 0;
    c->wvmax = 0.f; c->wscale = false;
    c->rows.clear(); c->phys.clear(); c->usq.clear();
    c->stack.n = 0; c->stack.n_pad = 0; c->stack.usq_max = 0; c->stack.dim = 0;
    c->stack.nm_max = 0.f; c->stack.kscale = 0; c->stack.filt_ok = false;
    c->dirty = true;
    c->gen = coll_next_gen();
}

// Arrays of `kind` for `cap` rows into *nb (its other fields untouched); the first `copy` rows of `from`'s arrays are copied on
// the device when `from` is of the same kind.
static int coll_alloc(fm_ctx* ctx, fm::Bank* nb, int64_t cap, fm::Bank* from, int64_t copy)
{
    CollPlane np[4], op[4];
    const int n = coll_planes(*nb, np);
    hipError_t e = hipSuccess;
    for (int i = 0; i < n && e == hipSuccess; ++i) e = hipMalloc(np[i].p, (size_t)cap * np[i].row_bytes);
    if (e == hipSuccess && from && copy > 0) {
        coll_planes(*from, op);
        for (int i = 0; i < n && e == hipSuccess; ++i)
            e = hipMemcpyAsync(*np[i].p, *op[i].p, (size_t)copy * np[i].row_bytes, hipMemcpyDeviceToDevice, ctx->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        coll_free_planes(*nb);
        return fail(ctx, e == hipErrorOutOfMemory ? FM_ENOMEM : FM_EDEVICE, std::string("fm_collection_add: growing the arrays: ") + hipGetErrorString(e));
    }
    nb->cap_pad = cap;
    return FM_OK;
}

// room for `need` physical rows: new arrays of at least twice the size, the used part copied on the device
static int coll_reserve(fm_ctx* ctx, fm_collection* c, int64_t need)
{
    if (need <= c->stack.cap_pad) return FM_OK;
    int64_t cap = std::max<int64_t>(need, 2 * c->stack.cap_pad);
    cap = std::max<int64_t>(cap, 32 * kStageRows);
    if (cap > (int64_t)INT32_MAX - 2 * kStageRows) cap = need;
    if (cap > (int64_t)INT32_MAX - 2 * kStageRows) return fail(ctx, FM_EUNSUPPORTED, "fm_collection_add: the collection would exceed 2^31 rows");
    fm::Bank nb = c->stack;
    nb.rows8 = nullptr; nb.norm = nullptr; nb.aux = nullptr; nb.rowsf = nullptr; nb.rowsh = nullptr; nb.normf = nullptr; nb.auxf = nullptr;
    nb.rowsb = nullptr; nb.rows4 = nullptr; nb.wrows = nullptr; nb.wrowsh = nullptr;
    int rc = coll_alloc(ctx, &nb, cap, &c->stack, c->used);
    if (rc != FM_OK) return rc;
    coll_free_planes(c->stack);
    c->stack = nb;
    return FM_OK;
}

// The stack in another kind (it holds no rows, or the caller fills the new arrays): frees the old arrays.
static int coll_set_kind(fm_ctx* ctx, fm_collection* c, int kind, int ksteps, int64_t cap)
{
    sync_all_streams(ctx);
    coll_free_planes(c->stack);
    c->stack.kind = kind;
    c->stack.ksteps = ksteps;
    return cap > 0 ? coll_alloc(ctx, &c->stack, cap, nullptr, 0) : FM_OK;
}

int coll_check(fm_ctx* ctx, const fm_collection* c, const char* who)
{
    if (!ctx) return fail(nullptr, FM_EINVAL, std::string(who) + ": ctx is NULL");
    if (!c) return fail(ctx, FM_EINVAL, std::string(who) + ": collection is NULL");
    if (c->ctx != ctx) return fail(ctx, FM_EINVAL, std::string(who) + ": the collection belongs to another context");
    return FM_OK;
}

extern "C" int fm_collection_create(fm_ctx* ctx, fm_collection** out)
{
    if (!ctx) return fail(nullptr, FM_EINVAL, "fm_collection_create: ctx is NULL");
    if (!out) return fail(ctx, FM_EINVAL, "fm_collection_create: out pointer is NULL");
    fm_collection* c = new (std::nothrow) fm_collection();
    if (!c) return fail(ctx, FM_ENOMEM, "fm_collection_create: out of host memory");
    c->ctx = ctx;
    c->stack.kind = FM_BANK_I8;
    c->gen = coll_next_gen();
    *out = c;
    return FM_OK;
}

extern "C" int fm_collection_destroy(fm_ctx* ctx, fm_collection* c)
{
    if (!c) return FM_OK;
    int rc = coll_check(ctx, c, "fm_collection_destroy");
    if (rc != FM_OK) return rc;
    (void)hipSetDevice(ctx->device);
    sync_all_streams(ctx);
    coll_free(c);
    delete c;
    return FM_OK;
}

extern "C" int fm_collection_clear(fm_ctx* ctx, fm_collection* c)
{
    int rc = coll_check(ctx, c, "fm_collection_clear");
    if (rc != FM_OK) return rc;
    coll_reset(c);            // (the arrays stay: the next images re-use them)
    return FM_OK;
}

// fp16 planes of an image's range and the padding rows' far value in rowsf (the planes are prepared while those rows are 0)
static int coll_f32_finish(fm_ctx* ctx, fm_collection* c, int64_t off, int64_t n, int64_t n_pad)
{
    float nmx = 0.f;
    int rc = bank_f32_range_planes(ctx, c->stack, off, n, n_pad, &nmx);
    if (rc != FM_OK) return rc;
    if (nmx > c->stack.nm_max) c->stack.nm_max = nmx;
    if (n_pad > n) {
        const int64_t cnt = (n_pad - n) * kDim;
        hipLaunchKernelGGL(coll_fill_f32_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, ctx->stream,
                           c->stack.rowsf + (size_t)(off + n) * kDim, cnt, kCollPadF32);
        HIP_TRY(ctx, hipGetLastError());
    }
    return FM_OK;
}

static int coll_kscale(float vmax)
{
    int ex = 0;
    if (vmax > 0.f) (void)frexpf(vmax, &ex);
    return vmax > 0.f ? 14 - ex : 0;
}

// An integer-route collection of float32 images becomes a float32-route one: float32 rows from the int8 rows, on the device.
static int coll_rebuild_f32(fm_ctx* ctx, fm_collection* c, float vmax_new, int64_t need)
{
    fm::Bank old = c->stack;                       // (keeps the int8 arrays until the float32 ones are filled)
    fm::Bank nb = fm::Bank();
    nb.kind = FM_BANK_F32; nb.dim = c->dim; nb.n = nb.n_pad = c->used; nb.usq_max = old.usq_max;
    int64_t cap = std::max<int64_t>(std::max<int64_t>(need, old.cap_pad), 32 * kStageRows);
    int rc = coll_alloc(ctx, &nb, cap, nullptr, 0);
    if (rc != FM_OK) return rc;
    nb.kscale = coll_kscale(std::max(vmax_new, c->total > 0 ? 255.f : 0.f));
    nb.filt_ok = true;
    nb.nm_max = 0.f;
    c->stack = nb;
    for (size_t i = 0; i < c->rows.size(); ++i) {
        const int64_t n = c->rows[i], off = c->phys[i];
        if (n == 0) continue;
        const int64_t n_pad = pad128(n);
        hipError_t e = hipMemsetAsync(nb.rowsf + (size_t)off * kDim, 0, (size_t)n_pad * kDim * 4, ctx->stream);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(coll_i8_to_f32_kernel, dim3((unsigned)((n * kDim + 255) / 256)), dim3(256), 0, ctx->stream,
                               (const int8_t*)(old.rows8 + (size_t)off * kDim), n, c->dim, nb.rowsf + (size_t)off * kDim);
            e = hipGetLastError();
        }
        if (e == hipSuccess) rc = coll_f32_finish(ctx, c, off, n, n_pad);
        if (e != hipSuccess || rc != FM_OK) {
            coll_free_planes(c->stack);
            c->stack = old;
            return rc != FM_OK ? rc : fail(ctx, FM_EDEVICE, std::string("fm_collection_add_f32: rebuild on the float32 route: ") + hipGetErrorString(e));
        }
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    coll_free_planes(old);
    return FM_OK;
}

// src: 1 uint8 rows, 2 float32 rows, 3 binary rows (dim = bytes).  dev != nullptr (fm_collection_add_dev): the rows are dev's,
// in device memory, read in place by the device forms of the same preparation steps -- for src 2 as float32, half or
// bfloat16 elements, widened exactly; `rows` is then dev->rows.
static int coll_add(fm_ctx* ctx, fm_collection* c, const void* rows, int64_t n, int dim, int src, int32_t* img_idx, const char* who,
                    const DevSrc* dev = nullptr)
{
    int rc = coll_check(ctx, c, who);
    if (rc != FM_OK) return rc;
    if (n < 0 || dim < 1 || (n > 0 && !rows)) return fail(ctx, FM_EINVAL, std::string(who) + ": bad rows / n / width");
    if (src == 3 ? dim > 64 : dim > kDim)
        return fail(ctx, FM_EUNSUPPORTED, std::string(who) + (src == 3 ? ": binary rows of more than 64 bytes are not supported" :
                                                                    src == 2 && dim <= kWideDim ? ": dim > 128 is not supported (wide float rows, FM_BANK_F32W, enter a collection through fm_collection_add_wide)" :
                                                                    ": dim > 128 is not supported"));
    if (c->rows.size() >= (size_t)INT32_MAX) return fail(ctx, FM_EUNSUPPORTED, std::string(who) + ": too many images");
    if (c->src == 4)
        return fail(ctx, FM_EINVAL, std::string(who) + ": the collection holds wide float images (fm_collection_add_wide); wide and other images do not mix in one collection");
    if (n > 0 && c->dim != 0) {
        if (dim != c->dim) return fail(ctx, FM_EINVAL, std::string(who) + ": the image's width differs from the collection's");
        if (src != c->src) return fail(ctx, FM_EINVAL, std::string(who) + ": uint8, float32 and binary images do not mix in one collection (cv2 raises on the dtype)");
    }
    if (n > 0) {
        const int64_t n_pad = pad128(n);
        const int64_t off = c->used;
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        int usq = 0;
        if (c->dim == 0) {                       // the first non-empty image fixes the kind's arrays
            const int kind = src == 3 ? FM_BANK_BIN : FM_BANK_I8;
            if (c->stack.kind != kind || (kind == FM_BANK_BIN && c->stack.ksteps != (dim + 15) / 16))
                if ((rc = coll_set_kind(ctx, c, kind, kind == FM_BANK_BIN ? (dim + 15) / 16 : 0, 0)) != FM_OK) return rc;
        }
        if (c->stack.kind == FM_BANK_BIN) {
            if ((rc = coll_reserve(ctx, c, off + n_pad)) != FM_OK) return rc;
            const fm::Bank v = bank_rows_view(c->stack, off, n);
            if (dev) {
                HIP_TRY(ctx, launch_hamming_prep(dev->rows, n, dim, v, ctx->stream, dev->pitch));
            } else {
                const size_t src_bytes = (size_t)n * dim;
                if ((rc = ws_ensure(ctx, &ctx->ws_in, &ctx->ws_in_bytes, src_bytes + 64)) != FM_OK) return rc;
                HIP_TRY(ctx, hipMemcpyAsync(ctx->ws_in, rows, src_bytes, hipMemcpyHostToDevice, ctx->stream));
                HIP_TRY(ctx, launch_hamming_prep((const uint8_t*)ctx->ws_in, n, dim, v, ctx->stream));
            }
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));      // (ws_in is free for the next upload; a device source is read)
        } else {
            bool as_f32 = c->stack.kind == FM_BANK_F32;
            if (!as_f32) {
                if ((rc = coll_reserve(ctx, c, off + n_pad)) != FM_OK) return rc;
                int flags[2] = {0, 0};
                if ((rc = bank_prep_range(ctx, rows, n, dim, src == 2, c->stack, off, n_pad, flags, dev)) != FM_OK) return rc;
                usq = flags[1];
                if (src == 2 && flags[0]) as_f32 = true;          // (the range just written lies behind `used`: not part of anything)
                else if (n_pad > n) {
                    hipLaunchKernelGGL(coll_pad_norm_kernel, dim3((unsigned)((n_pad - n + 255) / 256)), dim3(256), 0, ctx->stream,
                                       c->stack.norm + off + n, (int)(n_pad - n));
                    HIP_TRY(ctx, hipGetLastError());              // (stream ordered before every sweep: no synchronisation)
                }
            }
            if (as_f32) {
                // the largest finite magnitude first: it decides the refusal, and the scale of a rebuild, before anything changes
                // (what the integer-route attempt wrote lies behind `used`)
                float hmax = 0.f;
                if (dev) {
                    if ((rc = dev_src_absmax(ctx, *dev, n, dim, &hmax)) != FM_OK) return rc;
                } else {
                    const float* f = (const float*)rows;
                    for (int64_t i = 0; i < n * dim; ++i) { const float a = fabsf(f[i]); if (a <= 3.0e38f && a > hmax) hmax = a; }
                }
                if (hmax > kCollF32Max)
                    return fail(ctx, FM_EUNSUPPORTED, std::string(who) + ": a finite magnitude above 2^57 (FM_COLLECTION_F32_MAX): a float32 "
                                                      "collection masks its padding rows by value (1e18) and cannot hold these rows");
                if (c->stack.kind != FM_BANK_F32) {
                    if (c->dim == 0) c->dim = dim;                // (the rebuild converts rows of this width; no rows yet if this is the first)
                    if ((rc = coll_rebuild_f32(ctx, c, hmax, off + n_pad)) != FM_OK) { if (c->total == 0) c->dim = 0; return rc; }
                }
                if ((rc = coll_reserve(ctx, c, off + n_pad)) != FM_OK) return rc;
                float vmax = 0.f; bool finite = true;
                if ((rc = bank_f32_range_rows(ctx, (const float*)rows, n, dim, c->stack, off, n_pad, &vmax, &finite, dev)) != FM_OK) return rc;
                if (!finite || !(ldexpf(vmax, c->stack.kscale) < 60000.f)) c->stack.filt_ok = false;   // K5 alone from here on (planes unused)
                if ((rc = coll_f32_finish(ctx, c, off, n, n_pad)) != FM_OK) return rc;
            }
        }
        if (c->dim == 0) c->dim = dim;
        if (c->src == 0) c->src = src;
        c->phys.push_back(off);
        c->usq.push_back(usq);
        c->used += n_pad;
        c->total += n;
        if (usq > c->stack.usq_max) c->stack.usq_max = usq;
    } else {
        c->phys.push_back(c->used);
        c->usq.push_back(0);
    }
    c->rows.push_back(n);
    c->stack.dim = c->dim;
    c->stack.n = c->stack.n_pad = c->used;
    c->dirty = true;
    c->gen = coll_next_gen();
    if (img_idx) *img_idx = (int32_t)(c->rows.size() - 1);
    return FM_OK;
}

extern "C" int fm_collection_add_u8(fm_ctx* ctx, fm_collection* c, const uint8_t* rows, int64_t n, int dim, int32_t* img_idx)
{
    return coll_add(ctx, c, rows, n, dim, 1, img_idx, "fm_collection_add_u8");
}

extern "C" int fm_collection_add_f32(fm_ctx* ctx, fm_collection* c, const float* rows, int64_t n, int dim, int32_t* img_idx)
{
    return coll_add(ctx, c, rows, n, dim, 2, img_idx, "fm_collection_add_f32");
}

extern "C" int fm_collection_add_bin(fm_ctx* ctx, fm_collection* c, const uint8_t* rows, int64_t n, int bytes, int32_t* img_idx)
{
    return coll_add(ctx, c, rows, n, bytes, 3, img_idx, "fm_collection_add_bin");
}

// An image from rows that are already in device memory (include/fastmatch_hip.h: "device sources"): fm_bank_create_dev's
// source rules, then coll_add's collection rules on the device forms of its steps.  Passes over the source: uint8 and
// binary one; a floating-point image one on the integer route while it stays integer valued (the preparation with its flag
// words), two on the float32 route (the largest finite magnitude, then the typed copy), three for the image that turns an
// integer-route collection into a float32-route one (the failed integer attempt, the magnitude, the copy).
extern "C" int fm_collection_add_dev(fm_ctx* ctx, fm_collection* c, const void* d_rows, int dtype, int64_t n, int dim,
                                     int64_t row_pitch_bytes, void* producer_stream, int32_t* img_idx)
{
    const char* who = "fm_collection_add_dev";
    int rc = coll_check(ctx, c, who);
    if (rc != FM_OK) return rc;
    if (dtype == FM_DT_BIN2)
        return fail(ctx, FM_EUNSUPPORTED, "fm_collection_add_dev: NORM_HAMMING2 rows (FM_DT_BIN2) are served as bank pairs only (fm_bank_create_dev, "
                                          "fm_bank_create_bin2); a collection takes none");
    if (dtype < FM_DT_U8 || dtype > FM_DT_BIN)
        return fail(ctx, FM_EINVAL, "fm_collection_add_dev: unknown dtype " + std::to_string(dtype) + " (FM_DT_U8 .. FM_DT_BIN)");
    if (n < 0 || dim < 1) return fail(ctx, FM_EINVAL, "fm_collection_add_dev: bad n / width");
    if (dtype == FM_DT_BIN ? dim > 64 : dim > kDim)
        return fail(ctx, FM_EUNSUPPORTED, std::string(who) + (dtype == FM_DT_BIN ? ": binary rows of more than 64 bytes are not supported" :
                                                                    dtype != FM_DT_U8 && dim <= kWideDim ? ": dim > 128 is not supported (wide float rows, FM_BANK_F32W, enter a collection through fm_collection_add_wide)" :
                                                                    ": dim > 128 is not supported"));
    const int64_t elt = dtype == FM_DT_F32 ? 4 : (dtype == FM_DT_F16 || dtype == FM_DT_BF16) ? 2 : 1;
    const int64_t pitch = row_pitch_bytes == 0 ? dim * elt : row_pitch_bytes;
    if (pitch < dim * elt)
        return fail(ctx, FM_EINVAL, "fm_collection_add_dev: row_pitch_bytes " + std::to_string(row_pitch_bytes) + " is below the row size " +
                                    std::to_string(dim * elt));
    if (pitch % elt != 0) return fail(ctx, FM_EINVAL, "fm_collection_add_dev: row_pitch_bytes is not a multiple of the element size");
    const int src = dtype == FM_DT_U8 ? 1 : dtype == FM_DT_BIN ? 3 : 2;
    if (n == 0) return coll_add(ctx, c, nullptr, 0, dim, src, img_idx, who);       // (d_rows is not looked at)
    if (!d_rows) return fail(ctx, FM_EINVAL, "fm_collection_add_dev: d_rows is NULL");
    if ((uintptr_t)d_rows % (uintptr_t)elt != 0) return fail(ctx, FM_EINVAL, "fm_collection_add_dev: d_rows is not aligned to the element size");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((rc = check_device_ptr(ctx, d_rows, who, "d_rows")) != FM_OK) return rc;
    // the rows are complete once the work producer_stream has been given so far is: no host wait for it
    if ((rc = wait_for_stream(ctx, producer_stream)) != FM_OK) return rc;
    const DevSrc dsrc{(const uint8_t*)d_rows, dtype, pitch};
    return coll_add(ctx, c, d_rows, n, dim, src, img_idx, who, &dsrc);
}

// ---- wide collections: images of 129 .. 256 float values per row (K14, wide_f32.hip) ------------------------------------------
// The stack is a FM_BANK_F32W bank (wrows / wrowsh / normf / auxf); an image starts on a 128-row stage, so coll_view(c, i) is a
// wide bank view: wide_copy_kernel writes its rows (zero padded to 256 values and to the stage's end) and wide_planes_kernel
// its scaled planes, the two kernels of fm_bank_create_f32 on the same values -- host and device adds build the same bytes.
// Padding rows are excluded by INDEX in every wide kernel, so any value is accepted: there is no FM_COLLECTION_F32_MAX here.
// One fp16 scale for the whole stack (both views of a pair share it): K8's rule on the running largest finite magnitude.  An
// add that lifts the maximum beyond the scale's range rewrites wrowsh / normf / auxf of every image from wrows on the device
// (nothing is uploaded again); the scale never goes back down.  stack.nm_max is the stack's largest scaled squared norm: the
// filter's margin takes it for every view (wide_f32.hip, part 4).  A value that is not finite switches the filter off for the
// collection (stack.filt_ok): the exact kernel alone, same results.
static int coll_add_wide(fm_ctx* ctx, fm_collection* c, const void* rows, int64_t n, int dim, int32_t* img_idx, const char* who,
                         const DevSrc* dev = nullptr)
{
    int rc = coll_check(ctx, c, who);
    if (rc != FM_OK) return rc;
    if (n < 0 || (n > 0 && !rows)) return fail(ctx, FM_EINVAL, std::string(who) + ": bad rows / n");
    if (dim <= kDim)
        return fail(ctx, FM_EINVAL, std::string(who) + ": wide rows have 129 .. 256 values; rows of up to 128 go to fm_collection_add_f32 / fm_collection_add_dev");
    if (dim > kWideDim) return fail(ctx, FM_EUNSUPPORTED, std::string(who) + ": dim > 256 is not supported");
    if (c->rows.size() >= (size_t)INT32_MAX) return fail(ctx, FM_EUNSUPPORTED, std::string(who) + ": too many images");
    if (c->src != 4 && !c->rows.empty())
        return fail(ctx, FM_EINVAL, std::string(who) + ": the collection holds images of another kind; wide and other images do not mix in one collection");
    if (c->src == 4 && dim != c->dim) return fail(ctx, FM_EINVAL, std::string(who) + ": the image's width differs from the collection's");
    if (c->used + pad128(n) > (int64_t)INT32_MAX - 2 * kStageRows) return fail(ctx, FM_EUNSUPPORTED, std::string(who) + ": the collection would exceed 2^31 rows");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const bool first = c->src != 4;
    if (first && c->stack.kind != FM_BANK_F32W && (rc = coll_set_kind(ctx, c, FM_BANK_F32W, 0, 0)) != FM_OK) return rc;
    float vmax_run = first ? 0.f : c->wvmax, nm_max = first ? 0.f : c->stack.nm_max;
    bool scaled = first ? false : c->wscale, filt_ok = first ? true : c->stack.filt_ok;
    int kscale = first ? 0 : c->stack.kscale;
    if (n > 0) {
        const int64_t n_pad = pad128(n), off = c->used;
        c->stack.dim = dim;
        if ((rc = coll_reserve(ctx, c, off + n_pad)) != FM_OK) return rc;
        const size_t src_bytes = dev ? 0 : (size_t)n * dim * 4;
        const size_t flag_off = (src_bytes + 15) & ~(size_t)15;
        if ((rc = ws_ensure(ctx, &ctx->ws_in, &ctx->ws_in_bytes, flag_off + 32)) != FM_OK) return rc;
        int* d_stat = (int*)((char*)ctx->ws_in + flag_off);
        fm::Bank v = bank_rows_view(c->stack, off, n);
        if (src_bytes) HIP_TRY(ctx, hipMemcpyAsync(ctx->ws_in, rows, src_bytes, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(d_stat, 0, 16, ctx->stream));
        if (dev) HIP_TRY(ctx, launch_wide_copy(dev->rows, dev->dtype, dev->pitch, n, dim, v, d_stat, ctx->stream));
        else     HIP_TRY(ctx, launch_wide_copy(ctx->ws_in, FM_DT_F32, (int64_t)dim * 4, n, dim, v, d_stat, ctx->stream));
        int stat[2] = {0, 0};
        HIP_TRY(ctx, hipMemcpyAsync(stat, d_stat, 8, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        float vmax = 0.f;
        memcpy(&vmax, &stat[0], 4);
        if (stat[1] != 0) filt_ok = false;
        if (vmax > vmax_run) vmax_run = vmax;
        // the scale: chosen at the first magnitude above 0 (all-zero rows have the same planes under every scale), lowered --
        // never raised -- when the running maximum leaves its range
        bool rescale = false;
        const int want = coll_kscale(vmax_run);
        if (!scaled) { if (vmax_run > 0.f) { kscale = want; scaled = true; } }
        else if (want < kscale) { kscale = want; rescale = true; }
        v.kscale = kscale;
        HIP_TRY(ctx, launch_wide_planes(v, d_stat + 2, ctx->stream));
        if (rescale) {
            for (size_t i = 0; i < c->rows.size(); ++i) {
                if (c->rows[i] == 0) continue;
                fm::Bank w = bank_rows_view(c->stack, c->phys[i], c->rows[i]);
                w.kscale = kscale;
                HIP_TRY(ctx, launch_wide_planes(w, d_stat + 2, ctx->stream));
            }
        }
        HIP_TRY(ctx, hipMemcpyAsync(stat, d_stat + 2, 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        float nmx = 0.f;
        memcpy(&nmx, &stat[0], 4);
        nm_max = rescale ? nmx : std::max(nm_max, nmx);
        c->phys.push_back(off);
        c->used += n_pad;
        c->total += n;
    } else {
        c->phys.push_back(c->used);
    }
    c->usq.push_back(0);
    c->rows.push_back(n);
    c->src = 4;
    c->dim = dim;
    c->wvmax = vmax_run; c->wscale = scaled;
    c->stack.kscale = kscale; c->stack.nm_max = nm_max; c->stack.filt_ok = filt_ok; c->stack.vfin_max = vmax_run;
    c->stack.dim = dim;
    c->stack.n = c->stack.n_pad = c->used;
    c->dirty = true;
    c->gen = coll_next_gen();
    if (img_idx) *img_idx = (int32_t)(c->rows.size() - 1);
    return FM_OK;
}

extern "C" int fm_collection_add_wide(fm_ctx* ctx, fm_collection* c, const float* rows, int64_t n, int dim, int32_t* img_idx)
{
    return coll_add_wide(ctx, c, rows, n, dim, img_idx, "fm_collection_add_wide");
}

// fm_collection_add_dev's source rules, then coll_add_wide on the caller's rows: one pass over the source (the typed copy).
extern "C" int fm_collection_add_wide_dev(fm_ctx* ctx, fm_collection* c, const void* d_rows, int dtype, int64_t n, int dim,
                                          int64_t row_pitch_bytes, void* producer_stream, int32_t* img_idx)
{
    const char* who = "fm_collection_add_wide_dev";
    int rc = coll_check(ctx, c, who);
    if (rc != FM_OK) return rc;
    if (dtype != FM_DT_F32 && dtype != FM_DT_F16 && dtype != FM_DT_BF16)
        return fail(ctx, FM_EINVAL, "fm_collection_add_wide_dev: dtype " + std::to_string(dtype) + " is not FM_DT_F32, FM_DT_F16 or FM_DT_BF16");
    if (n < 0) return fail(ctx, FM_EINVAL, "fm_collection_add_wide_dev: bad n");
    if (dim <= kDim || dim > kWideDim || n == 0) return coll_add_wide(ctx, c, nullptr, n > 0 ? 0 : n, dim, img_idx, who);   // (d_rows is not looked at)
    const int64_t elt = dtype == FM_DT_F32 ? 4 : 2;
    const int64_t pitch = row_pitch_bytes == 0 ? dim * elt : row_pitch_bytes;
    if (pitch < dim * elt)
        return fail(ctx, FM_EINVAL, "fm_collection_add_wide_dev: row_pitch_bytes " + std::to_string(row_pitch_bytes) + " is below the row size " +
                                    std::to_string(dim * elt));
    if (pitch % elt != 0) return fail(ctx, FM_EINVAL, "fm_collection_add_wide_dev: row_pitch_bytes is not a multiple of the element size");
    if (!d_rows) return fail(ctx, FM_EINVAL, "fm_collection_add_wide_dev: d_rows is NULL");
    if ((uintptr_t)d_rows % (uintptr_t)elt != 0) return fail(ctx, FM_EINVAL, "fm_collection_add_wide_dev: d_rows is not aligned to the element size");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((rc = check_device_ptr(ctx, d_rows, who, "d_rows")) != FM_OK) return rc;
    // the rows are complete once the work producer_stream has been given so far is: no host wait for it
    if ((rc = wait_for_stream(ctx, producer_stream)) != FM_OK) return rc;
    const DevSrc dsrc{(const uint8_t*)d_rows, dtype, pitch};
    return coll_add_wide(ctx, c, d_rows, n, dim, img_idx, who, &dsrc);
}

// the calls that are not built for a wide collection (include/fastmatch_hip.h, K14)
static int coll_refuse_wide(fm_ctx* ctx, const fm_collection* c, const char* who)
{
    if (!coll_is_wide(c)) return FM_OK;
    return fail(ctx, FM_EUNSUPPORTED, std::string(who) + ": a wide collection (fm_collection_add_wide, FM_BANK_F32W) is served by "
                                      "fm_collection_pairs_mutual_ratio(_dev) and, for a wide query bank, by "
                                      "fm_collection_wide_mutual_ratio_each(_dev) / fm_collection_wide_knn2_each / "
                                      "fm_collection_wide_match_accepted_each(_dev) / fm_collection_wide_radius_match(_dev) / "
                                      "fm_collection_wide_knn(_dev) / fm_collection_wide_knn2_ratio(_dev) / fm_collection_wide_votes only");
}

extern "C" int fm_collection_train(fm_ctx* ctx, fm_collection* c)
{
    int rc = coll_check(ctx, c, "fm_collection_train");
    if (rc != FM_OK) return rc;
    if (!c->dirty) return FM_OK;
    const int64_t ns = c->nstages(), ni = (int64_t)c->rows.size();
    std::vector<int32_t> tab((size_t)(2 * ns + ni + 1), 0);
    for (int64_t i = 0; i < ni; ++i) {
        tab[(size_t)(2 * ns + i)] = (int32_t)c->phys[(size_t)i];
        const int64_t s0 = c->phys[(size_t)i] / kStageRows, n = c->rows[(size_t)i];
        for (int64_t s = 0; s * kStageRows < n; ++s) {
            tab[(size_t)(s0 + s)] = (int32_t)i;
            tab[(size_t)(ns + s0 + s)] = (int32_t)std::min<int64_t>(kStageRows, n - s * kStageRows);
        }
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t bytes = tab.size() * 4;
    if (bytes > c->tab_bytes) {
        sync_all_streams(ctx);
        if (c->d_tab) (void)hipFree(c->d_tab);
        c->d_tab = nullptr; c->tab_bytes = 0;
        const size_t want = bytes * 2;
        HIP_TRY(ctx, hipMalloc((void**)&c->d_tab, want));
        c->tab_bytes = want;
    }
    HIP_TRY(ctx, hipMemcpyAsync(c->d_tab, tab.data(), bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    c->dirty = false;
    return FM_OK;
}

extern "C" int fm_collection_info(const fm_collection* c, int32_t* n_images, int64_t* n_rows_total, int* dim, int* kind)
{
    if (!c) return fail(nullptr, FM_EINVAL, "fm_collection_info: collection is NULL");
    if (n_images) *n_images = (int32_t)c->rows.size();
    if (n_rows_total) *n_rows_total = c->total;
    if (dim) *dim = c->dim;
    if (kind) *kind = c->dim ? c->stack.kind : 0;
    return FM_OK;
}

extern "C" int fm_collection_image_rows(const fm_collection* c, int64_t* rows)
{
    if (!c) return fail(nullptr, FM_EINVAL, "fm_collection_image_rows: collection is NULL");
    if (!rows && !c->rows.empty()) return fail(nullptr, FM_EINVAL, "fm_collection_image_rows: rows is NULL");
    for (size_t i = 0; i < c->rows.size(); ++i) rows[i] = c->rows[i];
    return FM_OK;
}

extern "C" int fm_collection_locate(const int64_t* first_row, int32_t n_images, const int64_t* g, int64_t m, int32_t* img, int64_t* local)
{
    if (n_images < 0 || m < 0 || !first_row || (m > 0 && (!g || !img || !local)))
        return fail(nullptr, FM_EINVAL, "fm_collection_locate: bad arguments");
    for (int32_t i = 0; i < n_images; ++i)
        if (first_row[i + 1] < first_row[i]) return fail(nullptr, FM_EINVAL, "fm_collection_locate: first_row does not ascend");
    for (int64_t j = 0; j < m; ++j) {
        const int64_t r = g[j];
        if (r < first_row[0] || r >= first_row[n_images]) { img[j] = -1; local[j] = -1; continue; }
        // the last image whose first row is <= r (empty images in between share a first row and are skipped)
        const int64_t* e = std::upper_bound(first_row, first_row + n_images + 1, r);
        const int32_t i = (int32_t)(e - first_row) - 1;
        img[j] = i;
        local[j] = r - first_row[i];
    }
    return FM_OK;
}

// ---------------------------------------------------------------------------------------
// matching
// ---------------------------------------------------------------------------------------
// empty_any_kind (the radius calls, as fm_radius_match pairs banks): a query bank without rows has no kind of its own -- the
// creators make every empty bank an integer-route one, fm_bank_create_f32_route included -- and is not held to the collection's.
static int coll_query_check(fm_ctx* ctx, fm_collection* c, const fm_bank* q, const char* who, bool empty_any_kind = false)
{
    int rc = coll_check(ctx, c, who);
    if (rc != FM_OK) return rc;
    if (!q) return fail(ctx, FM_EINVAL, std::string(who) + ": query bank is NULL");
    if ((rc = coll_refuse_wide(ctx, c, who)) != FM_OK) return rc;
    if ((rc = refuse_wide(ctx, q, who)) != FM_OK) return rc;
    if (c->dim != 0 && q->kind != c->stack.kind && !(empty_any_kind && q->n == 0))
        return fail(ctx, FM_EINVAL, std::string(who) + ": the query bank is not of the collection's kind (fm_collection_info)");
    if (c->dim != 0 && q->dim != c->dim) return fail(ctx, FM_EINVAL, std::string(who) + ": the query's width differs from the collection's");
    if (c->dim != 0 && c->stack.kind == FM_BANK_F32 && q->vfin_max > kCollF32Max)
        return fail(ctx, FM_EUNSUPPORTED, std::string(who) + ": the query bank holds a finite magnitude above 2^57 (FM_COLLECTION_F32_MAX): "
                                          "a float32 collection masks its padding rows by value (1e18); match image by image with fm_knn");
    return fm_collection_train(ctx, c);
}

// One-slot merge of a sweep's partials into the lists from entry `out` on (CollSlot::out); ps = null: no reduced rows, every
// entry -1 / +inf.
int coll_merge_one(fm_ctx* ctx, const PairSweep* ps, CollTab tab, int64_t nq, int64_t out, int32_t* d_img, int32_t* d_idx, float* d_dist)
{
    CollMerge mg{};
    CollSlot& sl = mg.s[0];
    sl.out = out;
    if (ps) { sl.partial = ps->partial; sl.nsplit = ps->nsplit; sl.ncols_alloc = ps->ncols_alloc; sl.fix = ps->fix; }
    hipLaunchKernelGGL(coll_merge2_kernel, dim3((unsigned)((nq + 255) / 256), 1), dim3(256), 0, ctx->stream, mg, tab, nq, d_img, d_idx, d_dist,
                       ps ? ps->f32_keys : 0);
    HIP_TRY(ctx, hipGetLastError());
    return FM_OK;
}

// The stacked 2-NN lists of a wide query bank over a wide collection (K14 over the stack, wide_stack.hip): wide_route's rule
// (api_match.hip) with the stack as the reduced bank -- "f32_filter" 0 / 1 / 2 and the 4e6 threshold on the REAL pairs,
// wide_filter_usable, "f32_nsplit", the record cap rule, ws_partial = partial | records | scores | bounds | count, one
// filter launch counted per filtered call and (by the exact kernel itself, behind run_flag) one fallback per call redone.
// The stack's scale, largest scaled squared norm and filt_ok are read HERE, at the call: a later add may rewrite them.
// c->total > 0; the tables are built (fm_collection_train).
static int coll_wide_knn2_device(fm_ctx* ctx, fm_collection* c, const fm_bank* q, const CollTab& tab, int32_t* d_img, int32_t* d_idx,
                                 float* d_dist, void* consumer)
{
    const int64_t nq = q->n;
    const fm::Bank& t = c->stack;
    ctx->pending_pairs += nq * c->total;
    ctx->pending_bytes += bank_bytes(q) + bank_bytes(&t);
    const RowReducePlan pl = plan_rowreduce_f32(q->n_pad, t.n_pad, ctx->tune.nsplit);
    const WideFilterPlan fp = plan_wide_filter(q->n_pad, nq, t.n_pad, ctx->tune);
    const bool filter = ctx->tune.f32_filter != 0 && ctx->d_counters && wide_filter_usable(*q, t) &&
                        (ctx->tune.f32_filter >= 2 || (double)nq * (double)c->total >= 4.0e6) &&
                        nq * std::min<int64_t>(16, c->total) <= (int64_t)fp.cap;
    const size_t part = pl.partial_bytes(2);
    unsigned long long* d_part;
    int rc;
    if (!filter) {
        if ((rc = ws_ensure(ctx, &ctx->ws_partial, &ctx->ws_partial_bytes, part + 64)) != FM_OK) return rc;
        d_part = (unsigned long long*)ctx->ws_partial;
        HIP_TRY(ctx, hipEventRecord(ctx->ev_k0, ctx->stream));
        HIP_TRY(ctx, launch_wide_stack_exact(*q, t, tab.st_real, pl, d_part, nullptr, ctx->stream));
    } else {
        size_t off = 0;
        const size_t o_part = carve(off, part), o_list = carve(off, fp.list_bytes()), o_score = carve(off, fp.list_bytes() / 2),
                     o_bound = carve(off, (size_t)q->n_pad * 4), o_cnt = carve(off, 16);
        if ((rc = ws_ensure(ctx, &ctx->ws_partial, &ctx->ws_partial_bytes, off + 64)) != FM_OK) return rc;
        char* w = (char*)ctx->ws_partial;
        d_part = (unsigned long long*)(w + o_part);
        HIP_TRY(ctx, hipMemsetAsync(d_part, 0xff, part, ctx->stream));
        // (the bounds and the count are neighbours: one fill)
        HIP_TRY(ctx, hipMemsetAsync(w + o_bound, 0, o_cnt + 16 - o_bound, ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(ctx->d_counters, 0, 8, ctx->stream));
        HIP_TRY(ctx, hipEventRecord(ctx->ev_k0, ctx->stream));
        HIP_TRY(ctx, launch_wide_stack_filter(*q, t, tab.st_real, fp, (uint2*)(w + o_list), (float*)(w + o_score), (unsigned*)(w + o_bound),
                                              (unsigned long long*)(w + o_cnt), ctx->d_counters, d_part, ctx->stream));
        HIP_TRY(ctx, launch_wide_stack_exact(*q, t, tab.st_real, pl, d_part, ctx->d_counters, ctx->stream));
        ctx->filter_launches += 1;
    }
    if ((rc = wait_for_stream(ctx, consumer)) != FM_OK) return rc;
    PairSweep ps{};
    ps.partial = d_part; ps.nsplit = pl.nsplit; ps.ncols_alloc = pl.ncols_alloc; ps.f32_keys = 1;
    if ((rc = coll_merge_one(ctx, &ps, tab, nq, 0, d_img, d_idx, d_dist)) != FM_OK) return rc;
    HIP_TRY(ctx, hipEventRecord(ctx->ev_k1, ctx->stream));
    ctx->kernel_timed = true;
    return FM_OK;
}

// The stacked 2-NN lists of q on the device: img / idx / dist [nq][2].  ws_partial: partial | bounds | fix list.  consumer
// (fm_collection_knn_dev: the arrays are the caller's): the stream whose work so far the merge -- the first kernel that writes
// them -- waits for, behind the sweep.
static int coll_knn2_device(fm_ctx* ctx, fm_collection* c, const fm_bank* q, int32_t* d_img, int32_t* d_idx, float* d_dist,
                            void* consumer = FM_NO_STREAM)
{
    const int64_t nq = q->n;
    const CollTab none{nullptr, nullptr, nullptr};
    if (c->total == 0) {
        if (int rc = wait_for_stream(ctx, consumer)) return rc;
        return coll_merge_one(ctx, nullptr, none, nq, 0, d_img, d_idx, d_dist);
    }
    const CollTab tab{c->st_img(), c->st_real(), c->img_phys()};
    const fm::Bank& t = c->stack;
    // (a wide collection gets here from the fm_collection_wide_* calls alone: the L2-named ones have refused it)
    if (coll_is_wide(c)) return coll_wide_knn2_device(ctx, c, q, tab, d_img, d_idx, d_dist, consumer);
    const bool i8 = t.kind == FM_BANK_I8;
    // (the pairs are the real rows'; the stack's padding rows are swept and read like any bank's)
    ctx->pending_pairs += nq * c->total;
    ctx->pending_bytes += bank_bytes(q) + bank_bytes(&t);
    // the float32 route and K11: the bracket takes the merge in
    PairSweep ps;
    int rc;
    if (!i8) HIP_TRY(ctx, hipEventRecord(ctx->ev_k0, ctx->stream));
    if ((rc = sweep_pair(ctx, *q, t, 2, nq, nullptr, i8 ? nullptr : c->st_real(), kSweepNoCount | (i8 ? 0u : kSweepNoEvents), &ps)) != FM_OK) return rc;
    if ((rc = wait_for_stream(ctx, consumer)) != FM_OK) return rc;
    if ((rc = coll_merge_one(ctx, &ps, tab, nq, 0, d_img, d_idx, d_dist)) != FM_OK) return rc;
    if (!i8) {
        HIP_TRY(ctx, hipEventRecord(ctx->ev_k1, ctx->stream));
        ctx->kernel_timed = true;
    }
    if (ps.fix) {
        hipLaunchKernelGGL(coll_sqrt_fix_kernel, dim3(kFixGrid), dim3(256), 0, ctx->stream, (const unsigned*)ps.fix,
                           (const int8_t*)q->rows8, (const int32_t*)q->norm, (const int8_t*)t.rows8, (const int32_t*)t.norm, (int)t.n,
                           tab, (int64_t)0, d_img, d_idx, d_dist);
        HIP_TRY(ctx, hipGetLastError());
    }
    return FM_OK;
}

// fm_collection_knn behind its checks of the handles, the kinds and k (1 .. 8; a wide collection: 1, 2) -- shared with
// fm_collection_wide_knn, whose checks differ and whose sweep coll_knn2_device picks by the collection's kind.
static int coll_knn_host(fm_ctx* ctx, fm_collection* c, const fm_bank* q, int32_t k, int32_t* img, int32_t* idx, float* dist, const char* who)
{
    int rc;
    const int64_t nq = q->n;
    if (nq > 0 && (!img || !idx || !dist)) return fail(ctx, FM_EINVAL, std::string(who) + ": output pointer is NULL");
    if (nq == 0) return FM_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int kk = k < 2 ? 2 : k;
    const size_t ob = align256((size_t)nq * kk * 4), cb = align256((size_t)nq * 4);
    if ((rc = ws_ensure(ctx, &ctx->ws_out, &ctx->ws_out_bytes, 3 * ob + 3 * cb + 64)) != FM_OK) return rc;
    char* b = (char*)ctx->ws_out;
    int32_t* d_img = (int32_t*)b; int32_t* d_idx = (int32_t*)(b + ob); float* d_dist = (float*)(b + 2 * ob);
    int32_t* d_img1 = (int32_t*)(b + 3 * ob); int32_t* d_idx1 = (int32_t*)(b + 3 * ob + cb); float* d_dist1 = (float*)(b + 3 * ob + 2 * cb);
    CallScope cs(ctx);
    if (k <= 2 || c->total == 0) {
        if (k <= 2) {
            if ((rc = coll_knn2_device(ctx, c, q, d_img, d_idx, d_dist)) != FM_OK) return rc;
        } else {
            HIP_TRY(ctx, hipMemsetAsync(d_img, 0xff, (size_t)nq * k * 4, ctx->stream));
            HIP_TRY(ctx, hipMemsetAsync(d_idx, 0xff, (size_t)nq * k * 4, ctx->stream));
            HIP_TRY(ctx, hipMemsetD32Async((hipDeviceptr_t)d_dist, 0x7f800000, (size_t)nq * k, ctx->stream));
        }
        if (k == 1) {
            hipLaunchKernelGGL(coll_col0_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, ctx->stream, (const int32_t*)d_img,
                               (const float*)d_dist, (const int32_t*)d_idx, nq, d_img1, d_dist1, d_idx1);
            HIP_TRY(ctx, hipGetLastError());
            HIP_TRY(ctx, d2h(ctx, img, d_img1, (size_t)nq * 4));
            HIP_TRY(ctx, d2h(ctx, idx, d_idx1, (size_t)nq * 4));
            HIP_TRY(ctx, d2h(ctx, dist, d_dist1, (size_t)nq * 4));
            return cs.finish();
        }
    } else {
        const fm::Bank& t = c->stack;
        if ((rc = ws_ensure(ctx, &ctx->ws_partial, &ctx->ws_partial_bytes, knnk_partial_bytes(nq, t.n, k) + 64)) != FM_OK) return rc;
        HIP_TRY(ctx, hipEventRecord(ctx->ev_k0, ctx->stream));
        if (t.kind == FM_BANK_BIN)
            HIP_TRY(ctx, launch_hamming_knnk(*q, t, k, (unsigned long long*)ctx->ws_partial, d_idx, d_dist, ctx->stream, c->st_real()));
        else
            HIP_TRY(ctx, launch_knnk(*q, t, k, (unsigned long long*)ctx->ws_partial, d_idx, d_dist, ctx->stream));
        HIP_TRY(ctx, hipEventRecord(ctx->ev_k1, ctx->stream));
        ctx->kernel_timed = true;
        ctx->pending_pairs += nq * c->total;
        ctx->pending_bytes += bank_bytes(q) + bank_bytes(static_cast<const fm_bank*>(&t));
        hipLaunchKernelGGL(coll_translate_kernel, dim3((unsigned)((nq * k + 255) / 256)), dim3(256), 0, ctx->stream,
                           CollTab{c->st_img(), c->st_real(), c->img_phys()}, nq * k, d_img, d_idx, d_dist);
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, d2h(ctx, img, d_img, (size_t)nq * k * 4));
    HIP_TRY(ctx, d2h(ctx, idx, d_idx, (size_t)nq * k * 4));
    HIP_TRY(ctx, d2h(ctx, dist, d_dist, (size_t)nq * k * 4));
    return cs.finish();
}

extern "C" int fm_collection_knn(fm_ctx* ctx, fm_collection* c, const fm_bank* q, int32_t k, int32_t* img, int32_t* idx, float* dist)
{
    int rc = coll_query_check(ctx, c, q, "fm_collection_knn");
    if (rc != FM_OK) return rc;
    if (k < 1) return fail(ctx, FM_EINVAL, "fm_collection_knn: k must be at least 1");
    if (k > 8) return fail(ctx, FM_EUNSUPPORTED, "fm_collection_knn: k above 8 is not built");
    return coll_knn_host(ctx, c, q, k, img, idx, dist, "fm_collection_knn");
}

// fm_collection_knn2_ratio behind coll_query_check -- shared with fm_collection_wide_knn2_ratio
static int coll_knn2_ratio_host(fm_ctx* ctx, fm_collection* c, const fm_bank* q, double tau, int64_t cap, int32_t* qidx, int32_t* img,
                                int32_t* tidx, float* dist, double* ratio, int64_t* n_accepted, const char* who)
{
    int rc;
    if (n_accepted) *n_accepted = 0;
    const int64_t nq = q->n;
    if (nq == 0) return FM_OK;
    if (cap < 0 || !qidx || !img || !tidx || !dist || !ratio) return fail(ctx, FM_EINVAL, std::string(who) + ": bad output arguments");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int nblk = (int)((nq + 255) / 256);
    const int64_t ccap = cap < nq ? cap : nq;
    size_t off = 0;
    const size_t o_m2 = carve(off, (size_t)nq * 8), o_i2 = carve(off, (size_t)nq * 8), o_d2 = carve(off, (size_t)nq * 8);
    const size_t o_ti = carve(off, (size_t)nq * 4), o_di = carve(off, (size_t)nq * 4), o_ra = carve(off, (size_t)nq * 8);
    const size_t o_pa = carve(off, (size_t)nq), o_bc = carve(off, (size_t)nblk * 4), o_cnt = carve(off, 16);
    const size_t o_cq = carve(off, (size_t)ccap * 4), o_ct = carve(off, (size_t)ccap * 4), o_cm = carve(off, (size_t)ccap * 4);
    const size_t o_cd = carve(off, (size_t)ccap * 4), o_cr = carve(off, (size_t)ccap * 8);
    if ((rc = ws_ensure(ctx, &ctx->ws_out, &ctx->ws_out_bytes, off + 64)) != FM_OK) return rc;
    char* b = (char*)ctx->ws_out;
    CallScope cs(ctx);
    if ((rc = coll_knn2_device(ctx, c, q, (int32_t*)(b + o_m2), (int32_t*)(b + o_i2), (float*)(b + o_d2))) != FM_OK) return rc;
    // the ratio test of fm_knn2_ratio on the row lists, then the ordered compaction with the image column
    hipLaunchKernelGGL(lowe_kernel, dim3((unsigned)nblk), dim3(256), 0, ctx->stream, (const int32_t*)(b + o_i2), (const float*)(b + o_d2), nq, tau,
                       (int32_t*)(b + o_ti), (float*)(b + o_di), (double*)(b + o_ra), (uint8_t*)(b + o_pa), (int*)(b + o_bc));
    HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(coll_compact_kernel, dim3((unsigned)nblk), dim3(256), 0, ctx->stream, (const int32_t*)(b + o_m2), (const int32_t*)(b + o_ti),
                       (const float*)(b + o_di), (const double*)(b + o_ra), (const uint8_t*)(b + o_pa), (const int*)(b + o_bc), nq, ccap,
                       (int32_t*)(b + o_cq), (int32_t*)(b + o_cm), (int32_t*)(b + o_ct), (float*)(b + o_cd), (double*)(b + o_cr),
                       (unsigned long long*)(b + o_cnt));
    HIP_TRY(ctx, hipGetLastError());
    return cs.finish_rows((const unsigned long long*)(b + o_cnt), ccap,
                          {{qidx, b + o_cq, 4}, {img, b + o_cm, 4}, {tidx, b + o_ct, 4}, {dist, b + o_cd, 4}, {ratio, b + o_cr, 8}}, n_accepted);
}

extern "C" int fm_collection_knn2_ratio(fm_ctx* ctx, fm_collection* c, const fm_bank* q, double tau, int64_t cap,
                                        int32_t* qidx, int32_t* img, int32_t* tidx, float* dist, double* ratio, int64_t* n_accepted)
{
    int rc = coll_query_check(ctx, c, q, "fm_collection_knn2_ratio");
    if (rc != FM_OK) return rc;
    return coll_knn2_ratio_host(ctx, c, q, tau, cap, qidx, img, tidx, dist, ratio, n_accepted, "fm_collection_knn2_ratio");
}

// fm_collection_knn / fm_collection_knn2_ratio with the results left in caller-supplied device memory: the same pipelines, the
// merge / lookup / compaction kernels handed the caller's pointers, ordered against consumer_stream as fm_knn_dev and
// fm_knn2_ratio_dev are (api_match.hip).  Not accounted in fm_stats.
// fm_collection_knn_dev behind its checks of the handles, the kinds and k -- shared with fm_collection_wide_knn_dev
static int coll_knn_dev(fm_ctx* ctx, fm_collection* c, const fm_bank* q, int32_t k, int32_t* d_img, int32_t* d_idx, float* d_dist,
                        void* consumer_stream, const char* who)
{
    int rc;
    const int64_t nq = q->n;
    if (nq == 0) return FM_OK;
    if (!d_img || !d_idx || !d_dist) return fail(ctx, FM_EINVAL, std::string(who) + ": output pointer is NULL");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((rc = check_device_ptr(ctx, d_img, who, "d_img")) != FM_OK || (rc = check_device_ptr(ctx, d_idx, who, "d_idx")) != FM_OK ||
        (rc = check_device_ptr(ctx, d_dist, who, "d_dist")) != FM_OK) return rc;
    if (k == 2) {
        if ((rc = coll_knn2_device(ctx, c, q, d_img, d_idx, d_dist, consumer_stream)) != FM_OK) return rc;
    } else if (k == 1) {
        const size_t ob = align256((size_t)nq * 8);
        if ((rc = ws_ensure(ctx, &ctx->ws_out, &ctx->ws_out_bytes, 3 * ob + 64)) != FM_OK) return rc;
        char* b = (char*)ctx->ws_out;
        if ((rc = coll_knn2_device(ctx, c, q, (int32_t*)b, (int32_t*)(b + ob), (float*)(b + 2 * ob))) != FM_OK) return rc;
        if ((rc = wait_for_stream(ctx, consumer_stream)) != FM_OK) return rc;
        hipLaunchKernelGGL(coll_col0_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, ctx->stream, (const int32_t*)b,
                           (const float*)(b + 2 * ob), (const int32_t*)(b + ob), nq, d_img, d_dist, d_idx);
        HIP_TRY(ctx, hipGetLastError());
    } else if (c->total == 0) {
        if ((rc = wait_for_stream(ctx, consumer_stream)) != FM_OK) return rc;
        HIP_TRY(ctx, hipMemsetAsync(d_img, 0xff, (size_t)nq * k * 4, ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(d_idx, 0xff, (size_t)nq * k * 4, ctx->stream));
        HIP_TRY(ctx, hipMemsetD32Async((hipDeviceptr_t)d_dist, 0x7f800000, (size_t)nq * k, ctx->stream));
    } else {
        // K9 / K11's vector-ALU lists: their merge kernel writes the physical rows into the caller's d_idx, the lookup pass
        // turns them into (image, row) in place
        const fm::Bank& t = c->stack;
        if ((rc = ws_ensure(ctx, &ctx->ws_partial, &ctx->ws_partial_bytes, knnk_partial_bytes(nq, t.n, k) + 64)) != FM_OK) return rc;
        if ((rc = wait_for_stream(ctx, consumer_stream)) != FM_OK) return rc;
        if (t.kind == FM_BANK_BIN)
            HIP_TRY(ctx, launch_hamming_knnk(*q, t, k, (unsigned long long*)ctx->ws_partial, d_idx, d_dist, ctx->stream, c->st_real()));
        else
            HIP_TRY(ctx, launch_knnk(*q, t, k, (unsigned long long*)ctx->ws_partial, d_idx, d_dist, ctx->stream));
        hipLaunchKernelGGL(coll_translate_kernel, dim3((unsigned)((nq * k + 255) / 256)), dim3(256), 0, ctx->stream,
                           CollTab{c->st_img(), c->st_real(), c->img_phys()}, nq * k, d_img, d_idx, d_dist);
        HIP_TRY(ctx, hipGetLastError());
    }
    return results_written(ctx, consumer_stream);
}

extern "C" int fm_collection_knn_dev(fm_ctx* ctx, fm_collection* c, const fm_bank* q, int32_t k, int32_t* d_img, int32_t* d_idx,
                                     float* d_dist, void* consumer_stream)
{
    const char* who = "fm_collection_knn_dev";
    int rc = coll_query_check(ctx, c, q, who);
    if (rc != FM_OK) return rc;
    if (k < 1) return fail(ctx, FM_EINVAL, "fm_collection_knn_dev: k must be at least 1");
    if (k > 8) return fail(ctx, FM_EUNSUPPORTED, "fm_collection_knn_dev: k above 8 is not built");
    return coll_knn_dev(ctx, c, q, k, d_img, d_idx, d_dist, consumer_stream, who);
}

// ---- K13: knnMatch(q, k, masks = [...]) (masked.hip) ---------------------------------------------------------------------------
// The train operand is the stack viewed as one bank; the mask lies on the physical stack and forbids the padding rows behind
// every image itself, so the masked kernels take no real-row table.  The lists come back as physical rows and the lookup
// pass of the k >= 3 path (coll_translate_kernel) turns the nq * k entries into (image, row) for every k.
extern "C" int fm_mask_create_coll(fm_ctx* ctx, int64_t nq, fm_collection* c, fm_mask** mask)
{
    int rc = coll_check(ctx, c, "fm_mask_create_coll");
    if (rc != FM_OK) return rc;
    if (!mask) return fail(ctx, FM_EINVAL, "fm_mask_create_coll: mask out pointer is NULL");
    *mask = nullptr;
    if ((rc = coll_refuse_wide(ctx, c, "fm_mask_create_coll")) != FM_OK) return rc;
    if (nq < 0) return fail(ctx, FM_EINVAL, "fm_mask_create_coll: bad nq");
    if (nq > 0x7fffffff) return fail(ctx, FM_EUNSUPPORTED, "fm_mask_create_coll: more than 2^31 - 1 query rows");
    if ((rc = mask_alloc(ctx, nq, c->rows, c->phys, c->used, "fm_mask_create_coll", mask)) != FM_OK) return rc;
    (*mask)->coll = c;
    (*mask)->coll_gen = c->gen;
    return FM_OK;
}

// Steps 1 .. 4 of the collection forms' error order (the header).
static int coll_masked_check(fm_ctx* ctx, fm_collection* c, const fm_bank* q, const fm_mask* m, int32_t k, const char* who)
{
    if (ctx && c && q && !m) return fail(ctx, FM_EINVAL, std::string(who) + ": mask is NULL");
    int rc = coll_query_check(ctx, c, q, who);
    if (rc != FM_OK) return rc;
    if (k < 1) return fail(ctx, FM_EINVAL, std::string(who) + ": k must be at least 1");
    if (k > 8) return fail(ctx, FM_EUNSUPPORTED, std::string(who) + ": k above 8 is not built");
    if ((rc = mask_check(ctx, m, who)) != FM_OK) return rc;
    if (!m->coll) return fail(ctx, FM_EINVAL, std::string(who) + ": the mask was made for a bank pair (fm_mask_create); a collection takes fm_mask_create_coll's");
    if (m->coll != c) return fail(ctx, FM_EINVAL, std::string(who) + ": the mask was made for another collection");
    if (m->coll_gen != c->gen)
        return fail(ctx, FM_EINVAL, std::string(who) + ": the collection has changed (add or clear) since fm_mask_create_coll: the mask had " +
                                    std::to_string(m->rows.size()) + " images and " + std::to_string(m->nt) + " rows");
    if (m->nq != q->n)
        return fail(ctx, FM_EINVAL, std::string(who) + ": the mask has " + std::to_string(m->nq) + " query rows, the query bank " + std::to_string(q->n));
    return FM_OK;
}

// The masked lists of q against the stack into d_img / d_idx / d_dist [nq][k] (device memory) on the context's stream.
static int coll_knn_masked_device(fm_ctx* ctx, fm_collection* c, const fm_bank* q, const fm_mask* m, int k, int32_t* d_img, int32_t* d_idx, float* d_dist)
{
    const int64_t nq = q->n;
    if (c->total == 0) {
        HIP_TRY(ctx, hipMemsetAsync(d_img, 0xff, (size_t)nq * k * 4, ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(d_idx, 0xff, (size_t)nq * k * 4, ctx->stream));
        HIP_TRY(ctx, hipMemsetD32Async((hipDeviceptr_t)d_dist, 0x7f800000, (size_t)nq * k, ctx->stream));
        return FM_OK;
    }
    int rc = knn_masked_device(ctx, *q, c->stack, m, k, d_idx, d_dist);
    if (rc != FM_OK) return rc;
    hipLaunchKernelGGL(coll_translate_kernel, dim3((unsigned)((nq * k + 255) / 256)), dim3(256), 0, ctx->stream,
                       CollTab{c->st_img(), c->st_real(), c->img_phys()}, nq * k, d_img, d_idx, d_dist);
    HIP_TRY(ctx, hipGetLastError());
    return FM_OK;
}

extern "C" int fm_collection_knn_masked(fm_ctx* ctx, fm_collection* c, const fm_bank* q, const fm_mask* mask, int32_t k,
                                        int32_t* img, int32_t* idx, float* dist)
{
    int rc = coll_masked_check(ctx, c, q, mask, k, "fm_collection_knn_masked");
    if (rc != FM_OK) return rc;
    const int64_t nq = q->n;
    if (nq > 0 && (!img || !idx || !dist)) return fail(ctx, FM_EINVAL, "fm_collection_knn_masked: output pointer is NULL");
    if (nq == 0) return FM_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t ob = align256((size_t)nq * k * 4);
    if ((rc = ws_ensure(ctx, &ctx->ws_out, &ctx->ws_out_bytes, 3 * ob + 64)) != FM_OK) return rc;
    char* b = (char*)ctx->ws_out;
    int32_t* d_img = (int32_t*)b; int32_t* d_idx = (int32_t*)(b + ob); float* d_dist = (float*)(b + 2 * ob);
    CallScope cs(ctx);
    HIP_TRY(ctx, hipEventRecord(ctx->ev_k0, ctx->stream));
    if ((rc = coll_knn_masked_device(ctx, c, q, mask, k, d_img, d_idx, d_dist)) != FM_OK) return rc;
    HIP_TRY(ctx, hipEventRecord(ctx->ev_k1, ctx->stream));
    ctx->kernel_timed = true;
    ctx->pending_pairs += nq * c->total;
    ctx->pending_bytes += bank_bytes(q) + bank_bytes(static_cast<const fm_bank*>(&c->stack));
    HIP_TRY(ctx, d2h(ctx, img, d_img, (size_t)nq * k * 4));
    HIP_TRY(ctx, d2h(ctx, idx, d_idx, (size_t)nq * k * 4));
    HIP_TRY(ctx, d2h(ctx, dist, d_dist, (size_t)nq * k * 4));
    return cs.finish();
}

extern "C" int fm_collection_knn_masked_dev(fm_ctx* ctx, fm_collection* c, const fm_bank* q, const fm_mask* mask, int32_t k,
                                            int32_t* d_img, int32_t* d_idx, float* d_dist, void* consumer_stream)
{
    const char* who = "fm_collection_knn_masked_dev";
    int rc = coll_masked_check(ctx, c, q, mask, k, who);
    if (rc != FM_OK) return rc;
    const int64_t nq = q->n;
    if (nq == 0) return FM_OK;
    if (!d_img || !d_idx || !d_dist) return fail(ctx, FM_EINVAL, "fm_collection_knn_masked_dev: output pointer is NULL");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((rc = check_device_ptr(ctx, d_img, who, "d_img")) != FM_OK || (rc = check_device_ptr(ctx, d_idx, who, "d_idx")) != FM_OK ||
        (rc = check_device_ptr(ctx, d_dist, who, "d_dist")) != FM_OK) return rc;
    if ((rc = wait_for_stream(ctx, consumer_stream)) != FM_OK) return rc;
    if ((rc = coll_knn_masked_device(ctx, c, q, mask, k, d_img, d_idx, d_dist)) != FM_OK) return rc;
    return results_written(ctx, consumer_stream);
}

// fm_collection_knn2_ratio_dev behind coll_query_check -- shared with fm_collection_wide_knn2_ratio_dev
static int coll_knn2_ratio_dev(fm_ctx* ctx, fm_collection* c, const fm_bank* q, double tau, int64_t cap, int32_t* d_rows, int64_t* d_count,
                               int64_t* n_accepted, void* consumer_stream, const char* who)
{
    int rc;
    if (n_accepted) *n_accepted = 0;
    if (cap < 0 || !d_count || (cap > 0 && !d_rows)) return fail(ctx, FM_EINVAL, std::string(who) + ": bad output arguments");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((rc = check_device_ptr(ctx, d_count, who, "d_count")) != FM_OK) return rc;
    if (cap > 0 && (rc = check_device_ptr(ctx, d_rows, who, "d_rows")) != FM_OK) return rc;
    const int64_t nq = q->n;
    if (nq == 0) {
        if ((rc = wait_for_stream(ctx, consumer_stream)) != FM_OK) return rc;
        HIP_TRY(ctx, hipMemsetAsync(d_count, 0, 8, ctx->stream));
        return results_written(ctx, consumer_stream);
    }
    const int nblk = (int)((nq + 255) / 256);
    size_t off = 0;
    const size_t o_m2 = carve(off, (size_t)nq * 8), o_i2 = carve(off, (size_t)nq * 8), o_d2 = carve(off, (size_t)nq * 8);
    const size_t o_ti = carve(off, (size_t)nq * 4), o_di = carve(off, (size_t)nq * 4), o_ra = carve(off, (size_t)nq * 8);
    const size_t o_pa = carve(off, (size_t)nq), o_bc = carve(off, (size_t)nblk * 4), o_cnt = carve(off, 16);
    if ((rc = ws_ensure(ctx, &ctx->ws_out, &ctx->ws_out_bytes, off + 64)) != FM_OK) return rc;
    char* b = (char*)ctx->ws_out;
    if ((rc = coll_knn2_device(ctx, c, q, (int32_t*)(b + o_m2), (int32_t*)(b + o_i2), (float*)(b + o_d2))) != FM_OK) return rc;
    hipLaunchKernelGGL(lowe_kernel, dim3((unsigned)nblk), dim3(256), 0, ctx->stream, (const int32_t*)(b + o_i2), (const float*)(b + o_d2), nq, tau,
                       (int32_t*)(b + o_ti), (float*)(b + o_di), (double*)(b + o_ra), (uint8_t*)(b + o_pa), (int*)(b + o_bc));
    HIP_TRY(ctx, hipGetLastError());
    if ((rc = wait_for_stream(ctx, consumer_stream)) != FM_OK) return rc;
    hipLaunchKernelGGL(coll_compact_rows_kernel, dim3((unsigned)nblk), dim3(256), 0, ctx->stream, (const int32_t*)(b + o_m2),
                       (const int32_t*)(b + o_ti), (const float*)(b + o_di), (const uint8_t*)(b + o_pa), (const int*)(b + o_bc), nq, cap, d_rows,
                       (long long*)d_count, (unsigned long long*)(b + o_cnt));
    HIP_TRY(ctx, hipGetLastError());
    if ((rc = results_written(ctx, consumer_stream)) != FM_OK) return rc;
    if (n_accepted) {       // (the one host synchronisation of the integer and binary routes: the caller asked for a host number)
        unsigned long long cnt = 0;
        HIP_TRY(ctx, hipMemcpyAsync(&cnt, b + o_cnt, 8, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        *n_accepted = (int64_t)cnt;
    }
    return FM_OK;
}

extern "C" int fm_collection_knn2_ratio_dev(fm_ctx* ctx, fm_collection* c, const fm_bank* q, double tau, int64_t cap, int32_t* d_rows,
                                            int64_t* d_count, int64_t* n_accepted, void* consumer_stream)
{
    const char* who = "fm_collection_knn2_ratio_dev";
    int rc = coll_query_check(ctx, c, q, who);
    if (rc != FM_OK) return rc;
    return coll_knn2_ratio_dev(ctx, c, q, tau, cap, d_rows, d_count, n_accepted, consumer_stream, who);
}

// radiusMatch against the stacked images (K10, radius.hip): the stack is the train bank of ONE sweep whose epilogue masks
// the padding rows by index (st_real), and the compaction turns a key's physical row into (image, row).  Host arrays, or
// (dev) the caller's device arrays.
// ham: the Hamming entry points (fm_collection_hamming_radius_match(_dev)) -- a binary query against a binary collection;
// the L2-named ones keep refusing a binary collection.
static int coll_radius(fm_ctx* ctx, fm_collection* c, const fm_bank* q, const float* radius, float radius_all, int64_t cap, int64_t* offsets,
                       int32_t* img, int32_t* idx, float* dist, int64_t* n_total, bool dev, void* consumer, const char* who, bool ham = false)
{
    int rc = coll_query_check(ctx, c, q, who, true);
    if (rc != FM_OK) return rc;
    if (!ham && c->dim != 0 && c->stack.kind == FM_BANK_BIN)
        return fail(ctx, FM_EUNSUPPORTED, std::string(who) + ": Hamming radiusMatch is not built here (binary collection): "
                                          "fm_collection_hamming_radius_match serves it");
    if (ham && (q->kind != FM_BANK_BIN || (c->dim != 0 && c->stack.kind != FM_BANK_BIN)))
        return fail(ctx, FM_EINVAL, std::string(who) + ": the query bank and the collection must be binary (FM_BANK_BIN); "
                                    "fm_collection_radius_match is the L2 call");
    if (cap < 0) return fail(ctx, FM_EINVAL, std::string(who) + ": cap is negative");
    if (!offsets) return fail(ctx, FM_EINVAL, std::string(who) + ": offsets is NULL");
    if (cap > 0 && (!img || !idx || !dist)) return fail(ctx, FM_EINVAL, std::string(who) + ": img / idx / dist is NULL with cap > 0");
    if (dev) {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        if (radius && (rc = check_device_ptr(ctx, radius, who, "d_radius")) != FM_OK) return rc;
        if ((rc = check_device_ptr(ctx, offsets, who, "d_offsets")) != FM_OK) return rc;
        if (img && (rc = check_device_ptr(ctx, img, who, "d_img")) != FM_OK) return rc;
        if (idx && (rc = check_device_ptr(ctx, idx, who, "d_idx")) != FM_OK) return rc;
        if (dist && (rc = check_device_ptr(ctx, dist, who, "d_dist")) != FM_OK) return rc;
    }
    const CollTab tab{c->st_img(), c->st_real(), c->img_phys()};
    const RadiusArgs a{who, radius, radius_all, cap, offsets, img, idx, dist, n_total, dev, consumer, &tab, c->total};
    return radius_match(ctx, *q, c->stack, a);
}

extern "C" int fm_collection_radius_match(fm_ctx* ctx, fm_collection* c, const fm_bank* q, const float* radius, float radius_all, int64_t cap,
                                          int64_t* offsets, int32_t* img, int32_t* idx, float* dist, int64_t* n_total)
{
    return coll_radius(ctx, c, q, radius, radius_all, cap, offsets, img, idx, dist, n_total, false, FM_NO_STREAM, "fm_collection_radius_match");
}

extern "C" int fm_collection_radius_match_dev(fm_ctx* ctx, fm_collection* c, const fm_bank* q, const float* d_radius, float radius_all,
                                              int64_t cap, int64_t* d_offsets, int32_t* d_img, int32_t* d_idx, float* d_dist,
                                              int64_t* n_total, void* consumer_stream)
{
    return coll_radius(ctx, c, q, d_radius, radius_all, cap, d_offsets, d_img, d_idx, d_dist, n_total, true, consumer_stream,
                       "fm_collection_radius_match_dev");
}

extern "C" int fm_collection_hamming_radius_match(fm_ctx* ctx, fm_collection* c, const fm_bank* q, const float* radius, float radius_all,
                                                  int64_t cap, int64_t* offsets, int32_t* img, int32_t* idx, float* dist, int64_t* n_total)
{
    return coll_radius(ctx, c, q, radius, radius_all, cap, offsets, img, idx, dist, n_total, false, FM_NO_STREAM,
                       "fm_collection_hamming_radius_match", true);
}

extern "C" int fm_collection_hamming_radius_match_dev(fm_ctx* ctx, fm_collection* c, const fm_bank* q, const float* d_radius, float radius_all,
                                                      int64_t cap, int64_t* d_offsets, int32_t* d_img, int32_t* d_idx, float* d_dist,
                                                      int64_t* n_total, void* consumer_stream)
{
    return coll_radius(ctx, c, q, d_radius, radius_all, cap, d_offsets, d_img, d_idx, d_dist, n_total, true, consumer_stream,
                       "fm_collection_hamming_radius_match_dev", true);
}

// Masked radiusMatch against the stacked images (radius.hip's masked sweeps): integer, float32 and binary collections under one
// name, the route chosen by the query bank's kind as radius_match chooses it.  A wide collection is refused by
// coll_query_check (FM_EUNSUPPORTED; fm_mask_create_coll makes no mask for one either).  Checks in the header's order: handles,
// the collection and its query, the mask (fm_collection_knn_masked's), cap and the outputs.  The sweeps keep testing st_real
// beside the mask although the mask's padding bits are 0 already: one uniform table word per stage, and the same code as
// the unmasked sweeps'.
static int coll_radius_masked(fm_ctx* ctx, fm_collection* c, const fm_bank* q, const fm_mask* m, const float* radius, float radius_all, int64_t cap,
                              int64_t* offsets, int32_t* img, int32_t* idx, float* dist, int64_t* n_total, bool dev, void* consumer, const char* who)
{
    if (ctx && c && q && !m) return fail(ctx, FM_EINVAL, std::string(who) + ": mask is NULL");
    int rc = coll_query_check(ctx, c, q, who, true);
    if (rc != FM_OK) return rc;
    if ((rc = mask_check(ctx, m, who)) != FM_OK) return rc;
    if (!m->coll) return fail(ctx, FM_EINVAL, std::string(who) + ": the mask was made for a bank pair (fm_mask_create); a collection takes fm_mask_create_coll's");
    if (m->coll != c) return fail(ctx, FM_EINVAL, std::string(who) + ": the mask was made for another collection");
    if (m->coll_gen != c->gen)
        return fail(ctx, FM_EINVAL, std::string(who) + ": the collection has changed (add or clear) since fm_mask_create_coll: the mask had " +
                                    std::to_string(m->rows.size()) + " images and " + std::to_string(m->nt) + " rows");
    if (m->nq != q->n)
        return fail(ctx, FM_EINVAL, std::string(who) + ": the mask has " + std::to_string(m->nq) + " query rows, the query bank " + std::to_string(q->n));
    const char* pre = dev ? "d_" : "";
    if (cap < 0) return fail(ctx, FM_EINVAL, std::string(who) + ": cap is negative");
    if (!offsets) return fail(ctx, FM_EINVAL, std::string(who) + ": " + pre + "offsets is NULL");
    if (cap > 0 && (!img || !idx || !dist)) return fail(ctx, FM_EINVAL, std::string(who) + ": img / idx / dist is NULL with cap > 0");
    if (dev) {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        if (radius && (rc = check_device_ptr(ctx, radius, who, "d_radius")) != FM_OK) return rc;
        if ((rc = check_device_ptr(ctx, offsets, who, "d_offsets")) != FM_OK) return rc;
        if (img && (rc = check_device_ptr(ctx, img, who, "d_img")) != FM_OK) return rc;
        if (idx && (rc = check_device_ptr(ctx, idx, who, "d_idx")) != FM_OK) return rc;
        if (dist && (rc = check_device_ptr(ctx, dist, who, "d_dist")) != FM_OK) return rc;
    }
    const CollTab tab{c->st_img(), c->st_real(), c->img_phys()};
    const RadiusArgs a{who, radius, radius_all, cap, offsets, img, idx, dist, n_total, dev, consumer, &tab, c->total, m->bits, m->words};
    return radius_match(ctx, *q, c->stack, a);
}

extern "C" int fm_collection_radius_match_masked(fm_ctx* ctx, fm_collection* c, const fm_bank* q, const fm_mask* mask, const float* radius,
                                                 float radius_all, int64_t cap, int64_t* offsets, int32_t* img, int32_t* idx, float* dist,
                                                 int64_t* n_total)
{
    return coll_radius_masked(ctx, c, q, mask, radius, radius_all, cap, offsets, img, idx, dist, n_total, false, FM_NO_STREAM,
                              "fm_collection_radius_match_masked");
}

extern "C" int fm_collection_radius_match_masked_dev(fm_ctx* ctx, fm_collection* c, const fm_bank* q, const fm_mask* mask, const float* d_radius,
                                                     float radius_all, int64_t cap, int64_t* d_offsets, int32_t* d_img, int32_t* d_idx,
                                                     float* d_dist, int64_t* n_total, void* consumer_stream)
{
    return coll_radius_masked(ctx, c, q, mask, d_radius, radius_all, cap, d_offsets, d_img, d_idx, d_dist, n_total, true, consumer_stream,
                              "fm_collection_radius_match_masked_dev");
}

// Wide radiusMatch against the stacked images of a WIDE collection (radius.hip, the wide route): the stack is the train bank of
// one sweep, its padding rows masked by index through the stage table fm_collection_train builds for every kind.  The
// L2-named calls above keep refusing a wide collection (coll_query_check); these are the ones that serve it.  Checks in the
// header's order: handles, the kinds (coll_query_check refuses wide data and is not asked), the widths, cap and the outputs.
// The stack's scale and largest scaled squared norm are read by radius_match at this call: a later add may rewrite them.
static int coll_wide_radius(fm_ctx* ctx, fm_collection* c, const fm_bank* q, const float* radius, float radius_all, int64_t cap, int64_t* offsets,
                            int32_t* img, int32_t* idx, float* dist, int64_t* n_total, bool dev, void* consumer, const char* who_)
{
    const std::string who(who_);
    int rc = coll_check(ctx, c, who_);
    if (rc != FM_OK) return rc;
    if (!q) return fail(ctx, FM_EINVAL, who + ": query bank is NULL");
    if ((rc = refuse_bin2(ctx, q, who_)) != FM_OK) return rc;
    const bool cbin = c->dim != 0 && c->stack.kind == FM_BANK_BIN && !coll_is_wide(c);
    if (q->kind != FM_BANK_F32W || (!c->rows.empty() && !coll_is_wide(c)))
        return fail(ctx, FM_EINVAL, who + ": the collection and the query bank must be wide float (fm_collection_add_wide; FM_BANK_F32W: "
                                          "fm_bank_create_f32 with 129 .. 256 values per row); " +
                                          ((q->kind == FM_BANK_BIN || cbin) ? "fm_collection_hamming_radius_match is the Hamming call"
                                                                            : "fm_collection_radius_match is the L2 call"));
    if (c->dim != 0 && q->dim != c->dim) return fail(ctx, FM_EINVAL, who + ": the query's width differs from the collection's");
    if (cap < 0) return fail(ctx, FM_EINVAL, who + ": cap is negative");
    if (!offsets) return fail(ctx, FM_EINVAL, who + ": offsets is NULL");
    if (cap > 0 && (!img || !idx || !dist)) return fail(ctx, FM_EINVAL, who + ": img / idx / dist is NULL with cap > 0");
    if (dev) {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        if (radius && (rc = check_device_ptr(ctx, radius, who_, "d_radius")) != FM_OK) return rc;
        if ((rc = check_device_ptr(ctx, offsets, who_, "d_offsets")) != FM_OK) return rc;
        if (img && (rc = check_device_ptr(ctx, img, who_, "d_img")) != FM_OK) return rc;
        if (idx && (rc = check_device_ptr(ctx, idx, who_, "d_idx")) != FM_OK) return rc;
        if (dist && (rc = check_device_ptr(ctx, dist, who_, "d_dist")) != FM_OK) return rc;
    }
    if ((rc = fm_collection_train(ctx, c)) != FM_OK) return rc;
    const CollTab tab{c->st_img(), c->st_real(), c->img_phys()};
    const RadiusArgs a{who_, radius, radius_all, cap, offsets, img, idx, dist, n_total, dev, consumer, &tab, c->total};
    return radius_match(ctx, *q, c->stack, a);
}

extern "C" int fm_collection_wide_radius_match(fm_ctx* ctx, fm_collection* c, const fm_bank* q, const float* radius, float radius_all,
                                               int64_t cap, int64_t* offsets, int32_t* img, int32_t* idx, float* dist, int64_t* n_total)
{
    return coll_wide_radius(ctx, c, q, radius, radius_all, cap, offsets, img, idx, dist, n_total, false, FM_NO_STREAM,
                            "fm_collection_wide_radius_match");
}

extern "C" int fm_collection_wide_radius_match_dev(fm_ctx* ctx, fm_collection* c, const fm_bank* q, const float* d_radius, float radius_all,
                                                   int64_t cap, int64_t* d_offsets, int32_t* d_img, int32_t* d_idx, float* d_dist,
                                                   int64_t* n_total, void* consumer_stream)
{
    return coll_wide_radius(ctx, c, q, d_radius, radius_all, cap, d_offsets, d_img, d_idx, d_dist, n_total, true, consumer_stream,
                            "fm_collection_wide_radius_match_dev");
}

// The per-image 2-NN lists on the device: d_idx / d_dist [n_images][nq][2].  Up to "batch_group" images per launch of the
// batched top-2 sweep, every image under its own plan in the batched shape (4 blocks per wave, 8 waves, three stage
// buffers, LDS-DMA staging -- whatever the shape options say: results do not depend on them); one merge launch per sweep
// launch.  The launches follow each other on the context's stream and share one workspace.
static int coll_each_device(fm_ctx* ctx, fm_collection* c, const fm_bank* q, int32_t* d_idx, float* d_dist)
{
    const int64_t nq = q->n;
    const int ni = (int)c->rows.size();
    if (c->stack.kind != FM_BANK_I8 && c->total > 0) {
        // float32-route and binary collections: the per-image sweeps (K8 / K5, K11) enqueued back to back, each followed by its
        // merge -- one stream, one workspace, no host synchronisation between images
        HIP_TRY(ctx, hipEventRecord(ctx->ev_k0, ctx->stream));
        for (int i = 0; i < ni; ++i) {
            const fm::Bank v = coll_view(c, i);
            PairSweep ps;
            int rc;
            if (v.n > 0 && (rc = sweep_pair(ctx, *q, v, 2, 0, nullptr, nullptr, kSweepNoEvents, &ps)) != FM_OK) return rc;
            if ((rc = coll_merge_one(ctx, v.n > 0 ? &ps : nullptr, CollTab{nullptr, nullptr, nullptr}, nq, (int64_t)i * nq, nullptr, d_idx, d_dist)) != FM_OK)
                return rc;
        }
        HIP_TRY(ctx, hipEventRecord(ctx->ev_k1, ctx->stream));
        ctx->kernel_timed = true;
        return FM_OK;
    }
    int group = ctx->tune.batch_group;
    if (group < 1) group = 1;
    if (group > kRRBatchMax) group = kRRBatchMax;
    Tuning shaped = ctx->tune;
    shaped.nb = 4; shaped.nw = 8; shaped.nbuf = 0; shaped.nsplit = 0; shaped.k1_order = 0;
    // workspace of one launch: per slot partial | bounds | fix list, sized for the largest image
    int64_t max_pad = kStageRows;
    for (int i = 0; i < ni; ++i) max_pad = std::max<int64_t>(max_pad, pad128(c->rows[(size_t)i]));
    const RowReducePlan big = plan_rowreduce(q->n_pad, max_pad, shaped);
    size_t slot_p = 0;
    for (int i = 0; i < ni; ++i) {           // (the split count is not monotonic in the image size: take the maximum)
        if (c->rows[(size_t)i] == 0) continue;
        const RowReducePlan p = plan_rowreduce(q->n_pad, pad128(c->rows[(size_t)i]), shaped);
        slot_p = std::max(slot_p, align256(p.partial_bytes(2)));
    }
    const size_t slot_b = align256(big.bound_bytes()), slot_f = align256(fix_bytes(nq));
    const size_t slot = slot_p + slot_b + slot_f;
    int rc = ws_ensure(ctx, &ctx->ws_partial, &ctx->ws_partial_bytes, slot * (size_t)group + 64);
    if (rc != FM_OK) return rc;
    bool timed = false;
    for (int i0 = 0; i0 < ni; i0 += group) {
        const int g = std::min(group, ni - i0);
        fm::Bank views[kRRBatchMax];
        const fm::Bank* cols[kRRBatchMax]; const fm::Bank* red[kRRBatchMax];
        RowReducePlan plans[kRRBatchMax];
        unsigned long long* parts[kRRBatchMax]; int* bounds[kRRBatchMax];
        int slot_of[kRRBatchMax];
        CollMerge mg{};
        int nl = 0;
        for (int j = 0; j < g; ++j) {
            const int i = i0 + j;
            const int64_t n = c->rows[(size_t)i];
            CollSlot& sl = mg.s[j];
            sl.out = (int64_t)i * nq;
            sl.partial = nullptr; sl.nsplit = 0; sl.ncols_alloc = 0; sl.fix = nullptr;
            if (n == 0) continue;
            char* base = (char*)ctx->ws_partial + slot * (size_t)j;
            fm::Bank& v = views[nl];
            v = coll_view(c, i);
            plans[nl] = plan_rowreduce(q->n_pad, v.n_pad, shaped);
            cols[nl] = q; red[nl] = &v;
            parts[nl] = (unsigned long long*)base;
            bounds[nl] = nullptr;
            if (ctx->tune.coop != 0 && plans[nl].nsplit > 1) {
                bounds[nl] = (int*)(base + slot_p);
                HIP_TRY(ctx, hipMemsetD32Async((hipDeviceptr_t)bounds[nl], (int)0x80000000, (size_t)plans[nl].ncols_alloc * 2, ctx->stream));
            }
            sl.partial = parts[nl]; sl.nsplit = plans[nl].nsplit; sl.ncols_alloc = plans[nl].ncols_alloc;
            if (sqrt_tie_possible(*q, v)) {
                sl.fix = (unsigned*)(base + slot_p + slot_b);
                HIP_TRY(ctx, hipMemsetAsync(sl.fix, 0, 16, ctx->stream));
            }
            slot_of[nl] = j;
            ctx->pending_pairs += nq * n;
            ctx->pending_bytes += bank_bytes(q) + v.n * 128;
            ++nl;
        }
        if (nl > 0) {
            if (!timed) HIP_TRY(ctx, hipEventRecord(ctx->ev_k0, ctx->stream));
            HIP_TRY(ctx, launch_rowreduce_batch2(nl, cols, red, plans, parts, bounds, ctx->stream));
            timed = true;
        }
        hipLaunchKernelGGL(coll_merge2_kernel, dim3((unsigned)((nq + 255) / 256), (unsigned)g), dim3(256), 0, ctx->stream, mg,
                           CollTab{nullptr, nullptr, nullptr}, nq, (int32_t*)nullptr, d_idx, d_dist, 0);
        HIP_TRY(ctx, hipGetLastError());
        for (int l = 0; l < nl; ++l) {
            const CollSlot& sl = mg.s[slot_of[l]];
            if (!sl.fix) continue;
            hipLaunchKernelGGL(coll_sqrt_fix_kernel, dim3(kFixGrid), dim3(256), 0, ctx->stream, (const unsigned*)sl.fix,
                               (const int8_t*)q->rows8, (const int32_t*)q->norm, (const int8_t*)views[l].rows8, (const int32_t*)views[l].norm,
                               (int)views[l].n, CollTab{nullptr, nullptr, nullptr}, sl.out, (int32_t*)nullptr, d_idx, d_dist);
            HIP_TRY(ctx, hipGetLastError());
        }
    }
    if (timed) {
        HIP_TRY(ctx, hipEventRecord(ctx->ev_k1, ctx->stream));       // (the sweeps and the merges between them)
        ctx->kernel_timed = true;
    }
    return FM_OK;
}

extern "C" int fm_collection_knn2_each(fm_ctx* ctx, fm_collection* c, const fm_bank* q, int32_t* idx, float* dist)
{
    int rc = coll_query_check(ctx, c, q, "fm_collection_knn2_each");
    if (rc != FM_OK) return rc;
    const int64_t nq = q->n, ni = (int64_t)c->rows.size();
    if (nq == 0 || ni == 0) return FM_OK;
    if (!idx || !dist) return fail(ctx, FM_EINVAL, "fm_collection_knn2_each: output pointer is NULL");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t ob = align256((size_t)ni * nq * 8);
    if ((rc = ws_ensure(ctx, &ctx->ws_out, &ctx->ws_out_bytes, 2 * ob + 64)) != FM_OK) return rc;
    int32_t* d_idx = (int32_t*)ctx->ws_out;
    float* d_dist = (float*)((char*)ctx->ws_out + ob);
    CallScope cs(ctx);
    if ((rc = coll_each_device(ctx, c, q, d_idx, d_dist)) != FM_OK) return rc;
    // (copies of up to 128 MB each keep the staging buffer of fm::d2h within bounds)
    const size_t total = (size_t)ni * nq * 8, piece = (size_t)128 << 20;
    for (size_t o = 0; o < total; o += piece) {
        const size_t nb = std::min(piece, total - o);
        HIP_TRY(ctx, d2h(ctx, (char*)idx + o, (char*)d_idx + o, nb));
        HIP_TRY(ctx, d2h(ctx, (char*)dist + o, (char*)d_dist + o, nb));
    }
    return cs.finish();
}

// fm_collection_votes behind its checks of the handles and the kinds -- shared with fm_collection_wide_votes.  A wide
// collection's per-image lists (mode 1) are those behind fm_collection_wide_knn2_each, counted where they lie (api_pairs.hip).
static int coll_votes_host(fm_ctx* ctx, fm_collection* c, const fm_bank* q, double tau, int32_t mode, int64_t* votes, const char* who)
{
    int rc;
    if (mode != 0 && mode != 1) return fail(ctx, FM_EINVAL, std::string(who) + ": mode must be 0 (stacked lists) or 1 (per-image lists)");
    const int64_t nq = q->n, ni = (int64_t)c->rows.size();
    if (ni == 0) return FM_OK;
    if (!votes) return fail(ctx, FM_EINVAL, std::string(who) + ": votes is NULL");
    for (int64_t i = 0; i < ni; ++i) votes[i] = 0;
    if (nq == 0) return FM_OK;
    if (mode == 1 && coll_is_wide(c)) return coll_wide_each_votes(ctx, c, q, tau, votes);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t vb = align256((size_t)ni * 8);
    const size_t lb = align256((size_t)(mode == 0 ? 1 : ni) * nq * 8);
    if ((rc = ws_ensure(ctx, &ctx->ws_out, &ctx->ws_out_bytes, vb + 3 * lb + 64)) != FM_OK) return rc;
    char* b = (char*)ctx->ws_out;
    unsigned long long* d_votes = (unsigned long long*)b;
    int32_t* d_idx = (int32_t*)(b + vb); float* d_dist = (float*)(b + vb + lb); int32_t* d_img = (int32_t*)(b + vb + 2 * lb);
    CallScope cs(ctx);
    HIP_TRY(ctx, hipMemsetAsync(d_votes, 0, (size_t)ni * 8, ctx->stream));
    if (mode == 0) {
        if ((rc = coll_knn2_device(ctx, c, q, d_img, d_idx, d_dist)) != FM_OK) return rc;
        hipLaunchKernelGGL(coll_votes_kernel, dim3((unsigned)((nq + 255) / 256), 1), dim3(256), 0, ctx->stream, (const int32_t*)d_img,
                           (const int32_t*)d_idx, (const float*)d_dist, nq, tau, d_votes);
    } else {
        if ((rc = coll_each_device(ctx, c, q, d_idx, d_dist)) != FM_OK) return rc;
        hipLaunchKernelGGL(coll_votes_kernel, dim3((unsigned)((nq + 255) / 256), (unsigned)ni), dim3(256), 0, ctx->stream, (const int32_t*)nullptr,
                           (const int32_t*)d_idx, (const float*)d_dist, nq, tau, d_votes);
    }
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, d2h(ctx, votes, d_votes, (size_t)ni * 8));
    return cs.finish();
}

extern "C" int fm_collection_votes(fm_ctx* ctx, fm_collection* c, const fm_bank* q, double tau, int32_t mode, int64_t* votes)
{
    int rc = coll_query_check(ctx, c, q, "fm_collection_votes");
    if (rc != FM_OK) return rc;
    return coll_votes_host(ctx, c, q, tau, mode, votes, "fm_collection_votes");
}

// ---------------------------------------------------------------------------------------
// Wide stacked knnMatch: fm_collection_wide_knn(_dev), fm_collection_wide_knn2_ratio(_dev), fm_collection_wide_votes
// ---------------------------------------------------------------------------------------
// cv2.BFMatcher.add(images) + knnMatch(query, k) against ALL images of a WIDE collection at once: the calls above under names
// of their own, as every wide feature has come.  The L2-named calls keep refusing a wide collection and a wide query bank
// (coll_query_check); these run the same pipelines -- merge, ratio test, compaction, votes -- behind K14's sweep over the
// stack (coll_wide_knn2_device; the kernels and why the bank-pair ones cannot serve: wide_stack.hip).
// Steps 1 .. 3 of the header's error order: the handles, the kinds, the widths.  Then the tables (fm_collection_train).
static int coll_wide_stack_check(fm_ctx* ctx, fm_collection* c, const fm_bank* q, const char* who_, const char* narrow)
{
    const std::string who(who_);
    int rc = coll_check(ctx, c, who_);
    if (rc != FM_OK) return rc;
    if (!q) return fail(ctx, FM_EINVAL, who + ": query bank is NULL");
    if ((rc = refuse_bin2(ctx, q, who_)) != FM_OK) return rc;
    if (q->kind != FM_BANK_F32W || (!c->rows.empty() && !coll_is_wide(c)))
        return fail(ctx, FM_EINVAL, who + ": the collection and the query bank must be wide float (fm_collection_add_wide; FM_BANK_F32W: "
                                          "fm_bank_create_f32 with 129 .. 256 values per row); " + narrow +
                                          " is the call that serves the L2 kinds and the binary (Hamming) kind");
    if (c->dim != 0 && q->dim != c->dim) return fail(ctx, FM_EINVAL, who + ": the query's width differs from the collection's");
    return fm_collection_train(ctx, c);
}

static int coll_wide_k_check(fm_ctx* ctx, int32_t k, const char* who)
{
    if (k < 1) return fail(ctx, FM_EINVAL, std::string(who) + ": k must be at least 1");
    if (k > 2) return fail(ctx, FM_EUNSUPPORTED, std::string(who) + ": k >= 3 is not built for wide float banks (fm_knn serves them with k <= 2 too)");
    return FM_OK;
}

extern "C" int fm_collection_wide_knn(fm_ctx* ctx, fm_collection* c, const fm_bank* q, int32_t k, int32_t* img, int32_t* idx, float* dist)
{
    const char* who = "fm_collection_wide_knn";
    int rc = coll_wide_stack_check(ctx, c, q, who, "fm_collection_knn");
    if (rc != FM_OK || (rc = coll_wide_k_check(ctx, k, who)) != FM_OK) return rc;
    return coll_knn_host(ctx, c, q, k, img, idx, dist, who);
}

extern "C" int fm_collection_wide_knn_dev(fm_ctx* ctx, fm_collection* c, const fm_bank* q, int32_t k, int32_t* d_img, int32_t* d_idx,
                                          float* d_dist, void* consumer_stream)
{
    const char* who = "fm_collection_wide_knn_dev";
    int rc = coll_wide_stack_check(ctx, c, q, who, "fm_collection_knn_dev");
    if (rc != FM_OK || (rc = coll_wide_k_check(ctx, k, who)) != FM_OK) return rc;
    return coll_knn_dev(ctx, c, q, k, d_img, d_idx, d_dist, consumer_stream, who);
}

extern "C" int fm_collection_wide_knn2_ratio(fm_ctx* ctx, fm_collection* c, const fm_bank* q, double tau, int64_t cap, int32_t* qidx,
                                             int32_t* img, int32_t* tidx, float* dist, double* ratio, int64_t* n_accepted)
{
    const char* who = "fm_collection_wide_knn2_ratio";
    int rc = coll_wide_stack_check(ctx, c, q, who, "fm_collection_knn2_ratio");
    if (rc != FM_OK) return rc;
    return coll_knn2_ratio_host(ctx, c, q, tau, cap, qidx, img, tidx, dist, ratio, n_accepted, who);
}

extern "C" int fm_collection_wide_knn2_ratio_dev(fm_ctx* ctx, fm_collection* c, const fm_bank* q, double tau, int64_t cap, int32_t* d_rows,
                                                 int64_t* d_count, int64_t* n_accepted, void* consumer_stream)
{
    const char* who = "fm_collection_wide_knn2_ratio_dev";
    int rc = coll_wide_stack_check(ctx, c, q, who, "fm_collection_knn2_ratio_dev");
    if (rc != FM_OK) return rc;
    return coll_knn2_ratio_dev(ctx, c, q, tau, cap, d_rows, d_count, n_accepted, consumer_stream, who);
}

extern "C" int fm_collection_wide_votes(fm_ctx* ctx, fm_collection* c, const fm_bank* q, double tau, int32_t mode, int64_t* votes)
{
    const char* who = "fm_collection_wide_votes";
    int rc = coll_wide_stack_check(ctx, c, q, who, "fm_collection_votes");
    if (rc != FM_OK) return rc;
    return coll_votes_host(ctx, c, q, tau, mode, votes, who);
}

// ---------------------------------------------------------------------------------------
// Fast-Match's accepted-match test per image: fm_collection_match_accepted_each
// ---------------------------------------------------------------------------------------
// Slot i = fm_match_accepted(q, bank(T_i)): the cross-checked nearest neighbour of q inside image i, kept when
// (double)dist / selfdist[q] < tau (fastmatch.pyx:122-124, 161-165).
//
// Integer route.  Which query row a train row elects does not depend on the image the train row belongs to, so the reverse
// top-1 sweep runs ONCE over the stack (output rows = the stack's physical rows, reduced over the query rows) and only the
// second step is per image: a segmented scatter-min into qbest[image][query].
// The stack as the OUTPUT operand of a sweep (first use), what its padding rows do there:
//   * an output row is read through rows8 (zero bytes) and norm (2^26) only; the aux words / kPadCinit of a padding row
//     belong to the REDUCED side and are not read.  Its partial is a valid key with d2 = 2^26 + |q|^2 (no overflow: < 2^27)
//     that nothing reads as a candidate: the election drops the row by index (st_real, as coll_real does).
//   * shared bounds ("coop", bound[]): one word per OUTPUT row, read and raised only by the workgroups that sweep that same
//     row over other splits.  A padding row's word bounds the padding row's own candidates; no real row reads it.
//   * the ratio cut seeds an output row's threshold from its own norm: a padding row (2^26) starts above every query row's
//     reach and keeps the empty key, which the election skips anyway.
// Float32-root ties: a train row whose best d2 >= kSqrtTieMin shares its root with d2 + 1 goes to the tie list and is
// redone exactly (coll_sqrt_fix1_kernel).  The list exists when sqrt_tie_possible holds for ANY image of the chunk (usq per
// image, the query's largest norm); a row can reach the listed range only inside an image for which it holds
// (d2 <= |q|^2 + |t|^2), so the rows listed are those fm_xcheck1 lists image by image.
// Ratio cut: as ratio_sync (accepted-only: every reported row passes the test).  D* depends on the query bank and tau alone;
// a candidate at d2 >= D* can win qbest[image][q] only where no acceptable row elected q in that image, and then fails the
// ratio test: the accepted rows are those of the unseeded sweep.
// Chunks: qbest and the decode arrays cost 25 bytes per (image, query row).  Beyond the budget (option "coll_ws_bytes"; 0 = a
// quarter of the free device memory) the images go in chunks of consecutive images -- whose stack rows are one bank view -- ,
// enqueued back to back on the context's stream into the same arrays; counts and compacted rows of all images are copied
// out once, at the end.
// Float32 route: per-image reverse sweeps (K8 / K5) enqueued back to back on the images' bank views, each followed by
// fm_xcheck1's own election into slot i of the table; the tail is shared.  (One reverse K8 sweep over the stack is not
// built: every padding output row would put its candidates into the filter's lists.)
//
// fm_collection_xcheck1_each is the same table without the ratio test -- cv2.BFMatcher(norm, crossCheck=True).match(q, T_i)
// image by image, kept while dist < max_dist -- and takes it to binary collections:
// Binary route.  The election of a train row does not depend on its image here either: ONE reverse K11 sweep per chunk,
// cols = the chunk's stack view, red = the query bank (stage_real stays null: the reduced side is an ordinary bank whose
// tail the sweep masks by nred).  The stack as the OUTPUT operand of ham_sweep_kernel (first use), its padding rows:
//   * an output row is read through rows4 only.  A padding row is an all-zero FP4 row: every dot product is 0, so it sits
//     at h = W / 2 from every query row and leaves a VALID key (W / 2, the lowest query row) -- no value marks it.
//   * nothing may read that key as a candidate: the election drops the row by index (coll_lookup: st_real), exactly as
//     it drops the integer route's.  Output rows share no state in K11 (no bounds, no cut), so a padding row cannot
//     change a real row's key.
// The keys' high word already holds the float32 bits of h (an integer <= 512: exact, one root per value), so the election
// takes them as they are: no sqrt_bits, no tie list.  Ties follow from the key order alone: (h bits, query row) per train
// row -- the lowest query index --, then (h bits, row inside the image) per (image, query row) -- the lowest row.

// Segmented election: xcheck_scatter_kernel over the physical rows [p0, p0 + nrows) of the stack; the key's low word is the
// row inside its image, the table slot (image - img0, query).  f32: the keys' high word holds the distance's float32 bits
// (K11) and is taken as it is; else the exact d2 (integer route: float32 root, tie list).
__global__ void coll_elect_kernel(const unsigned long long* __restrict__ partial, int nsplit, int ncols_alloc, int64_t nrows,
                                  unsigned p0, CollTab tab, int img0, int64_t nq, unsigned long long* __restrict__ qbest,
                                  int f32, unsigned* __restrict__ fix)
{
    // four lanes per physical row, each takes every 4th split
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t t = gid >> 2;
    const int part = (int)(gid & 3);
    unsigned long long b = ~0ull;
    if (t < nrows) {
        for (int s = part; s < nsplit; s += 4) {
            const unsigned long long v = partial[(size_t)s * ncols_alloc + t];
            b = v < b ? v : b;
        }
    }
    unsigned long long o = __shfl_xor(b, 1);
    b = o < b ? o : b;
    o = __shfl_xor(b, 2);
    b = o < b ? o : b;
    if (t >= nrows || part != 0 || b == ~0ull) return;
    const unsigned p = p0 + (unsigned)t;
    int32_t img, local;
    if (!coll_lookup(tab, p, img, local)) return;          // a padding row of the stack
    const unsigned q = (unsigned)b;
    unsigned hi = (unsigned)(b >> 32);
    if (!f32) {
        if (fix && hi >= kSqrtTieMin && sqrt_ties_up(hi)) { fix[4 + atomicAdd(fix, 1u)] = p; return; }
        hi = sqrt_bits(hi);
    }
    atomicMin(&qbest[(int64_t)(img - img0) * nq + q], ((unsigned long long)hi << 32) | (unsigned)local);
}

// sqrt_fix_kernel<1> (api_match.hip) per image: the listed physical rows of the stack elect again, exactly, over all query
// rows in (float32 root, query row) order; the winner's slot takes (distance bits, row inside the image).
__global__ __launch_bounds__(256)
void coll_sqrt_fix1_kernel(const unsigned* __restrict__ fix, const int8_t* __restrict__ stack_rows, const int32_t* __restrict__ stack_norm,
                           const int8_t* __restrict__ q_rows, const int32_t* __restrict__ q_norm, int nq_rows, CollTab tab, int img0,
                           int64_t nq, unsigned long long* __restrict__ qbest)
{
    __shared__ unsigned long long best;
    const int tid = threadIdx.x;
    const unsigned n = fix[0];
    for (unsigned e = blockIdx.x; e < n; e += gridDim.x) {
        const unsigned c = fix[4 + e];
        if (tid == 0) best = ~0ull;
        __syncthreads();
        v4i cr[kDim / 16];
#pragma unroll
        for (int w = 0; w < kDim / 16; ++w) cr[w] = *(const v4i*)(stack_rows + (size_t)c * kDim + 16 * w);
        const int cn = stack_norm[c];
        unsigned long long k0 = ~0ull;
        for (int m = tid; m < nq_rows; m += 256) {
            int dot = 0;
#pragma unroll
            for (int w = 0; w < kDim / 16; ++w) {
                const v4i y = *(const v4i*)(q_rows + (size_t)m * kDim + 16 * w);
#pragma unroll
                for (int u = 0; u < 4; ++u) dot = __builtin_amdgcn_sdot4(cr[w][u], y[u], dot, false);
            }
            const unsigned d2 = (unsigned)(cn + q_norm[m] - 2 * dot);
            const unsigned long long key = ((unsigned long long)sqrt_bits(d2) << 32) | (unsigned)m;
            if (key < k0) k0 = key;
        }
        if (k0 != ~0ull) atomicMin(&best, k0);
        __syncthreads();
        if (tid == 0 && best != ~0ull) {
            const unsigned long long g0 = best;
            int32_t img, local;
            if (coll_lookup(tab, c, img, local))
                atomicMin(&qbest[(int64_t)(img - img0) * nq + (unsigned)g0], (g0 & 0xffffffff00000000ull) | (unsigned long long)(unsigned)local);
        }
        __syncthreads();
    }
}

// The test a decoded entry must pass.  selfdist set: Fast-Match's accepted-match test, (double)dist / selfdist[q] < tau.
// Null: the plain cross-check under a distance limit, dist < max_dist -- a strict float32 compare on the reported value
// (+inf keeps every match, a limit <= 0 or NaN none) -- and a dropped entry then reads -1 / +inf in the decode arrays, which
// are the host form's dense result.
struct CollKeep { const double* selfdist; double tau; float max_dist; };

// xcheck_finalize_kernel for a chunk's table, blockIdx.y = image of the chunk: decode, the test (the same float64 division),
// the flag, and the block counts of the compaction behind it.  ratio: null without self distances.
__global__ __launch_bounds__(256)
void coll_each_finalize_kernel(const unsigned long long* __restrict__ qbest, int64_t nq, CollKeep keep,
                               int32_t* __restrict__ tidx, float* __restrict__ dist, double* __restrict__ ratio, uint8_t* __restrict__ pass,
                               int* __restrict__ block_counts)
{
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t e = (int64_t)blockIdx.y * nq + q;
    bool p = false;
    if (q < nq) {
        const unsigned long long key = qbest[e];
        int32_t ti = -1;
        float d = INFINITY;
        double r = NAN;
        if (key != ~0ull) {
            ti = (int32_t)(unsigned)key;
            d = __uint_as_float((unsigned)(key >> 32));
            if (keep.selfdist) {
                r = (double)d / keep.selfdist[q];
                p = r < keep.tau;
            } else {
                p = d < keep.max_dist;
                if (!p) { ti = -1; d = INFINITY; }
            }
        }
        tidx[e] = ti;
        dist[e] = d;
        if (ratio) ratio[e] = r;
        pass[e] = p ? 1 : 0;
    }
    emit_block_count(__ballot(p), block_counts + (size_t)blockIdx.y * gridDim.x);
}

// Ordered compaction of image blockIdx.y's kept rows (compact_slot) into its slot of the outputs, addressed from the
// chunk's first image: four arrays [.][cap] (o_rows null) or 12-byte rows [.][cap][3] with o_count = the rows that are there;
// full = the number kept.  cap = 0: counts only.
__global__ __launch_bounds__(256)
void coll_each_compact_kernel(const int32_t* __restrict__ tidx, const float* __restrict__ dist, const double* __restrict__ ratio,
                              const uint8_t* __restrict__ pass, const int* __restrict__ block_counts, int64_t nq, int64_t cap,
                              int32_t* __restrict__ o_q, int32_t* __restrict__ o_t, float* __restrict__ o_d, double* __restrict__ o_r,
                              int32_t* __restrict__ o_rows, long long* __restrict__ o_count, unsigned long long* __restrict__ full)
{
    const int64_t i = blockIdx.y;
    int64_t q, total;
    bool p;
    const int64_t dst = compact_slot(block_counts + (size_t)i * gridDim.x, pass + i * nq, nq, &q, &p, &total);
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
        full[i] = (unsigned long long)total;
        if (o_count) o_count[i] = total < cap ? (long long)total : (long long)cap;
    }
    if (p && dst < cap) {
        const int64_t e = i * nq + q, o = i * cap + dst;
        if (o_rows) {
            o_rows[3 * o] = (int32_t)q;
            o_rows[3 * o + 1] = tidx[e];
            o_rows[3 * o + 2] = (int32_t)__float_as_uint(dist[e]);
        } else {
            o_q[o] = (int32_t)q; o_t[o] = tidx[e]; o_d[o] = dist[e]; o_r[o] = ratio[e];
        }
    }
}

constexpr size_t kCollAcceptEntry = 25;            // qbest 8 | tidx 4 | dist 4 | ratio 8 | pass 1 bytes per (image, query row)
constexpr size_t kCollXcheckEntry = 17;            // fm_collection_xcheck1_each: the same without the ratio
constexpr int kCollAcceptMaxChunk = 65535;         // (blockIdx.y of the tail kernels)

// The images [i0, i1) as one bank view of the stack (consecutive images are consecutive physical rows)
static fm::Bank coll_chunk_view(const fm_collection* c, int64_t i0, int64_t i1)
{
    const int64_t ni = (int64_t)c->rows.size();
    const int64_t p0 = c->phys[(size_t)i0], p1 = i1 < ni ? c->phys[(size_t)i1] : c->used;
    fm::Bank v = bank_rows_view(c->stack, p0, p1 - p0);
    v.usq_max = 0;
    for (int64_t i = i0; i < i1; ++i) v.usq_max = std::max(v.usq_max, c->usq[(size_t)i]);
    return v;
}

// ---- wide collections: a chunk's reverse top-1 sweeps through the table kernels (wide_f32.hip, part 5, KTOP = 1) -----------
// fm_collection_wide_match_accepted_each.  The images of a chunk are swept in GROUPS of consecutive images: the non-empty
// images of a group are the slots of ONE table -- reverse slots alone: output rows = the image's rows (a view of the stack),
// reduced rows = the query bank, the operand outside the stack -- side by side in the group's output-row space, swept by one
// filter launch, one rescoring launch and one guarded exact launch (or the exact launch alone; wide_route's rule on the
// group's work), then ONE segmented election: every image row's key (float32 distance bits << 32 | query row) scatter-mins
// (distance bits << 32 | row inside the image) into qbest[image][query row] -- xcheck_scatter_kernel's election, image by
// image, so the table is fm_wide_match_accepted(q, bank(image))'s.  A group ends with the chunk, or before the image that
// would lift its real rows past kWideEachGroupRows: the group's record list holds 256 records per output row (at least 2^20),
// and that bounds it at 2^26 records (768 MiB of the context's workspace) whatever "coll_ws_bytes" lets a chunk hold.
constexpr int64_t kWideEachGroupRows = (int64_t)1 << 18;

struct WideEachGroup {
    int64_t i0 = 0, i1 = 0;                 // the images
    int nslots = 0, fwg = 0;                // non-empty images, the filter's grid
    int64_t rows = 0, real = 0;             // the output-row space (a multiple of 128), real rows
    bool filt = false; unsigned cap = 0;    // the route, the record list's size
    size_t o_slots = 0, o_wg0 = 0, o_rowp = 0, o_img = 0;       // WideSlot [n] | first workgroups [n + 1] | first rows [n + 1] | image - the chunk's first [n]
};
struct WideEachPlan {
    std::vector<WideEachGroup> groups;
    std::vector<char> tab;                  // the call's table image
    size_t w_cnt = 0, w_bound = 0, w_list = 0, w_score = 0;     // ws_partial: partial [rows] | count | bounds [rows] | records | their scores
};

__global__ __launch_bounds__(256)
void coll_wide_elect_kernel(const unsigned long long* __restrict__ partial, const WideSlot* __restrict__ slots, const int* __restrict__ rowp,
                            const int* __restrict__ img, int nslots, int rows, int64_t nq, unsigned long long* __restrict__ qbest)
{
    const int r = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (r >= rows) return;
    const unsigned long long key = partial[r];
    if (key == ~0ull) return;
    const int s = table_slot_of(rowp, nslots, r);
    const int local = r - rowp[s];
    if (local >= slots[s].ncols) return;                   // a padding row behind the image
    atomicMin(&qbest[(int64_t)img[s] * nq + (unsigned)key], (key & 0xffffffff00000000ull) | (unsigned long long)(unsigned)local);
}

// The groups of every chunk of nc images, their tables (uploaded once, into ws_in) and ws_partial for the largest group: all
// before anything is enqueued.
static int coll_wide_each_plan(fm_ctx* ctx, const fm_collection* c, const fm_bank* q, int64_t nc, const char* who, WideEachPlan* pl)
{
    const int64_t ni = (int64_t)c->rows.size(), nq = q->n;
    const fm::Bank& stack = c->stack;
    const bool filter_on = ctx->tune.f32_filter != 0 && ctx->d_counters && stack.filt_ok && stack.wrowsh && wide_filter_usable(*q, stack);
    const int dk = q->kscale - stack.kscale;                // kred - kcol: the reduced side is the query bank (launch_wide_filter's terms)
    int64_t max_rows = 0;
    size_t max_cap = 0;
    try {
        auto put = [&](const void* src, size_t bytes) {
            const size_t at = pl->tab.size();
            pl->tab.resize(at + align256(bytes));
            memcpy(pl->tab.data() + at, src, bytes);
            return at;
        };
        for (int64_t c0 = 0; c0 < ni; c0 += nc) {
            const int64_t c1 = std::min(ni, c0 + nc);
            for (int64_t i = c0; i < c1;) {
                WideEachGroup g;
                g.i0 = i;
                while (i < c1 && (g.real == 0 || g.real + c->rows[(size_t)i] <= kWideEachGroupRows)) {
                    const int64_t n = c->rows[(size_t)i++];
                    if (n > 0) { g.real += n; g.rows += pad128(n); ++g.nslots; }
                }
                g.i1 = i;
                if (g.rows > ((int64_t)1 << 30)) return fail(ctx, FM_EUNSUPPORTED, std::string(who) + ": one image of a wide collection has more than 2^30 rows");
                if (g.nslots > 0) {
                    // a group whose slots fill the chip without splits takes one split per slot (the match graph's rule)
                    const bool one_split = g.rows / kStageRows >= 512 && ctx->tune.f32_nsplit == 0;
                    std::vector<WideSlot> sl;
                    std::vector<int> wg0, rowp, img;
                    int wrow = 0, wg = 0;
                    for (int64_t j = g.i0; j < g.i1; ++j) {
                        const int64_t n = c->rows[(size_t)j];
                        if (n == 0) continue;
                        WideSlot w{};
                        w.col0 = (int)c->phys[(size_t)j]; w.ncols = (int)n;
                        w.red0 = 0; w.nred = (int)nq;
                        w.outside = kWideOutRed;
                        w.cscale = ldexpf(1.f, dk); w.nscale = ldexpf(1.f, 2 * dk); w.red_nm_max = q->nm_max;
                        const WideFilterPlan fp = plan_wide_filter(pad128(n), n, pad128(nq), ctx->tune);
                        w.ntiles = fp.ntiles;
                        w.nsplit = one_split ? 1 : fp.nsplit;
                        w.tiles_per_split = one_split ? fp.ntiles : fp.tiles_per_split;
                        w.row0 = wrow;
                        sl.push_back(w); wg0.push_back(wg); rowp.push_back(wrow); img.push_back((int)(j - c0));
                        wg += fp.nchunks * w.nsplit;
                        wrow += (int)pad128(n);
                    }
                    wg0.push_back(wg); rowp.push_back(wrow);
                    g.fwg = wg;
                    g.filt = filter_on && (ctx->tune.f32_filter >= 2 || (double)nq * (double)g.real >= 4.0e6);
                    if (g.filt) g.cap = (unsigned)std::min<int64_t>(std::max<int64_t>(256 * g.real, 1 << 20), (int64_t)1 << 26);
                    g.o_slots = put(sl.data(), sl.size() * sizeof(WideSlot));
                    g.o_wg0 = put(wg0.data(), wg0.size() * 4);
                    g.o_rowp = put(rowp.data(), rowp.size() * 4);
                    g.o_img = put(img.data(), img.size() * 4);
                    max_rows = std::max(max_rows, g.rows);
                    max_cap = std::max<size_t>(max_cap, g.cap);
                }
                pl->groups.push_back(g);
            }
        }
    } catch (const std::bad_alloc&) { return fail(ctx, FM_ENOMEM, std::string(who) + ": out of host memory"); }
    if (max_rows == 0) return FM_OK;
    int rc;
    pl->w_cnt = align256((size_t)max_rows * 8); pl->w_bound = pl->w_cnt + 256; pl->w_list = pl->w_bound + align256((size_t)max_rows * 4);
    pl->w_score = pl->w_list + align256(max_cap * 8);
    if ((rc = ws_ensure(ctx, &ctx->ws_partial, &ctx->ws_partial_bytes, pl->w_score + align256(max_cap * 4) + 64)) != FM_OK) return rc;
    const size_t tab_bytes = pl->tab.size();
    if ((rc = ws_ensure(ctx, &ctx->ws_in, &ctx->ws_in_bytes, tab_bytes + 64)) != FM_OK) return rc;
    if ((rc = table_host(ctx, tab_bytes)) != FM_OK) return rc;
    memcpy(ctx->h_tab, pl->tab.data(), tab_bytes);
    return table_upload(ctx, ctx->ws_in, tab_bytes);
}

// The groups of the chunk [i0, i1) into d_qbest [image - i0][query row] (preset to ~0).
static int coll_wide_qbest_groups(fm_ctx* ctx, const fm_collection* c, const fm_bank* q, const WideEachPlan& pl, int64_t i0, int64_t i1,
                                  unsigned long long* d_qbest, bool* timed)
{
    const int64_t nq = q->n;
    char* wp = (char*)ctx->ws_partial;
    const char* d = (const char*)ctx->ws_in;
    for (const WideEachGroup& g : pl.groups) {
        if (g.i0 < i0 || g.i1 > i1 || g.nslots == 0) continue;
        ctx->pending_pairs += nq * g.real;
        ctx->pending_bytes += (nq + g.real) * 1024;
        if (!*timed) HIP_TRY(ctx, hipEventRecord(ctx->ev_k0, ctx->stream));
        *timed = true;
        const WideTableLaunch tl{(const WideSlot*)(d + g.o_slots), (const int*)(d + g.o_wg0), (const int*)(d + g.o_rowp), g.nslots, g.fwg, g.rows, q};
        unsigned long long* part = (unsigned long long*)wp;
        if (g.filt) {
            HIP_TRY(ctx, hipMemsetAsync(part, 0xff, (size_t)g.rows * 8, ctx->stream));
            HIP_TRY(ctx, hipMemsetAsync(wp + pl.w_cnt, 0, 256 + (size_t)g.rows * 4, ctx->stream));      // (the count and the bounds are neighbours)
            HIP_TRY(ctx, hipMemsetAsync(ctx->d_counters, 0, 8, ctx->stream));
            HIP_TRY(ctx, launch_wide_filter_table(c->stack, tl, g.cap, (uint2*)(wp + pl.w_list), (float*)(wp + pl.w_score), (unsigned*)(wp + pl.w_bound),
                                                  (unsigned long long*)(wp + pl.w_cnt), ctx->d_counters, part, ctx->stream, 1));
            HIP_TRY(ctx, launch_wide_exact_table(c->stack, tl, part, ctx->d_counters, ctx->stream, 1));
            ctx->filter_launches += 1;
        } else {
            HIP_TRY(ctx, launch_wide_exact_table(c->stack, tl, part, nullptr, ctx->stream, 1));
        }
        hipLaunchKernelGGL(coll_wide_elect_kernel, dim3((unsigned)((g.rows + 255) / 256)), dim3(256), 0, ctx->stream, (const unsigned long long*)part,
                           tl.d_slots, tl.d_rowp, (const int*)(d + g.o_img), g.nslots, (int)g.rows, nq, d_qbest);
        HIP_TRY(ctx, hipGetLastError());
    }
    return FM_OK;
}

// The front half for the images [i0, i1): d_qbest[image - i0][query row] = (float32 distance bits << 32 | row inside the
// image) of the closest row of the image that elects the query row, ~0 where none does -- slot by slot the table of
// fm_xcheck1(q, bank(image)).  Integer and binary routes: one reverse top-1 sweep over the chunk's stack view and the
// segmented election (the integer route's tie list redone exactly); float32 route: the per-image sweeps, each with
// fm_xcheck1's own election.  cut: launch_rowreduce's (integer route) or null.  *timed: a sweep was enqueued; on the
// integer and binary routes ev_k0 is recorded in front of the first one and ev_k1 is the caller's.
static int coll_qbest_chunk(fm_ctx* ctx, fm_collection* c, const fm_bank* q, int64_t i0, int64_t i1, const unsigned* cut,
                            unsigned long long* d_qbest, bool* timed, const WideEachPlan* wide = nullptr)
{
    const int64_t nq = q->n;
    int rc;
    HIP_TRY(ctx, hipMemsetAsync(d_qbest, 0xff, (size_t)(i1 - i0) * nq * 8, ctx->stream));
    if (c->stack.kind == FM_BANK_F32W) return coll_wide_qbest_groups(ctx, c, q, *wide, i0, i1, d_qbest, timed);
    if (c->stack.kind == FM_BANK_F32) {
        for (int64_t i = i0; i < i1; ++i) {
            const fm::Bank v = coll_view(c, (int)i);
            if (v.n == 0) continue;
            PairSweep ps;
            if ((rc = sweep_pair(ctx, v, *q, 1, 0, nullptr, nullptr, kSweepNoEvents, &ps)) != FM_OK) return rc;
            *timed = true;                   // (the route brackets every sweep itself: the last one's events stand)
            hipLaunchKernelGGL(xcheck_scatter_kernel, dim3((unsigned)((v.n * 4 + 255) / 256)), dim3(256), 0, ctx->stream, ps.partial,
                               ps.nsplit, ps.ncols_alloc, v.n, d_qbest + (i - i0) * nq, 0u, ps.f32_keys, (int*)nullptr, (unsigned*)nullptr);
            HIP_TRY(ctx, hipGetLastError());
        }
        return FM_OK;
    }
    const fm::Bank v = coll_chunk_view(c, i0, i1);
    if (v.n == 0) return FM_OK;
    const CollTab tab{c->st_img(), c->st_real(), c->img_phys()};
    int64_t real = 0;
    for (int64_t i = i0; i < i1; ++i) real += c->rows[(size_t)i];
    ctx->pending_pairs += nq * real;
    ctx->pending_bytes += bank_bytes(q) + real * (v.kind == FM_BANK_BIN ? v.dim : 128);
    if (!*timed) HIP_TRY(ctx, hipEventRecord(ctx->ev_k0, ctx->stream));
    *timed = true;
    PairSweep ps;
    if ((rc = sweep_pair(ctx, v, *q, 1, v.n, cut, nullptr, kSweepNoEvents | kSweepNoCount, &ps)) != FM_OK) return rc;
    hipLaunchKernelGGL(coll_elect_kernel, dim3((unsigned)((v.n * 4 + 255) / 256)), dim3(256), 0, ctx->stream, ps.partial, ps.nsplit,
                       ps.ncols_alloc, v.n, (unsigned)c->phys[(size_t)i0], tab, (int)i0, nq, d_qbest, ps.f32_keys, ps.fix);
    HIP_TRY(ctx, hipGetLastError());
    if (ps.fix) {
        hipLaunchKernelGGL(coll_sqrt_fix1_kernel, dim3(kFixGrid), dim3(256), 0, ctx->stream, (const unsigned*)ps.fix,
                           (const int8_t*)c->stack.rows8, (const int32_t*)c->stack.norm, (const int8_t*)q->rows8,
                           (const int32_t*)q->norm, (int)nq, tab, (int)i0, nq, d_qbest);
        HIP_TRY(ctx, hipGetLastError());
    }
    return FM_OK;
}

// What a per-image election call tests and where its rows go.
// The device form's output pointers of the _each calls (any device's memory: a peer buffer is a valid destination).
static int coll_each_dev_check(fm_ctx* ctx, const char* who, const int64_t* d_counts, const int32_t* d_rows, int64_t cap)
{
    int rc;
    if (!d_counts || (cap > 0 && !d_rows)) return fail(ctx, FM_EINVAL, std::string(who) + ": device output pointer is NULL");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((rc = check_device_ptr(ctx, d_counts, who, "d_counts", false)) != FM_OK) return rc;
    if (cap > 0 && (rc = check_device_ptr(ctx, d_rows, who, "d_rows", false)) != FM_OK) return rc;
    return FM_OK;
}

// An _each call whose query bank has no rows: zero counts for every image.  d_counts (device form, else null) is zeroed on
// the context's stream behind the consumer's work; h_counts: the host counts, or null.
static int coll_each_no_rows(fm_ctx* ctx, int64_t ni, int64_t* d_counts, int64_t* h_counts, void* consumer)
{
    int rc;
    if (d_counts) {
        if ((rc = wait_for_stream(ctx, consumer)) != FM_OK) return rc;
        HIP_TRY(ctx, hipMemsetAsync(d_counts, 0, (size_t)ni * 8, ctx->stream));
        if ((rc = results_written(ctx, consumer)) != FM_OK) return rc;
        ctx->rows_stream = ctx->stream;
    }
    if (h_counts) for (int64_t i = 0; i < ni; ++i) h_counts[i] = 0;
    return FM_OK;
}

struct CollEachArgs {
    const char* who;
    bool accept;                     // the accepted-match test (tau, q's self distances); else the cross-check under max_dist
    double tau; float max_dist;
    int64_t cap;                     // rows per image of the compacted outputs (the cross-check's host form has none: 0)
    // host form.  accept: qidx / tidx / dist / ratio [n_images][cap], compacted; else tidx / dist [n_images][nq], dense (both
    // null: counts only).  counts [n_images]: the full counts.
    int32_t* qidx; int32_t* tidx; float* dist; double* ratio; int64_t* counts;
    // device form: d_rows [n_images][cap][3], d_counts [n_images], h_counts host [n_images] or null
    bool to_dev; int32_t* d_rows; int64_t* d_counts; int64_t* h_counts; void* consumer;
    // the Hamming form of the accepted-match test (fm_collection_hamming_match_accepted_each(_dev)): a binary collection and a
    // binary query bank with Hamming self distances; l2 = the L2 call its refusals name.  Else binary data is refused.
    bool hamming = false; const char* l2 = nullptr;
    // the wide form (fm_collection_wide_match_accepted_each(_dev)): a wide collection and a wide query bank with wide self
    // distances; l2 / ham = the calls its refusals name
    bool wide = false; const char* ham = nullptr;
};

static int coll_elect_each(fm_ctx* ctx, fm_collection* c, const fm_bank* q, const CollEachArgs& a)
{
    const std::string who(a.who);
    // (the cross-check: a query bank without rows is not held to the collection's kind, as in the radius calls -- every
    // creator makes an empty bank an integer-route one)
    int rc;
    if (a.hamming) {
        // (the kinds before coll_query_check's own refusals: a collection or a query bank that is not binary is FM_EINVAL here)
        if ((rc = coll_check(ctx, c, a.who)) != FM_OK) return rc;
        if (!q) return fail(ctx, FM_EINVAL, who + ": query bank is NULL");
        if ((rc = refuse_bin2(ctx, q, a.who)) != FM_OK) return rc;
        if (q->kind != FM_BANK_BIN || (c->dim != 0 && c->stack.kind != FM_BANK_BIN))
            return fail(ctx, FM_EINVAL, who + ": the collection and the query bank must be binary (fm_collection_add_bin, fm_bank_create_bin); " +
                                            a.l2 + " is the L2 call");
    }
    if (a.wide) {
        // (the header's order: handles, the kinds, the widths; coll_query_check refuses wide data and is not asked)
        if ((rc = coll_check(ctx, c, a.who)) != FM_OK) return rc;
        if (!q) return fail(ctx, FM_EINVAL, who + ": query bank is NULL");
        if ((rc = refuse_bin2(ctx, q, a.who)) != FM_OK) return rc;
        const bool cbin = c->dim != 0 && c->stack.kind == FM_BANK_BIN && !coll_is_wide(c);
        if (q->kind != FM_BANK_F32W || (!c->rows.empty() && !coll_is_wide(c)))
            return fail(ctx, FM_EINVAL, who + ": the collection and the query bank must be wide float (fm_collection_add_wide; FM_BANK_F32W: "
                                              "fm_bank_create_f32 with 129 .. 256 values per row); " +
                                              ((q->kind == FM_BANK_BIN || cbin) ? std::string(a.ham) + " is the Hamming call" : std::string(a.l2) + " is the L2 call"));
        if (c->dim != 0 && q->dim != c->dim) return fail(ctx, FM_EINVAL, who + ": the query's width differs from the collection's");
    } else if ((rc = coll_query_check(ctx, c, q, a.who, !a.accept)) != FM_OK) return rc;
    if (a.accept && !a.hamming && q->kind == FM_BANK_BIN)
        return fail(ctx, FM_EUNSUPPORTED, who + ": binary banks carry no self distances here: fm_collection_hamming_match_accepted_each(_dev) "
                                                "is the self-distance test of a binary collection");
    const int64_t nq = q->n, ni = (int64_t)c->rows.size(), cap = a.cap;
    if (a.accept && nq > 0 && !q->selfdist)
        return fail(ctx, FM_EINVAL, who + ": query bank has no self distances (" +
                                        (a.hamming ? "fm_hamming_set_selfdist, fm_hamming_self_dist_batch" :
                                         a.wide ? "fm_wide_set_selfdist, fm_wide_self_dist_batch" : "fm_bank_set_selfdist") + ")");
    if (cap < 0) return fail(ctx, FM_EINVAL, who + ": cap < 0");
    if (ni == 0) return FM_OK;
    if (a.to_dev) {
        if ((rc = coll_each_dev_check(ctx, a.who, a.d_counts, a.d_rows, cap)) != FM_OK) return rc;
    } else if (a.accept) {
        if (!a.counts) return fail(ctx, FM_EINVAL, who + ": n_accepted is NULL");
        if (nq > 0 && cap > 0 && (!a.qidx || !a.tidx || !a.dist || !a.ratio)) return fail(ctx, FM_EINVAL, who + ": output pointer is NULL");
        HIP_TRY(ctx, hipSetDevice(ctx->device));
    } else {
        if (!a.tidx != !a.dist) return fail(ctx, FM_EINVAL, who + ": tidx and dist are given together or not at all");
        if (!a.tidx && !a.counts) return fail(ctx, FM_EINVAL, who + ": every output pointer is NULL");
        HIP_TRY(ctx, hipSetDevice(ctx->device));
    }
    if (nq == 0) return coll_each_no_rows(ctx, ni, a.to_dev ? a.d_counts : nullptr, a.to_dev ? a.h_counts : a.counts, a.consumer);
    // images per chunk from the budget
    const int nblk = (int)((nq + 255) / 256);
    const size_t per = (size_t)nq * (a.accept ? kCollAcceptEntry : kCollXcheckEntry) + (size_t)nblk * 4;
    size_t budget = (size_t)ctx->tune.coll_ws_bytes;
    if (budget == 0) {
        budget = (size_t)64 << 20;
        if ((size_t)ni * per > budget) {              // (asked only where one chunk may not do)
            size_t f = 0, t = 0;
            HIP_TRY(ctx, hipMemGetInfo(&f, &t));
            budget = std::max(budget, f / 4);
        }
    }
    int64_t nc = (int64_t)(budget / per);
    nc = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(nc, ni), kCollAcceptMaxChunk));
    const bool columns = a.accept && !a.to_dev;                       // compacted columns kept in ws_out for the copy out
    const int64_t ccap = columns ? (cap < nq ? cap : nq) : 0;         // ... and their rows per image
    size_t off = 0;
    const size_t o_full = carve(off, (size_t)ni * 8);
    const size_t o_qbest = carve(off, (size_t)nc * nq * 8), o_ratio = carve(off, a.accept ? (size_t)nc * nq * 8 : 0);
    const size_t o_tidx = carve(off, (size_t)nc * nq * 4), o_dist = carve(off, (size_t)nc * nq * 4);
    const size_t o_pass = carve(off, (size_t)nc * nq), o_bc = carve(off, (size_t)nc * nblk * 4);
    const size_t o_cq = carve(off, (size_t)ni * ccap * 4), o_ct = carve(off, (size_t)ni * ccap * 4), o_cd = carve(off, (size_t)ni * ccap * 4);
    const size_t o_cr = carve(off, (size_t)ni * ccap * 8);
    if ((rc = ws_ensure(ctx, &ctx->ws_out, &ctx->ws_out_bytes, off + 64)) != FM_OK) return rc;
    char* b = (char*)ctx->ws_out;
    unsigned long long* d_full = (unsigned long long*)(b + o_full);
    unsigned long long* d_qbest = (unsigned long long*)(b + o_qbest);
    const bool wide = c->stack.kind == FM_BANK_F32W;
    const bool stacked = c->stack.kind != FM_BANK_F32;      // one sweep per chunk (a wide collection: per group of images, through the table kernels)
    // the sweep workspace is sized for the largest chunk before anything is enqueued (no reallocation between chunks)
    WideEachPlan wplan;
    if (wide && (rc = coll_wide_each_plan(ctx, c, q, nc, a.who, &wplan)) != FM_OK) return rc;
    if (stacked && !wide && c->total > 0) {
        for (int64_t i0 = 0; i0 < ni; i0 += nc) {
            const fm::Bank v = coll_chunk_view(c, i0, std::min(ni, i0 + nc));
            PairSweep ps;
            if (v.n > 0 && (rc = sweep_pair_plan(ctx, v, *q, 1, v.n, &ps)) != FM_OK) return rc;
        }
    }
    CallScope cs(ctx);
    const unsigned* cut = nullptr;
    if (a.accept && c->stack.kind == FM_BANK_I8 && c->total > 0 && (rc = enqueue_ratio_cut(ctx, 1, &q, a.tau, &cut)) != FM_OK) return rc;
    const CollKeep keep{a.accept ? (const double*)q->selfdist : (const double*)nullptr, a.tau, a.max_dist};
    bool timed = false;
    for (int64_t i0 = 0; i0 < ni; i0 += nc) {
        const int64_t i1 = std::min(ni, i0 + nc), g = i1 - i0;
        if ((rc = coll_qbest_chunk(ctx, c, q, i0, i1, cut, d_qbest, &timed, &wplan)) != FM_OK) return rc;
        hipLaunchKernelGGL(coll_each_finalize_kernel, dim3((unsigned)nblk, (unsigned)g), dim3(256), 0, ctx->stream,
                           (const unsigned long long*)d_qbest, nq, keep, (int32_t*)(b + o_tidx), (float*)(b + o_dist),
                           a.accept ? (double*)(b + o_ratio) : (double*)nullptr, (uint8_t*)(b + o_pass), (int*)(b + o_bc));
        HIP_TRY(ctx, hipGetLastError());
        if (!a.to_dev && !a.accept && a.tidx) {
            // the dense result of the chunk, before the next chunk decodes into the same arrays
            HIP_TRY(ctx, d2h_pieces(ctx, (size_t)g * nq, (size_t)32 << 20, {{a.tidx + i0 * nq, b + o_tidx, 4}, {a.dist + i0 * nq, b + o_dist, 4}}));
        }
        // (device form: the first compaction is the first kernel that writes the caller's buffers)
        if (a.to_dev && i0 == 0 && (rc = wait_for_stream(ctx, a.consumer)) != FM_OK) return rc;
        hipLaunchKernelGGL(coll_each_compact_kernel, dim3((unsigned)nblk, (unsigned)g), dim3(256), 0, ctx->stream,
                           (const int32_t*)(b + o_tidx), (const float*)(b + o_dist), (const double*)(b + o_ratio), (const uint8_t*)(b + o_pass),
                           (const int*)(b + o_bc), nq, a.to_dev ? cap : ccap,
                           (int32_t*)(b + o_cq) + i0 * ccap, (int32_t*)(b + o_ct) + i0 * ccap, (float*)(b + o_cd) + i0 * ccap,
                           (double*)(b + o_cr) + i0 * ccap, a.to_dev && cap > 0 ? a.d_rows + (size_t)i0 * cap * 3 : (int32_t*)nullptr,
                           a.to_dev ? (long long*)a.d_counts + i0 : (long long*)nullptr, d_full + i0);
        HIP_TRY(ctx, hipGetLastError());
    }
    if (timed) {
        if (stacked) HIP_TRY(ctx, hipEventRecord(ctx->ev_k1, ctx->stream));       // (the sweeps, the elections and the tails between them)
        ctx->kernel_timed = true;
    }
    if (a.to_dev) {
        if ((rc = results_written(ctx, a.consumer)) != FM_OK) return rc;
        ctx->rows_stream = ctx->stream;
        if (!a.h_counts) return FM_OK;            // (enqueued: nothing waits for the device)
        // the caller asked for host numbers: the call's one synchronisation
        HIP_TRY(ctx, hipMemcpyAsync(a.h_counts, d_full, (size_t)ni * 8, hipMemcpyDeviceToHost, ctx->stream));
        return cs.finish();
    }
    // the counts decide how much is copied: one small synchronous read, then min(count, cap) rows of every image
    std::vector<unsigned long long> cnt((size_t)ni);
    HIP_TRY(ctx, hipMemcpyAsync(cnt.data(), d_full, (size_t)ni * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (int64_t i = 0; columns && i < ni; ++i) {
        const size_t m = (size_t)std::min<int64_t>((int64_t)cnt[(size_t)i], ccap);
        if (m == 0) continue;
        HIP_TRY(ctx, d2h(ctx, a.qidx + i * cap, (int32_t*)(b + o_cq) + i * ccap, m * 4));
        HIP_TRY(ctx, d2h(ctx, a.tidx + i * cap, (int32_t*)(b + o_ct) + i * ccap, m * 4));
        HIP_TRY(ctx, d2h(ctx, a.dist + i * cap, (float*)(b + o_cd) + i * ccap, m * 4));
        HIP_TRY(ctx, d2h(ctx, a.ratio + i * cap, (double*)(b + o_cr) + i * ccap, m * 8));
    }
    if ((rc = cs.finish()) != FM_OK) return rc;
    if (a.counts) for (int64_t i = 0; i < ni; ++i) a.counts[i] = (int64_t)cnt[(size_t)i];
    return FM_OK;
}

extern "C" int fm_collection_match_accepted_each(fm_ctx* ctx, fm_collection* c, const fm_bank* q, double tau, int64_t cap, int32_t* qidx,
                                                 int32_t* tidx, float* dist, double* ratio, int64_t* n_accepted)
{
    const CollEachArgs a{"fm_collection_match_accepted_each", true, tau, 0.f, cap, qidx, tidx, dist, ratio, n_accepted,
                         false, nullptr, nullptr, nullptr, FM_NO_STREAM};
    return coll_elect_each(ctx, c, q, a);
}

extern "C" int fm_collection_match_accepted_each_dev(fm_ctx* ctx, fm_collection* c, const fm_bank* q, double tau, int64_t cap, int32_t* d_rows,
                                                     int64_t* d_counts, int64_t* h_counts, void* consumer_stream)
{
    const CollEachArgs a{"fm_collection_match_accepted_each_dev", true, tau, 0.f, cap, nullptr, nullptr, nullptr, nullptr, nullptr,
                         true, d_rows, d_counts, h_counts, consumer_stream};
    return coll_elect_each(ctx, c, q, a);
}

// The same two calls on a binary collection and a binary query bank that carries Hamming self distances (the header's "Hamming
// Fast-Match"): coll_qbest_chunk's binary route -- one reverse FP4 sweep per chunk, the segmented election -- and the tail above.
extern "C" int fm_collection_hamming_match_accepted_each(fm_ctx* ctx, fm_collection* c, const fm_bank* q, double tau, int64_t cap,
                                                         int32_t* qidx, int32_t* tidx, float* dist, double* ratio, int64_t* n_accepted)
{
    const CollEachArgs a{"fm_collection_hamming_match_accepted_each", true, tau, 0.f, cap, qidx, tidx, dist, ratio, n_accepted,
                         false, nullptr, nullptr, nullptr, FM_NO_STREAM, true, "fm_collection_match_accepted_each"};
    return coll_elect_each(ctx, c, q, a);
}

extern "C" int fm_collection_hamming_match_accepted_each_dev(fm_ctx* ctx, fm_collection* c, const fm_bank* q, double tau, int64_t cap,
                                                             int32_t* d_rows, int64_t* d_counts, int64_t* h_counts, void* consumer_stream)
{
    const CollEachArgs a{"fm_collection_hamming_match_accepted_each_dev", true, tau, 0.f, cap, nullptr, nullptr, nullptr, nullptr, nullptr,
                         true, d_rows, d_counts, h_counts, consumer_stream, true, "fm_collection_match_accepted_each_dev"};
    return coll_elect_each(ctx, c, q, a);
}

// The same two calls on a wide collection and a wide query bank that carries wide self distances (the header's "Wide
// Fast-Match"): coll_qbest_chunk's wide route -- groups of images through the top-1 table kernels, the segmented election --
// and the tail above.
extern "C" int fm_collection_wide_match_accepted_each(fm_ctx* ctx, fm_collection* c, const fm_bank* q, double tau, int64_t cap,
                                                      int32_t* qidx, int32_t* tidx, float* dist, double* ratio, int64_t* n_accepted)
{
    CollEachArgs a{"fm_collection_wide_match_accepted_each", true, tau, 0.f, cap, qidx, tidx, dist, ratio, n_accepted,
                   false, nullptr, nullptr, nullptr, FM_NO_STREAM, false, "fm_collection_match_accepted_each"};
    a.wide = true; a.ham = "fm_collection_hamming_match_accepted_each";
    return coll_elect_each(ctx, c, q, a);
}

extern "C" int fm_collection_wide_match_accepted_each_dev(fm_ctx* ctx, fm_collection* c, const fm_bank* q, double tau, int64_t cap,
                                                          int32_t* d_rows, int64_t* d_counts, int64_t* h_counts, void* consumer_stream)
{
    CollEachArgs a{"fm_collection_wide_match_accepted_each_dev", true, tau, 0.f, cap, nullptr, nullptr, nullptr, nullptr, nullptr,
                   true, d_rows, d_counts, h_counts, consumer_stream, false, "fm_collection_match_accepted_each_dev"};
    a.wide = true; a.ham = "fm_collection_hamming_match_accepted_each_dev";
    return coll_elect_each(ctx, c, q, a);
}

// cv2.BFMatcher(norm, crossCheck=True).match(q, T_i) image by image: the same table, kept while dist < max_dist.
extern "C" int fm_collection_xcheck1_each(fm_ctx* ctx, fm_collection* c, const fm_bank* q, float max_dist, int32_t* tidx, float* dist,
                                          int64_t* n_matched)
{
    const CollEachArgs a{"fm_collection_xcheck1_each", false, 0.0, max_dist, 0, nullptr, tidx, dist, nullptr, n_matched,
                         false, nullptr, nullptr, nullptr, FM_NO_STREAM};
    return coll_elect_each(ctx, c, q, a);
}

extern "C" int fm_collection_xcheck1_each_dev(fm_ctx* ctx, fm_collection* c, const fm_bank* q, float max_dist, int64_t cap, int32_t* d_rows,
                                              int64_t* d_counts, int64_t* h_counts, void* consumer_stream)
{
    const CollEachArgs a{"fm_collection_xcheck1_each_dev", false, 0.0, max_dist, cap, nullptr, nullptr, nullptr, nullptr, nullptr,
                         true, d_rows, d_counts, h_counts, consumer_stream};
    return coll_elect_each(ctx, c, q, a);
}

// ---------------------------------------------------------------------------------------
// mutual nearest neighbours + ratio test per image: fm_collection_mutual_ratio_each
// ---------------------------------------------------------------------------------------
// Slot i = fm_mutual_ratio(q, bank(T_i)).  The forward lists are fm_collection_knn2_each's (coll_each_device) and Lowe's
// test runs per (image, query row).  Which query rows a train row is nearest to does not depend on the image it sits in,
// so the candidates of ALL images -- (image, query row) entries that passed, in entry order, each naming its first
// neighbour by its physical row of the stack -- go through ONE restricted reverse sweep (mutual_reverse_device: the rows
// gathered from the stack's planes, chunks of consecutive candidates under "coll_ws_bytes"), one join, and the per-image
// ordered compaction of the other _each calls (coll_each_compact_kernel).
// Host form: the accepted rows of ALL images packed back to back in entry order (image, query row) -- the flat rank of the
// final flags -- so that four copies bring every image's rows down, whatever the number of images.
__global__ __launch_bounds__(256)
void coll_mutual_pack_kernel(const int32_t* __restrict__ tidx, const float* __restrict__ dist, const double* __restrict__ ratio,
                             const uint8_t* __restrict__ pass, const int* __restrict__ block_counts, int64_t nq, int nblk,
                             int32_t* __restrict__ o_q, int32_t* __restrict__ o_t, float* __restrict__ o_d, double* __restrict__ o_r)
{
    const int64_t q = (int64_t)(blockIdx.x % (unsigned)nblk) * 256 + threadIdx.x;
    const int64_t e = (int64_t)(blockIdx.x / (unsigned)nblk) * nq + q;
    const bool p = q < nq && pass[e];
    int64_t total;
    const int64_t dst = compact_rank(block_counts, (int)blockIdx.x, p, &total);
    if (p) { o_q[dst] = (int32_t)q; o_t[dst] = tidx[e]; o_d[dst] = dist[e]; o_r[dst] = ratio[e]; }
}

struct CollMutualArgs {
    const char* who;
    double tau; int symmetric; int64_t cap;
    int32_t* qidx; int32_t* tidx; float* dist; double* ratio; int64_t* counts;          // host form: [n_images][cap], [n_images]
    bool to_dev; int32_t* d_rows; int64_t* d_counts; int64_t* h_counts; void* consumer;  // device form
};

static int coll_mutual_each(fm_ctx* ctx, fm_collection* c, const fm_bank* q, const CollMutualArgs& a)
{
    const std::string who(a.who);
    int rc = coll_query_check(ctx, c, q, a.who, true);
    if (rc != FM_OK) return rc;
    const int64_t nq = q->n, ni = (int64_t)c->rows.size(), cap = a.cap;
    if (cap < 0) return fail(ctx, FM_EINVAL, who + ": cap < 0");
    if (ni == 0) return FM_OK;
    if (a.to_dev) {
        if ((rc = coll_each_dev_check(ctx, a.who, a.d_counts, a.d_rows, cap)) != FM_OK) return rc;
    } else {
        if (!a.counts) return fail(ctx, FM_EINVAL, who + ": n_accepted is NULL");
        if (nq > 0 && cap > 0 && (!a.qidx || !a.tidx || !a.dist || !a.ratio)) return fail(ctx, FM_EINVAL, who + ": output pointer is NULL");
        HIP_TRY(ctx, hipSetDevice(ctx->device));
    }
    if (nq == 0) return coll_each_no_rows(ctx, ni, a.to_dev ? a.d_counts : nullptr, a.to_dev ? a.h_counts : a.counts, a.consumer);
    const int nblk = (int)((nq + 255) / 256);
    const int64_t ne = ni * nq, nb = ni * nblk;
    if (nb > 0x7fffffff) return fail(ctx, FM_EUNSUPPORTED, who + ": n_images * ceil(nq / 256) exceeds 2^31 - 1");
    const int64_t pk = (a.to_dev || cap == 0) ? 0 : ne;            // host form: room for the packed rows of all images
    size_t off = 0;
    const size_t o_i2 = carve(off, (size_t)ne * 8), o_d2 = carve(off, (size_t)ne * 8), o_tidx = carve(off, (size_t)ne * 4), o_dist = carve(off, (size_t)ne * 4);
    const size_t o_ratio = carve(off, (size_t)ne * 8), o_pass = carve(off, (size_t)ne), o_pass2 = carve(off, (size_t)ne);
    const size_t o_bc = carve(off, (size_t)nb * 4), o_bc2 = carve(off, (size_t)nb * 4), o_cnt = carve(off, 16), o_full = carve(off, (size_t)ni * 8);
    const size_t o_cand = carve(off, (size_t)ne * 4);
    const size_t o_cq = carve(off, (size_t)pk * 4), o_ct = carve(off, (size_t)pk * 4), o_cd = carve(off, (size_t)pk * 4);
    const size_t o_cr = carve(off, (size_t)pk * 8);
    if ((rc = ws_ensure(ctx, &ctx->ws_out, &ctx->ws_out_bytes, off + 64)) != FM_OK) return rc;
    char* b = (char*)ctx->ws_out;
    int32_t* d_tidx = (int32_t*)(b + o_tidx); float* d_dist = (float*)(b + o_dist); double* d_ratio = (double*)(b + o_ratio);
    const uint8_t* d_pass = (const uint8_t*)(b + o_pass);
    const int* d_bc = (const int*)(b + o_bc);
    unsigned long long* d_cnt = (unsigned long long*)(b + o_cnt);
    unsigned long long* d_full = (unsigned long long*)(b + o_full);
    CallScope cs(ctx);
    if ((rc = coll_each_device(ctx, c, q, (int32_t*)(b + o_i2), (float*)(b + o_d2))) != FM_OK) return rc;
    hipLaunchKernelGGL(lowe_each_kernel, dim3((unsigned)nb), dim3(256), 0, ctx->stream, (const int32_t*)(b + o_i2), (const float*)(b + o_d2), nq, nblk,
                       a.tau, d_tidx, d_dist, d_ratio, (uint8_t*)(b + o_pass), (int*)(b + o_bc));
    HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(mutual_cand_kernel, dim3((unsigned)nb), dim3(256), 0, ctx->stream, (const int32_t*)d_tidx, d_pass, d_bc, nq, nblk,
                       c->total > 0 ? c->img_phys() : (const int32_t*)nullptr, (int32_t*)(b + o_cand), d_cnt);
    HIP_TRY(ctx, hipGetLastError());
    unsigned long long n_cand = 0;      // the call's host wait between the two sweeps
    HIP_TRY(ctx, hipMemcpyAsync(&n_cand, d_cnt, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (n_cand > 0) {
        fm::Bank t = c->stack;
        t.usq_max = 0;
        for (int64_t i = 0; i < ni; ++i) t.usq_max = std::max(t.usq_max, c->usq[(size_t)i]);
        size_t budget = (size_t)ctx->tune.coll_ws_bytes;
        if (budget == 0) budget = kMutualGatherBytes;
        int32_t* r_idx; float* r_dist;
        if ((rc = mutual_reverse_device(ctx, t, (const int32_t*)(b + o_cand), (int64_t)n_cand, q, budget, &r_idx, &r_dist)) != FM_OK) return rc;
        hipLaunchKernelGGL(mutual_join_kernel, dim3((unsigned)nb), dim3(256), 0, ctx->stream, d_pass, d_bc, nq, nblk, (const int32_t*)r_idx,
                           (const float*)r_dist, a.tau, a.symmetric, d_ratio, (uint8_t*)(b + o_pass2), (int*)(b + o_bc2));
        HIP_TRY(ctx, hipGetLastError());
        d_pass = (const uint8_t*)(b + o_pass2);
        d_bc = (const int*)(b + o_bc2);
    }
    // (no candidates: the forward flags are all clear and the same compaction writes the zero counts)
    if (a.to_dev && (rc = wait_for_stream(ctx, a.consumer)) != FM_OK) return rc;
    // per-image counts (device form: and the caller's rows) by the per-image ordered compaction of the other _each calls
    for (int64_t i0 = 0; i0 < ni; i0 += kCollAcceptMaxChunk) {           // (blockIdx.y of the compaction)
        const int64_t g = std::min<int64_t>(ni - i0, kCollAcceptMaxChunk);
        hipLaunchKernelGGL(coll_each_compact_kernel, dim3((unsigned)nblk, (unsigned)g), dim3(256), 0, ctx->stream,
                           (const int32_t*)d_tidx + i0 * nq, (const float*)d_dist + i0 * nq, (const double*)d_ratio + i0 * nq, d_pass + i0 * nq,
                           d_bc + i0 * nblk, nq, a.to_dev ? cap : 0, (int32_t*)nullptr, (int32_t*)nullptr, (float*)nullptr, (double*)nullptr,
                           a.to_dev && cap > 0 ? a.d_rows + (size_t)i0 * cap * 3 : (int32_t*)nullptr,
                           a.to_dev ? (long long*)a.d_counts + i0 : (long long*)nullptr, d_full + i0);
        HIP_TRY(ctx, hipGetLastError());
    }
    if (a.to_dev) {
        if ((rc = results_written(ctx, a.consumer)) != FM_OK) return rc;
        ctx->rows_stream = ctx->stream;
        if (!a.h_counts) return FM_OK;
        HIP_TRY(ctx, hipMemcpyAsync(a.h_counts, d_full, (size_t)ni * 8, hipMemcpyDeviceToHost, ctx->stream));
        return cs.finish();
    }
    if (pk > 0) {
        hipLaunchKernelGGL(coll_mutual_pack_kernel, dim3((unsigned)nb), dim3(256), 0, ctx->stream, (const int32_t*)d_tidx, (const float*)d_dist,
                           (const double*)d_ratio, d_pass, d_bc, nq, nblk, (int32_t*)(b + o_cq), (int32_t*)(b + o_ct), (float*)(b + o_cd),
                           (double*)(b + o_cr));
        HIP_TRY(ctx, hipGetLastError());
    }
    // the counts decide how much is copied: one small synchronous read, then the packed rows of all images in four copies
    std::vector<unsigned long long> cnt((size_t)ni);
    HIP_TRY(ctx, hipMemcpyAsync(cnt.data(), d_full, (size_t)ni * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    size_t total = 0;
    for (int64_t i = 0; i < ni; ++i) total += (size_t)cnt[(size_t)i];
    std::vector<int32_t> hq, ht;
    std::vector<float> hd;
    std::vector<double> hr;
    if (pk > 0 && total > 0) {
        try { hq.resize(total); ht.resize(total); hd.resize(total); hr.resize(total); }
        catch (const std::bad_alloc&) { return fail(ctx, FM_ENOMEM, who + ": out of host memory"); }
        HIP_TRY(ctx, d2h(ctx, hq.data(), b + o_cq, total * 4));
        HIP_TRY(ctx, d2h(ctx, ht.data(), b + o_ct, total * 4));
        HIP_TRY(ctx, d2h(ctx, hd.data(), b + o_cd, total * 4));
        HIP_TRY(ctx, d2h(ctx, hr.data(), b + o_cr, total * 8));
    }
    if ((rc = cs.finish()) != FM_OK) return rc;
    size_t at = 0;
    for (int64_t i = 0; i < ni; ++i) {
        const size_t n = (size_t)cnt[(size_t)i], m = std::min<size_t>(n, (size_t)cap);
        if (pk > 0 && m > 0) {
            memcpy(a.qidx + i * cap, hq.data() + at, m * 4);
            memcpy(a.tidx + i * cap, ht.data() + at, m * 4);
            memcpy(a.dist + i * cap, hd.data() + at, m * 4);
            memcpy(a.ratio + i * cap, hr.data() + at, m * 8);
        }
        at += n;
        a.counts[i] = (int64_t)n;
    }
    return FM_OK;
}

extern "C" int fm_collection_mutual_ratio_each(fm_ctx* ctx, fm_collection* c, const fm_bank* q, double tau, int32_t symmetric, int64_t cap,
                                               int32_t* qidx, int32_t* tidx, float* dist, double* ratio, int64_t* n_accepted)
{
    const CollMutualArgs a{"fm_collection_mutual_ratio_each", tau, symmetric, cap, qidx, tidx, dist, ratio, n_accepted,
                           false, nullptr, nullptr, nullptr, FM_NO_STREAM};
    return coll_mutual_each(ctx, c, q, a);
}

extern "C" int fm_collection_mutual_ratio_each_dev(fm_ctx* ctx, fm_collection* c, const fm_bank* q, double tau, int32_t symmetric, int64_t cap,
                                                   int32_t* d_rows, int64_t* d_counts, int64_t* h_counts, void* consumer_stream)
{
    const CollMutualArgs a{"fm_collection_mutual_ratio_each_dev", tau, symmetric, cap, nullptr, nullptr, nullptr, nullptr, nullptr,
                           true, d_rows, d_counts, h_counts, consumer_stream};
    return coll_mutual_each(ctx, c, q, a);
}
