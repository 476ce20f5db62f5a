// C-ABI of libfastmatch_hip.so (include/fastmatch_hip.h), part 1: the context (streams, workspaces, options,
// statistics, fm_mark / fm_wait), page-locked host memory and device-to-host staging, and the descriptor banks
// with K6, the bank upload kernel (bytes XOR 0x80, row norms, accumulator-order aux words).  The other
// entry points: api_match.hip (2-NN, cross-check, batches, rounds), api_expand.hip (K7), comm.hip (gather).
#include "ctx_internal.h"

using namespace fm;

// ---------------------------------------------------------------------------------------
// error plumbing
// ---------------------------------------------------------------------------------------
static std::mutex g_err_mu;
static std::string g_err;   // last context-less error

int fm::fail(fm_ctx* ctx, int code, const std::string& msg)
{
    if (ctx) ctx->err = msg;
    else { std::lock_guard<std::mutex> lk(g_err_mu); g_err = msg; }
    return code;
}

int fm::wait_for_stream(fm_ctx* ctx, void* s)
{
    if (s == FM_NO_STREAM) return FM_OK;
    hipEvent_t& ev = ctx->ev_foreign[(hipStream_t)s];
    if (!ev) HIP_TRY(ctx, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    HIP_TRY(ctx, hipEventRecord(ev, (hipStream_t)s));
    HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ev, 0));
    return FM_OK;
}

int fm::check_device_ptr(fm_ctx* ctx, const void* p, const char* who, const char* what, bool same_device)
{
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess || at.type != hipMemoryTypeDevice) {
        (void)hipGetLastError();
        return fail(ctx, FM_EINVAL, std::string(who) + ": " + what + " must be device memory");
    }
    if (same_device && at.device != ctx->device)
        return fail(ctx, FM_EINVAL, std::string(who) + ": " + what + " lives on device " + std::to_string(at.device) +
                                    ", the context on device " + std::to_string(ctx->device));
    return FM_OK;
}

int fm::ws_ensure(fm_ctx* ctx, void** p, size_t* cap, size_t need)
{
    if (need <= *cap && *p) return FM_OK;
    if (*p) { HIP_TRY(ctx, hipFree(*p)); *p = nullptr; *cap = 0; }
    size_t sz = need + need / 4 + 4096;
    HIP_TRY(ctx, hipMalloc(p, sz));
    *cap = sz;
    return FM_OK;
}
// ---------------------------------------------------------------------------------------
// K6: bank preparation
// ---------------------------------------------------------------------------------------
// One 256-thread block per 32-row tile; thread (r = tid>>3, c = tid&7) owns the 16 bytes
// [16c, 16c+16) of tile row r.  SRC_F32: source rows are float32; values are converted to
// uint8 and nonint[0] is raised if any value is not an integer in [0,255]; nonint[1] = max over the
// rows of the squared norm of the uint8 row (Bank::usq_max).
#ifdef FM_ENC_AB
// Measurement builds only (scripts/gpu_k1_enc_ab.sh): the shift of the int8 encoding, 128 = the product's
// u ^ 0x80.  L2 is shift invariant as long as BOTH banks of a call use one shift and no byte leaves int8: shift 0 is exact
// for rows whose bytes are <= 127.  The question it answers: does the operand ENCODING move the clock the chip holds
// (MI355X_MICROARCH.md, DVFS give-back (1): zero-heavy operands clock 2.30 vs 1.9 GHz) -- SIFT's many near-zero bytes are
// -128 .. -100 under the product's encoding, 0 .. 27 under shift 0.
__device__ int g_enc_shift = 128;
extern "C" int fm_debug_enc_shift(int s) { return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_enc_shift), &s, sizeof(int)); }
#define FM_ENC_SHIFT g_enc_shift
#else
#define FM_ENC_SHIFT 128
#endif
template <bool SRC_F32>
__global__ __launch_bounds__(256)
void bank_prep_kernel(const void* __restrict__ src, int64_t n, int dim,
                      int8_t* __restrict__ rows8, int32_t* __restrict__ norm,
                      int32_t* __restrict__ aux, int* __restrict__ nonint, int64_t ntiles,
                      const int32_t* __restrict__ map = nullptr)
{
    // map (fm_bank_create_*_gather): bank row i is source row map[i] -- a Grid_Cache over pre-extracted features packs
    // a keypoint into up to four cells; its descriptor crosses PCIe once and is copied here
    const int tid = threadIdx.x;
    const int r = tid >> 3, c = tid & 7;
    // A workgroup walks tiles blockIdx.x, + gridDim.x, ...: a refill (fm_bank_refill_u8_async) runs beside the distance
    // kernels with a small grid of long-lived workgroups -- thousands of one-tile workgroups each took a CU slot a
    // distance-kernel workgroup was waiting for (r04: 0.27 ms per 100k-row bank beside K1, 0.18 ms per image pair lost).
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t row = tile * kTileRows + r;
    unsigned w[4] = {0, 0, 0, 0};
    int sumsq = 0, usq = 0;
    bool bad = false;
    if (row < n) {
        const int64_t srow = map ? (int64_t)map[row] : row;
        // the thread's 16 values; full-width rows (dim = 128: SIFT) come in as 16-byte loads -- byte / float loads
        // one at a time ran the upload kernel at ~80 GB/s
        int uv[16];
        bool have[16];
        if (dim == kDim) {
            if constexpr (SRC_F32) {
                const float4* sp = (const float4*)((const float*)src + srow * kDim + 16 * c);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 v = sp[q];
                    const float f[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        const float fr = rintf(f[b]);
                        const bool ok = (f[b] == fr) && f[b] >= 0.f && f[b] <= 255.f;
                        bad |= !ok;
                        uv[4 * q + b] = ok ? (int)fr : 128;
                        have[4 * q + b] = true;
                    }
                }
            } else {
                const uint4 v = *(const uint4*)((const uint8_t*)src + srow * kDim + 16 * c);
                const unsigned ww[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int q = 0; q < 4; ++q)
#pragma unroll
                    for (int b = 0; b < 4; ++b) { uv[4 * q + b] = (int)((ww[q] >> (8 * b)) & 0xffu); have[4 * q + b] = true; }
            }
        } else {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int k = 16 * c + e;
                uv[e] = FM_ENC_SHIFT;                // padding beyond dim: 0 after the shift
                have[e] = k < dim;
                if (k < dim) {
                    if constexpr (SRC_F32) {
                        const float f = ((const float*)src)[srow * dim + k];
                        const float fr = rintf(f);
                        if (!(f == fr) || f < 0.f || f > 255.f) bad = true;
                        else uv[e] = (int)fr;
                    } else {
                        uv[e] = ((const uint8_t*)src)[srow * dim + k];
                    }
                }
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            unsigned word = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int u = uv[4 * q + b];
                if (have[4 * q + b]) usq += u * u;
                const int s = u - FM_ENC_SHIFT;      // 128: == (int8)(u ^ 0x80)
                sumsq += s * s;
                word |= (unsigned)(s & 0xff) << (8 * b);
            }
            w[q] = word;
        }
    }
    *(uint4*)(rows8 + row * kDim + 16 * c) = make_uint4(w[0], w[1], w[2], w[3]);
    sumsq += __shfl_xor(sumsq, 1);
    sumsq += __shfl_xor(sumsq, 2);
    sumsq += __shfl_xor(sumsq, 4);
    usq += __shfl_xor(usq, 1);
    usq += __shfl_xor(usq, 2);
    usq += __shfl_xor(usq, 4);
    usq = max(usq, __shfl_xor(usq, 8));
    usq = max(usq, __shfl_xor(usq, 16));
    usq = max(usq, __shfl_xor(usq, 32));
    if ((tid & 63) == 0 && usq > 0) atomicMax(nonint + 1, usq);
    if (c == 0) {
        // aux words of the 32-row unit in the accumulator order of v_mfma_i32_16x16x64_i8
        // (two 16-row tiles; tile row rr sits in lane group rr >> 2, register rr & 3)
        const int sub = r >> 4, rr = r & 15;
        const int id = 4 * sub + (rr & 3);
        int32_t* a = aux + tile * kAuxPerTile + 32 * sub;
        if (row < n) {
            norm[row] = sumsq;
            a[rr]      = -(sumsq >> 1);
            a[16 + rr] = ((1 - (sumsq & 1)) << 4) | (15 - id);
        } else {
            norm[row] = 0;
            a[rr]      = kPadCinit;
            a[16 + rr] = 15 - id;
        }
    }
    if constexpr (SRC_F32) {
        // one atomic per wave at most, and none once the flag is up (a bank that is not integer
        // valued would otherwise send one atomic per element to the same address)
        if (__builtin_amdgcn_ballot_w64(bad) != 0ull && (tid & 63) == 0 && *(volatile int*)nonint == 0) atomicOr(nonint, 1);
    }
  }
}

// The second half of bank_prep_kernel for the device-source kernel below: what a thread does with its 16 values uv[]
// (have[]: the value is inside the row's dim; live: the row is a real one) -- the int8 bytes, the row's norm and aux
// words, the largest uint8 norm into nonint[1].  (bank_prep_kernel keeps its own copy: it runs beside the distance kernels
// in a refill, and sharing this function cost it 46 VGPRs.)
__device__ __forceinline__ void bank_prep_emit(const int (&uv)[16], const bool (&have)[16], bool live, int64_t row, int64_t tile,
                                               int tid, int8_t* __restrict__ rows8, int32_t* __restrict__ norm,
                                               int32_t* __restrict__ aux, int* __restrict__ nonint)
{
    const int r = tid >> 3, c = tid & 7;
    unsigned w[4] = {0, 0, 0, 0};
    int sumsq = 0, usq = 0;
    if (live) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            unsigned word = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int u = uv[4 * q + b];
                if (have[4 * q + b]) usq += u * u;
                const int s = u - FM_ENC_SHIFT;      // 128: == (int8)(u ^ 0x80)
                sumsq += s * s;
                word |= (unsigned)(s & 0xff) << (8 * b);
            }
            w[q] = word;
        }
    }
    *(uint4*)(rows8 + row * kDim + 16 * c) = make_uint4(w[0], w[1], w[2], w[3]);
    sumsq += __shfl_xor(sumsq, 1);
    sumsq += __shfl_xor(sumsq, 2);
    sumsq += __shfl_xor(sumsq, 4);
    usq += __shfl_xor(usq, 1);
    usq += __shfl_xor(usq, 2);
    usq += __shfl_xor(usq, 4);
    usq = max(usq, __shfl_xor(usq, 8));
    usq = max(usq, __shfl_xor(usq, 16));
    usq = max(usq, __shfl_xor(usq, 32));
    if ((tid & 63) == 0 && usq > 0) atomicMax(nonint + 1, usq);
    if (c == 0) {
        // aux words of the 32-row unit in the accumulator order of v_mfma_i32_16x16x64_i8
        // (two 16-row tiles; tile row rr sits in lane group rr >> 2, register rr & 3)
        const int sub = r >> 4, rr = r & 15;
        const int id = 4 * sub + (rr & 3);
        int32_t* a = aux + tile * kAuxPerTile + 32 * sub;
        if (live) {
            norm[row] = sumsq;
            a[rr]      = -(sumsq >> 1);
            a[16 + rr] = ((1 - (sumsq & 1)) << 4) | (15 - id);
        } else {
            norm[row] = 0;
            a[rr]      = kPadCinit;
            a[16 + rr] = 15 - id;
        }
    }
}

// A float32 value of a row that may take the integer route: its uint8 value, or 128 (0 after the shift) and `bad` raised.
__device__ __forceinline__ int bank_prep_u8_of(float f, bool& bad)
{
    const float fr = rintf(f);
    const bool ok = (f == fr) && f >= 0.f && f <= 255.f;
    bad |= !ok;
    return ok ? (int)fr : 128;
}

// ---- fm_bank_create_dev: the same preparation from rows that are ALREADY in device memory -------------------------------------
// The caller's tensor is read in place -- no copy into ws_in -- as rows of `pitch` bytes (a column slice of a wider tensor
// is a pitched matrix) of uint8, float32, IEEE half or bfloat16 elements; half and bfloat16 widen to float32 in registers,
// exactly, and then follow the float32 rules.  DT = FM_DT_U8 / _F32 / _F16 / _BF16.
template <int DT>
__device__ __forceinline__ float dev_src_elem(const uint8_t* __restrict__ rowp, int k)
{
    if constexpr (DT == FM_DT_F32) return ((const float*)rowp)[k];
    else if constexpr (DT == FM_DT_F16) return (float)((const _Float16*)rowp)[k];
    else if constexpr (DT == FM_DT_BF16) return __uint_as_float((unsigned)((const uint16_t*)rowp)[k] << 16);
    else return (float)rowp[k];
}

// the 16 elements [16 c, 16 c + 16) of a full-width row whose address and pitch are multiples of 16 bytes
template <int DT>
__device__ __forceinline__ void dev_src_load16(const uint8_t* __restrict__ rowp, int c, float (&f)[16])
{
    if constexpr (DT == FM_DT_F32) {
        const float4* sp = (const float4*)rowp + 4 * c;
#pragma unroll
        for (int q = 0; q < 4; ++q) { const float4 v = sp[q]; f[4 * q] = v.x; f[4 * q + 1] = v.y; f[4 * q + 2] = v.z; f[4 * q + 3] = v.w; }
    } else if constexpr (DT == FM_DT_U8) {
        const uint4 v = *((const uint4*)rowp + c);
        const unsigned ww[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int e = 0; e < 16; ++e) f[e] = (float)((ww[e >> 2] >> (8 * (e & 3))) & 0xffu);
    } else {
        const uint4 v0 = *((const uint4*)rowp + 2 * c), v1 = *((const uint4*)rowp + 2 * c + 1);
        const unsigned ww[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const unsigned h = (ww[e >> 1] >> (16 * (e & 1))) & 0xffffu;
            if constexpr (DT == FM_DT_F16) f[e] = (float)__builtin_bit_cast(_Float16, (unsigned short)h);
            else f[e] = __uint_as_float(h << 16);
        }
    }
}

// bank_prep_kernel for a device source: same tiles, same outputs, same flag words.  vec: dim == 128 and the rows sit on
// 16-byte boundaries (16-byte loads); otherwise element loads.
template <int DT>
__global__ __launch_bounds__(256)
void bank_prep_dev_kernel(const uint8_t* __restrict__ src, int64_t pitch, int vec, int64_t n, int dim,
                          int8_t* __restrict__ rows8, int32_t* __restrict__ norm,
                          int32_t* __restrict__ aux, int* __restrict__ nonint, int64_t ntiles)
{
    const int tid = threadIdx.x;
    const int r = tid >> 3, c = tid & 7;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t row = tile * kTileRows + r;
        bool bad = false;
        int uv[16];
        bool have[16];
        if (row < n) {
            const uint8_t* rowp = src + row * pitch;
            float f[16];
            if (vec) {
                dev_src_load16<DT>(rowp, c, f);
#pragma unroll
                for (int e = 0; e < 16; ++e) have[e] = true;
            } else {
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int k = 16 * c + e;
                    have[e] = k < dim;
                    f[e] = k < dim ? dev_src_elem<DT>(rowp, k) : 0.f;
                }
            }
#pragma unroll
            for (int e = 0; e < 16; ++e) uv[e] = have[e] ? bank_prep_u8_of(f[e], bad) : FM_ENC_SHIFT;
        }
        bank_prep_emit(uv, have, row < n, row, tile, tid, rows8, norm, aux, nonint);
        if constexpr (DT != FM_DT_U8) {
            if (__builtin_amdgcn_ballot_w64(bad) != 0ull && (tid & 63) == 0 && *(volatile int*)nonint == 0) atomicOr(nonint, 1);
        }
    }
}

// bank_copy_f32_kernel for a device source: the float32 route's zero-padded [n_pad][128] rows.
template <int DT>
__global__ void bank_copy_dev_kernel(const uint8_t* __restrict__ src, int64_t pitch, int64_t n, int dim,
                                     float* __restrict__ dst, int64_t n_pad)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pad * kDim) return;
    const int64_t row = i / kDim;
    const int k = (int)(i % kDim);
    dst[i] = (row < n && k < dim) ? dev_src_elem<DT>(src + row * pitch, k) : 0.f;
}

// The largest FINITE magnitude of a device source (fm_collection_add_dev: it decides the 2^57 refusal and the scale of a
// rebuild before anything changes), bank_absmax_kernel's rule on the typed, pitched rows: |v| <= 3.0e38f counts, larger and
// NaN do not.  One atomic per wave on the bits of the non-negative float (bit order = value order).
template <int DT>
__global__ __launch_bounds__(256)
void dev_src_absmax_kernel(const uint8_t* __restrict__ src, int64_t pitch, int64_t n, int dim, unsigned* __restrict__ out)
{
    float m = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n * dim; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i / dim;
        const float v = fabsf(dev_src_elem<DT>(src + row * pitch, (int)(i - row * dim)));
        m = v <= 3.0e38f ? fmaxf(m, v) : m;
    }
#pragma unroll
    for (int mask = 1; mask < 64; mask <<= 1) m = fmaxf(m, __shfl_xor(m, mask));
    if ((threadIdx.x & 63) == 0 && m > 0.f) atomicMax(out, __float_as_uint(m));
}

// float32 bank for the general (non-integer) route: zero-padded copy [n_pad][128].
__global__ void bank_copy_f32_kernel(const float* __restrict__ src, int64_t n, int dim,
                                     float* __restrict__ dst, int64_t n_pad, const int32_t* __restrict__ map)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pad * kDim) return;
    const int64_t row = i / kDim;
    const int k = (int)(i % kDim);
    dst[i] = (row < n && k < dim) ? src[(map ? (int64_t)map[row] : row) * dim + k] : 0.f;
}

// fp16 rows, norms and accumulator inits of a float32 bank for the fp16 filter (filter_f16.hip).
// Pass 1: stat[0] = max finite |value| (float bits), stat[1] |= 1 if a value is not finite.
__global__ __launch_bounds__(256)
void bank_absmax_kernel(const float* __restrict__ rowsf, int64_t total, int* __restrict__ stat)
{
    float m = 0.f;
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const float v = fabsf(rowsf[i]);
        const bool fin = v <= 3.0e38f;
        bad |= !fin;
        m = fin ? fmaxf(m, v) : m;                    // the largest FINITE magnitude, whatever else the bank holds
    }
#pragma unroll
    for (int mask = 1; mask < 64; mask <<= 1) m = fmaxf(m, __shfl_xor(m, mask));
    if (__builtin_amdgcn_ballot_w64(bad) != 0ull && (threadIdx.x & 63) == 0) atomicOr(stat + 1, 1);
    if ((threadIdx.x & 63) == 0) atomicMax(stat, (int)__float_as_uint(m));          // m >= 0: bit order = value order
}

// Pass 2: 16 lanes per row, 8 dims per lane; rows scaled by 2^k (exact) and rounded to fp16
// (nearest even); norms of the scaled rows in float64 -> float32.  stat[0] = max norm.
__global__ __launch_bounds__(256)
void bank_prep_f16_kernel(const float* __restrict__ rowsf, int64_t n, int64_t n_pad, int k,
                          uint16_t* __restrict__ rowsh, float* __restrict__ normf,
                          float* __restrict__ auxf, int* __restrict__ stat)
{
    const int64_t row = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    const int c = threadIdx.x & 15;
    if (row >= n_pad) return;
    const float4 v0 = *(const float4*)(rowsf + row * kDim + 8 * c);
    const float4 v1 = *(const float4*)(rowsf + row * kDim + 8 * c + 4);
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
    *(uint4*)(rowsh + row * kDim + 8 * c) =
        make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
    ss += __shfl_xor(ss, 1);
    ss += __shfl_xor(ss, 2);
    ss += __shfl_xor(ss, 4);
    ss += __shfl_xor(ss, 8);
    if (c == 0) {
        const float nm = (float)ss;
        if (row < n) {
            normf[row] = nm;
            auxf[row] = -0.5f * nm;
        } else {
            normf[row] = 0.f;
            auxf[row] = -3.4e38f;
        }
    }
    // max norm: one atomic per wave (4 rows), not per row
    float m = (c == 0 && row < n) ? (float)ss : 0.f;
#pragma unroll
    for (int mask = 16; mask < 64; mask <<= 1) m = fmaxf(m, __shfl_xor(m, mask));
    if ((threadIdx.x & 63) == 0 && m > 0.f) atomicMax(stat, (int)__float_as_uint(m));
}

// ---------------------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------------------
extern "C" const char* fm_last_error(const fm_ctx* ctx)
{
    if (ctx) return ctx->err.c_str();
    std::lock_guard<std::mutex> lk(g_err_mu);
    static thread_local std::string copy;
    copy = g_err;
    return copy.c_str();
}

// Options of a context by name (include/fastmatch_hip.h lists them).
struct OptionDef { const char* name; int Tuning::* field; int lo, hi; const char* env; };
static const OptionDef kOptions[] = {
    {"nb", &Tuning::nb, 0, 8, "FM_NB"}, {"nsplit", &Tuning::nsplit, 0, 1 << 20, "FM_NSPLIT"}, {"nw", &Tuning::nw, 0, 16, "FM_NW"},
    {"nbuf", &Tuning::nbuf, 0, 3, "FM_NBUF"}, {"prio", &Tuning::prio, 0, 1, "FM_PRIO"},
    {"glds", &Tuning::glds, 0, 1, "FM_GLDS"}, {"coop", &Tuning::coop, 0, 1, "FM_COOP"},
    {"f32_filter", &Tuning::f32_filter, 0, 2, "FM_F32_FILTER"}, {"f32_nw", &Tuning::f32_nw, 0, 8, "FM_F32_NW"},
    {"f32_bound_every", &Tuning::f32_bound_every, 1, 64, "FM_F32_BOUND_EVERY"},
    {"f32_nsplit", &Tuning::f32_nsplit, 0, 1 << 20, "FM_F32_NSPLIT"}, {"f32_fused", &Tuning::f32_fused, -1, 1, "FM_F32_FUSED"},
    {"f32_lpc", &Tuning::f32_lpc, 0, 64, "FM_F32_LPC"},
    {"batch_group", &Tuning::batch_group, 1, kRRBatchMax, "FM_BATCH_GROUP"}, {"batch_tail", &Tuning::batch_tail, 0, kRRBatchMax, "FM_BATCH_TAIL"},
    {"async_time_every", &Tuning::async_time_every, 0, 1 << 20, "FM_ASYNC_TIME_EVERY"},
    {"k1_order", &Tuning::k1_order, 0, 2, "FM_K1_ORDER"}, {"bound_every", &Tuning::bound_every, 1, 1024, "FM_BOUND_EVERY"}, {"refill_grid", &Tuning::refill_grid, 1, 1 << 20, "FM_REFILL_GRID"},
    {"self_tri", &Tuning::self_tri, 0, 2, "FM_SELF_TRI"}, {"tri_stages", &Tuning::tri_stages, 0, 4096, "FM_TRI_STAGES"},
    {"expand_big", &Tuning::expand_big, 0, 1, nullptr}, {"expand_huge", &Tuning::expand_huge, 0, 1, nullptr}, {"expand_delegate", &Tuning::expand_delegate, 0, 1 << 30, "FM_EXPAND_DELEGATE"}, {"expand_grow", &Tuning::expand_grow, 0, 4, nullptr}, {"expand_prof", &Tuning::expand_prof, 0, 1, "FM_EXPAND_PROF"},
    {"delegated_rounds", &Tuning::delegated_rounds, 0, 0, nullptr},       // a counter: set to 0, read
    {"radius_ws_bytes", &Tuning::radius_ws_bytes, 1 << 16, 0x7fffffff, nullptr},
    {"coll_ws_bytes", &Tuning::coll_ws_bytes, 0, 0x7fffffff, nullptr},
    {"masked_mfma", &Tuning::masked_mfma, 0, 1, nullptr}, {"mask_pack_words", &Tuning::mask_pack_words, 64, (1 << 26) - 4, nullptr},
    {"fp6_filter", &Tuning::fp6_filter, 0, 1, nullptr}, {"fp6_cap", &Tuning::fp6_cap, 1, 1 << 24, nullptr},
    {"fp6_nsplit", &Tuning::fp6_nsplit, 0, 1 << 20, nullptr},
};

extern "C" int fm_ctx_set_option(fm_ctx* ctx, const char* name, int64_t value)
{
    if (!ctx || !name) return fail(ctx, FM_EINVAL, "fm_ctx_set_option: NULL argument");
    for (const OptionDef& o : kOptions) {
        if (strcmp(o.name, name) != 0) continue;
        if (value < o.lo || value > o.hi) return fail(ctx, FM_EINVAL, std::string("fm_ctx_set_option: value out of range for ") + name);
        if (o.field == &Tuning::f32_filter && value != 0 && !ctx->d_counters)
            return fail(ctx, FM_EDEVICE, "fm_ctx_set_option: the fp16 filter's counters could not be allocated on this context");
        ctx->tune.*(o.field) = (int)value;
        return FM_OK;
    }
    return fail(ctx, FM_EINVAL, std::string("fm_ctx_set_option: unknown option ") + name);
}

extern "C" int fm_ctx_get_option(fm_ctx* ctx, const char* name, int64_t* value)
{
    if (!ctx || !name || !value) return fail(ctx, FM_EINVAL, "fm_ctx_get_option: NULL argument");
    // read-only: what the last FP6 filter launch left in its words, summed over its pairs (waits for the context's stream)
    if (strcmp(name, "fp6_records") == 0 || strcmp(name, "fp6_fallbacks") == 0) {
        unsigned w[2 * kRRBatchMax] = {0};
        *value = 0;
        if (ctx->f6.cnt && ctx->f6_last_n > 0) {
            HIP_TRY(ctx, hipSetDevice(ctx->device));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->tails[fm_ctx::kTails - 1]));      // (a batched launch's rescoring and guard)
            HIP_TRY(ctx, hipMemcpy(w, ctx->f6.cnt, (size_t)ctx->f6_last_n * 8, hipMemcpyDeviceToHost));
            for (int i = 0; i < ctx->f6_last_n; ++i) *value += name[4] == 'r' ? (int64_t)w[2 * i] : (int64_t)(w[2 * i + 1] != 0);
        }
        return FM_OK;
    }
    for (const OptionDef& o : kOptions)
        if (strcmp(o.name, name) == 0) { *value = ctx->tune.*(o.field); return FM_OK; }
    return fail(ctx, FM_EINVAL, std::string("fm_ctx_get_option: unknown option ") + name);
}

extern "C" int fm_ctx_destroy(fm_ctx* ctx);

extern "C" int fm_ctx_create(int device_id, fm_ctx** out)
{
    if (!out) return fail(nullptr, FM_EINVAL, "fm_ctx_create: out is NULL");
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        (void)hipGetLastError();
        return fail(nullptr, FM_EDEVICE,
                    std::string("fm_ctx_create: no HIP device available (") +
                    (e != hipSuccess ? hipGetErrorString(e) : "device count 0") +
                    "); libfastmatch_hip has no CPU fallback");
    }
    if (device_id < 0 || device_id >= ndev) return fail(nullptr, FM_EINVAL, "fm_ctx_create: bad device id");
    fm_ctx* ctx = new (std::nothrow) fm_ctx();
    if (!ctx) return fail(nullptr, FM_ENOMEM, "fm_ctx_create: out of host memory");
    ctx->device = device_id;
    hipDeviceProp_t prop;
    if ((e = hipSetDevice(device_id)) != hipSuccess || (e = hipGetDeviceProperties(&prop, device_id)) != hipSuccess) {
        delete ctx;
        return fail(nullptr, FM_EDEVICE, std::string("fm_ctx_create: ") + hipGetErrorString(e));
    }
    ctx->devname = std::string(prop.gcnArchName) + " " + prop.name;
    ctx->ncu = prop.multiProcessorCount;
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        std::string m = "fm_ctx_create: device is " + ctx->devname + "; this library is built for gfx950 only";
        delete ctx;
        return fail(nullptr, FM_EUNSUPPORTED, m);
    }
    if ((e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking)) != hipSuccess ||
        (e = hipEventCreate(&ctx->ev_call0)) != hipSuccess || (e = hipEventCreate(&ctx->ev_call1)) != hipSuccess ||
        (e = hipEventCreate(&ctx->ev_k0)) != hipSuccess || (e = hipEventCreate(&ctx->ev_k1)) != hipSuccess) {
        delete ctx;
        return fail(nullptr, FM_EDEVICE, std::string("fm_ctx_create: ") + hipGetErrorString(e));
    }
    {
        // the tail stream gets the highest priority: its workgroups are few and short and should not
        // queue behind the thousands of workgroups of the K1 they overlap
        int least = 0, greatest = 0;
        if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) { (void)hipGetLastError(); least = greatest = 0; }
        if ((e = hipStreamCreateWithPriority(&ctx->tails[0], hipStreamNonBlocking, greatest)) != hipSuccess ||
            (e = hipStreamCreateWithPriority(&ctx->tails[1], hipStreamNonBlocking, greatest)) != hipSuccess ||
            (e = hipStreamCreateWithPriority(&ctx->tails[2], hipStreamNonBlocking, greatest)) != hipSuccess ||
            ((ctx->stream_tail = ctx->tails[0]), false) ||
            (e = hipEventCreateWithFlags(&ctx->aslot[0].tail_done, hipEventDisableTiming)) != hipSuccess ||
            (e = hipEventCreateWithFlags(&ctx->aslot[1].tail_done, hipEventDisableTiming)) != hipSuccess ||
            (e = hipEventCreateWithFlags(&ctx->ev_consumer, hipEventDisableTiming)) != hipSuccess ||
            (e = hipEventCreateWithFlags(&ctx->ev_tail_end[0], hipEventDisableTiming)) != hipSuccess ||
            (e = hipEventCreateWithFlags(&ctx->ev_tail_end[1], hipEventDisableTiming)) != hipSuccess ||
            (e = hipEventCreateWithFlags(&ctx->ev_tail_end[2], hipEventDisableTiming)) != hipSuccess ||
            (e = hipEventCreateWithFlags(&ctx->ev_f6_sweep[0], hipEventDisableTiming)) != hipSuccess ||
            (e = hipEventCreateWithFlags(&ctx->ev_f6_sweep[1], hipEventDisableTiming)) != hipSuccess ||
            (e = hipEventCreateWithFlags(&ctx->ev_f6_done[0], hipEventDisableTiming)) != hipSuccess ||
            (e = hipEventCreateWithFlags(&ctx->ev_f6_done[1], hipEventDisableTiming)) != hipSuccess ||
            (e = hipEventCreateWithFlags(&ctx->aslot[0].k_done, hipEventDisableTiming)) != hipSuccess ||
            (e = hipEventCreateWithFlags(&ctx->aslot[1].k_done, hipEventDisableTiming)) != hipSuccess) {
            fm_ctx_destroy(ctx);
            return fail(nullptr, FM_EDEVICE, std::string("fm_ctx_create: ") + hipGetErrorString(e));
        }
    }
    if (hipHostMalloc((void**)&ctx->h_scratch, 64, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); ctx->h_scratch = nullptr; }
    // defaults from the environment (experiments; a value out of range is ignored), then per context
    // through fm_ctx_set_option
    for (const OptionDef& o : kOptions)
        if (o.env) if (const char* s = getenv(o.env)) { const long v = atol(s); if (v >= o.lo && v <= o.hi) ctx->tune.*(o.field) = (int)v; }
    if (getenv("FM_EXPAND_NO_BIG")) ctx->tune.expand_big = 0;
    ctx->dbg_f32 = getenv("FM_F32_DEBUG") != nullptr;
    ctx->dbg_expand = getenv("FM_EXPAND_DEBUG") != nullptr;
    ctx->dbg_park = ctx->dbg_expand && getenv("FM_PARK_PROF") != nullptr;
    if (hipMalloc((void**)&ctx->d_cut, 2 * kRRBatchMax * sizeof(unsigned)) != hipSuccess) { (void)hipGetLastError(); ctx->d_cut = nullptr; }
    if (hipMalloc((void**)&ctx->d_counters, filter_flag_bytes()) != hipSuccess || hipMemset(ctx->d_counters, 0, filter_flag_bytes()) != hipSuccess) {
        (void)hipGetLastError();
        ctx->d_counters = nullptr;
        ctx->tune.f32_filter = 0;
    }
    *out = ctx;
    return FM_OK;
}

extern "C" int fm_ctx_destroy(fm_ctx* ctx)
{
    if (!ctx) return FM_OK;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    for (hipStream_t ts : ctx->tails) if (ts) (void)hipStreamSynchronize(ts);
    auto free_slot = [](fm_ctx::AsyncSlot& sl) {
        if (sl.ws) (void)hipFree(sl.ws);
        if (sl.tail_done) (void)hipEventDestroy(sl.tail_done);
        if (sl.k_done) (void)hipEventDestroy(sl.k_done);
    };
    for (auto& m : ctx->marks) for (hipEvent_t ev : m.ev) if (ev) (void)hipEventDestroy(ev);
    for (auto& sl : ctx->aslot) free_slot(sl);
    for (auto& sl : ctx->bslot) free_slot(sl);
    if (ctx->upload) { (void)hipStreamSynchronize(ctx->upload); (void)hipStreamDestroy(ctx->upload); }
    if (ctx->ev_upload) (void)hipEventDestroy(ctx->ev_upload);
    if (ctx->ev_consumer) (void)hipEventDestroy(ctx->ev_consumer);
    for (auto& kv : ctx->ev_foreign) (void)hipEventDestroy(kv.second);
    if (ctx->ev_results) (void)hipEventDestroy(ctx->ev_results);
    for (hipEvent_t ev : ctx->ev_tail_end) if (ev) (void)hipEventDestroy(ev);
    if (ctx->comm) { comm_destroy(ctx->comm); ctx->comm = nullptr; }      // (before the streams it was used on)
    for (hipStream_t ts : ctx->tails) if (ts) (void)hipStreamDestroy(ts);
    for (auto* v : {&ctx->pending, &ctx->timer_pool})
        for (auto& t : *v) { (void)hipEventDestroy(t.c0); (void)hipEventDestroy(t.c1); (void)hipEventDestroy(t.k0); (void)hipEventDestroy(t.k1); }
    if (ctx->ws_partial) (void)hipFree(ctx->ws_partial);
    if (ctx->ws_out) (void)hipFree(ctx->ws_out);
    if (ctx->ws_in) (void)hipFree(ctx->ws_in);
    for (void* w : ctx->ws_f6) if (w) (void)hipFree(w);
    for (hipEvent_t ev : ctx->ev_f6_sweep) if (ev) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : ctx->ev_f6_done) if (ev) (void)hipEventDestroy(ev);
    for (void* w : {ctx->ws_rrows, ctx->ws_rkeys, ctx->ws_rtmp}) if (w) (void)hipFree(w);
    if (ctx->h_scratch) (void)hipHostFree(ctx->h_scratch);
    if (ctx->h_stage) (void)hipHostFree(ctx->h_stage);
    if (ctx->h_tab) (void)hipHostFree(ctx->h_tab);
    if (ctx->ev_tab) (void)hipEventDestroy(ctx->ev_tab);
    if (ctx->d_counters) (void)hipFree(ctx->d_counters);
    if (ctx->d_cut) (void)hipFree(ctx->d_cut);
    if (ctx->ev_call0) (void)hipEventDestroy(ctx->ev_call0);
    if (ctx->ev_call1) (void)hipEventDestroy(ctx->ev_call1);
    if (ctx->ev_k0) (void)hipEventDestroy(ctx->ev_k0);
    if (ctx->ev_k1) (void)hipEventDestroy(ctx->ev_k1);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
    return FM_OK;
}

// Account the calls that were enqueued without a synchronisation; the stream must be idle.
int fm::drain_pending(fm_ctx* ctx)
{
    for (auto& t : ctx->pending) {
        float ms = 0.f;
        if (t.call_timed) {      // enqueue-to-results latency of the call (overlapped calls: not additive)
            if (hipEventElapsedTime(&ms, t.k0, t.c1) == hipSuccess) { ctx->stats.total_ms += ms; ctx->stats.calls += 1; }
            else (void)hipGetLastError();
        }
        if (t.timed) {
            if (hipEventElapsedTime(&ms, t.k0, t.k1) == hipSuccess) {
                ctx->stats.kernel_ms += ms;
                ctx->stats.kernel_launches += 1;
                ctx->stats.pairs += t.pairs;
                ctx->stats_bytes += t.bytes;
            } else (void)hipGetLastError();
        }
        ctx->timer_pool.push_back(t);
    }
    ctx->pending.clear();
    return FM_OK;
}

extern "C" int fm_sync(fm_ctx* ctx)
{
    if (!ctx) return fail(nullptr, FM_EINVAL, "fm_sync: ctx is NULL");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (ctx->upload) HIP_TRY(ctx, hipStreamSynchronize(ctx->upload));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (hipStream_t ts : ctx->tails) HIP_TRY(ctx, hipStreamSynchronize(ts));
    return drain_pending(ctx);
}

// fm_mark: remember "everything enqueued on this context so far"; fm_wait: block until that point is
// reached.  Work enqueued after the mark keeps running: a consumer can read the results of batch i while
// batch i + 1 is already on the device (double-buffered outputs) -- fm_sync would drain both.
extern "C" int fm_mark(fm_ctx* ctx, int64_t* ticket)
{
    if (!ctx || !ticket) return fail(ctx, FM_EINVAL, "fm_mark: NULL argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    fm_ctx::Mark& m = ctx->marks[ctx->next_mark % fm_ctx::kMarks];
    for (int u = 0; u < 1 + fm_ctx::kTails; ++u) {
        if (!m.ev[u]) HIP_TRY(ctx, hipEventCreateWithFlags(&m.ev[u], hipEventDisableTiming));
        HIP_TRY(ctx, hipEventRecord(m.ev[u], u == 0 ? ctx->stream : ctx->tails[u - 1]));
    }
    m.id = ctx->next_mark;
    *ticket = ctx->next_mark++;
    return FM_OK;
}

extern "C" int fm_wait(fm_ctx* ctx, int64_t ticket)
{
    if (!ctx) return fail(nullptr, FM_EINVAL, "fm_wait: ctx is NULL");
    if (ticket < 0 || ticket >= ctx->next_mark) return fail(ctx, FM_EINVAL, "fm_wait: unknown ticket");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    fm_ctx::Mark& m = ctx->marks[ticket % fm_ctx::kMarks];
    if (m.id != ticket) {            // the slot has been re-used by a later mark: everything older is covered by it
        if (m.id < ticket) return fail(ctx, FM_EINVAL, "fm_wait: unknown ticket");
    }
    for (hipEvent_t ev : m.ev) if (ev) HIP_TRY(ctx, hipEventSynchronize(ev));
    return FM_OK;
}

extern "C" int fm_get_stats(fm_ctx* ctx, fm_stats* out)
{
    if (!ctx || !out) return fail(ctx, FM_EINVAL, "fm_get_stats: NULL argument");
    if (!ctx->pending.empty()) {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        for (hipStream_t ts : ctx->tails) HIP_TRY(ctx, hipStreamSynchronize(ts));
        drain_pending(ctx);
    }
    *out = ctx->stats;
    return FM_OK;
}

extern "C" int fm_get_stats_ex(fm_ctx* ctx, fm_stats_ex* out, int64_t out_bytes)
{
    if (!ctx || !out || out_bytes < 8) return fail(ctx, FM_EINVAL, "fm_get_stats_ex: bad argument");
    fm_stats st;
    int rc = fm_get_stats(ctx, &st);
    if (rc != FM_OK) return rc;
    fm_stats_ex ex{};
    ex.struct_bytes = (int64_t)sizeof(fm_stats_ex);
    ex.kernel_ms = st.kernel_ms; ex.total_ms = st.total_ms; ex.kernel_launches = st.kernel_launches;
    ex.pairs = st.pairs; ex.calls = st.calls;
    ex.bytes_moved = ctx->stats_bytes;
    memcpy(out, &ex, (size_t)(out_bytes < (int64_t)sizeof(ex) ? out_bytes : (int64_t)sizeof(ex)));
    return FM_OK;
}

extern "C" int fm_abi_version(void) { return FM_ABI_VERSION; }

extern "C" int fm_reset_stats(fm_ctx* ctx)
{
    if (!ctx) return fail(nullptr, FM_EINVAL, "fm_reset_stats: ctx is NULL");
    ctx->stats = fm_stats{};
    ctx->stats_bytes = 0;
    return FM_OK;
}

extern "C" int fm_f32_filter_stats(fm_ctx* ctx, int64_t* launches, int64_t* fallbacks)
{
    if (!ctx) return fail(nullptr, FM_EINVAL, "fm_f32_filter_stats: ctx is NULL");
    int c[4] = {0, 0, 0, 0};
    if (ctx->d_counters) {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        HIP_TRY(ctx, hipMemcpy(c, ctx->d_counters, 16, hipMemcpyDeviceToHost));
    }
    if (ctx->dbg_f32) fprintf(stderr, "[fm] filter: launches %lld, redone by K5 %d, output rows rescanned %d\n",
                                        (long long)ctx->filter_launches, c[2], c[3]);
    if (launches) *launches = ctx->filter_launches;
    if (fallbacks) *fallbacks = c[2];
    return FM_OK;
}

extern "C" int fm_device_name(fm_ctx* ctx, char* buf, int buflen)
{
    if (!ctx || !buf || buflen <= 0) return fail(ctx, FM_EINVAL, "fm_device_name: bad argument");
    snprintf(buf, (size_t)buflen, "%s", ctx->devname.c_str());
    return FM_OK;
}

// Page-locked allocations made through fm_host_alloc, with their device-side aliases: the async entry
// points look up to fifty output pointers per call, and a runtime query per pointer (microseconds each)
// would sit in front of the first launch of a batch.
struct PinnedRange { size_t bytes; char* dev; };
static std::mutex g_pinned_mu;
static std::map<uintptr_t, PinnedRange> g_pinned;

extern "C" int fm_host_alloc(fm_ctx* ctx, int64_t bytes, void** out)
{
    if (!ctx || !out || bytes < 0) return fail(ctx, FM_EINVAL, "fm_host_alloc: bad argument");
    *out = nullptr;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t sz = (size_t)(bytes > 0 ? bytes : 1);
    HIP_TRY(ctx, hipHostMalloc(out, sz, hipHostMallocDefault));
    void* dev = nullptr;
    if (hipHostGetDevicePointer(&dev, *out, 0) == hipSuccess && dev) {
        std::lock_guard<std::mutex> lk(g_pinned_mu);
        g_pinned[(uintptr_t)*out] = PinnedRange{sz, (char*)dev};
    } else (void)hipGetLastError();
    return FM_OK;
}

extern "C" int fm_host_free(fm_ctx* ctx, void* p)
{
    if (!p) return FM_OK;
    if (ctx) (void)hipSetDevice(ctx->device);
    { std::lock_guard<std::mutex> lk(g_pinned_mu); g_pinned.erase((uintptr_t)p); }
    hipError_t e = hipHostFree(p);
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(ctx, FM_EDEVICE, std::string("fm_host_free: ") + hipGetErrorString(e)); }
    return FM_OK;
}

// Device-side alias of a page-locked host buffer (fm_host_alloc / hipHostMalloc), or NULL for
// ordinary pageable memory: kernels can then write results straight into the caller's buffer.
void* fm::pinned_device_alias(const void* host)
{
    if (!host) return nullptr;
    {
        std::lock_guard<std::mutex> lk(g_pinned_mu);
        auto it = g_pinned.upper_bound((uintptr_t)host);
        if (it != g_pinned.begin()) {
            --it;
            const size_t off = (uintptr_t)host - it->first;
            if (off < it->second.bytes) return it->second.dev + off;
        }
    }
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, host) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    if (at.type != hipMemoryTypeHost) return nullptr;
    return at.devicePointer;
}

// Copy through the kernel's own stores (dst is the device alias of page-locked host memory).
__global__ void copy_out_kernel(unsigned char* __restrict__ dst, const unsigned char* __restrict__ src, size_t bytes)
{
    const size_t words = bytes / 4;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += stride)
        ((unsigned*)dst)[i] = ((const unsigned*)src)[i];
    if (blockIdx.x == 0 && threadIdx.x < (bytes & 3)) dst[words * 4 + threadIdx.x] = src[words * 4 + threadIdx.x];
}

// Device -> caller memory on the context's stream.  A copy into pageable memory makes the
// runtime pin the destination pages for the transfer (milliseconds for results of ~100 KB and
// up), so such results land in the context's own page-locked staging buffer and are moved to
// the caller by CallScope::finish() after the call's single synchronisation.
static hipError_t copy_out(fm_ctx* ctx, unsigned char* dst_alias, const void* src, size_t bytes)
{
    const unsigned grid = (unsigned)((bytes / 4 + 255) / 256 < 1024 ? (bytes / 4 + 255) / 256 + 1 : 1024);
    hipLaunchKernelGGL(copy_out_kernel, dim3(grid), dim3(256), 0, ctx->stream, dst_alias, (const unsigned char*)src, bytes);
    return hipGetLastError();
}

hipError_t fm::d2h(fm_ctx* ctx, void* dst, const void* src, size_t bytes)
{
    if (bytes == 0) return hipSuccess;
    // A copy kernel rather than hipMemcpyAsync for anything but tiny results: the runtime hands
    // device-to-host copies of 64 KiB and more to a DMA queue behind a host-side wait for the
    // stream, which was seen to add 1-7 ms of idle time after multi-millisecond kernels.
    const bool kernel_ok = bytes >= 4096 && bytes <= ((size_t)256 << 20) && ((uintptr_t)src & 3) == 0;
    if (kernel_ok) {
        if (unsigned char* direct = (unsigned char*)pinned_device_alias(dst))       // page-locked destination
            return copy_out(ctx, direct, src, bytes);
        size_t off = (ctx->h_stage_used + 63) & ~(size_t)63;
        if (off + bytes > ctx->h_stage_bytes && ctx->staged.empty()) {
            if (ctx->h_stage) (void)hipHostFree(ctx->h_stage);
            ctx->h_stage = nullptr;
            ctx->h_stage_bytes = 0;
            const size_t want = bytes * 3 + (1 << 20);
            if (hipHostMalloc((void**)&ctx->h_stage, want, hipHostMallocDefault) == hipSuccess) ctx->h_stage_bytes = want;
            else { (void)hipGetLastError(); ctx->h_stage = nullptr; }
            off = 0;
        }
        if (ctx->h_stage && off + bytes <= ctx->h_stage_bytes) {
            if (unsigned char* alias = (unsigned char*)pinned_device_alias(ctx->h_stage + off)) {
                hipError_t e = copy_out(ctx, alias, src, bytes);
                if (e != hipSuccess) return e;
                ctx->staged.push_back({dst, off, bytes});
                ctx->h_stage_used = off + bytes;
                return hipSuccess;
            }
        }
    }
    return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream);
}
// ---------------------------------------------------------------------------------------
// banks
// ---------------------------------------------------------------------------------------
// The FP6 plane of an integer-route bank (filter6.hip); without it the accepted-only sweeps of the bank stay on K1.
static void bank_free6(Bank* b)
{
    if (b->rows6) (void)hipFree(b->rows6);
    if (b->aux6) (void)hipFree(b->aux6);
    if (b->stat6) (void)hipFree(b->stat6);
    if (b->max6) (void)hipFree(b->max6);
    b->rows6 = nullptr; b->aux6 = nullptr; b->stat6 = nullptr; b->max6 = nullptr;
}
// Arrays for cap_pad rows and the plane of the current rows, enqueued on `stream`.  Best effort: an allocation that fails
// leaves the bank without the plane.
static void bank_plane6(Bank* b, hipStream_t stream)
{
    if (b->kind != FM_BANK_I8 || b->dim != kDim || !b->rows8) return;
    const size_t rows = (size_t)(b->cap_pad > b->n_pad ? b->cap_pad : b->n_pad);
    if (hipMalloc((void**)&b->rows6, rows * kDim) != hipSuccess || hipMalloc((void**)&b->aux6, rows * 2 * 4) != hipSuccess ||
        hipMalloc((void**)&b->stat6, rows * 16) != hipSuccess || hipMalloc((void**)&b->max6, 8) != hipSuccess ||
        launch_prep6(*b, 0, stream) != hipSuccess) {
        (void)hipGetLastError();
        bank_free6(b);
    }
}

static void bank_free(Bank* b)
{
    bank_free6(b);
    if (b->rows8) (void)hipFree(b->rows8);
    if (b->norm) (void)hipFree(b->norm);
    if (b->aux) (void)hipFree(b->aux);
    if (b->rowsf) (void)hipFree(b->rowsf);
    if (b->rowsh) (void)hipFree(b->rowsh);
    if (b->normf) (void)hipFree(b->normf);
    if (b->auxf) (void)hipFree(b->auxf);
    if (b->selfdist) (void)hipFree(b->selfdist);
    if (b->stage) (void)hipFree(b->stage);
    if (b->rowsb) (void)hipFree(b->rowsb);
    if (b->rows4) (void)hipFree(b->rows4);
    if (b->wrows) (void)hipFree(b->wrows);
    if (b->wrowsh) (void)hipFree(b->wrowsh);
    if (b->real_mem) (void)hipFree(b->real_mem);
    b->real = nullptr; b->real_mem = nullptr;
    b->wrows = nullptr; b->wrowsh = nullptr;
    b->stage = nullptr; b->rowsb = nullptr; b->rows4 = nullptr;
    b->rows8 = nullptr; b->norm = nullptr; b->aux = nullptr; b->rowsf = nullptr; b->selfdist = nullptr;
    b->sdmax = nullptr; b->sdmax_rows = -1;
    b->rowsh = nullptr; b->normf = nullptr; b->auxf = nullptr;
}

static hipError_t launch_bank_prep_dev(const DevSrc& d, int64_t n, int dim, Bank& b, int* d_flag, int ntiles, hipStream_t stream)
{
    const int vec = dim == kDim && (((uintptr_t)d.rows | (uintptr_t)d.pitch) & 15) == 0;
#define FM_PREP_DEV(DT_)                                                                                                   \
    case DT_: hipLaunchKernelGGL((bank_prep_dev_kernel<DT_>), dim3(ntiles), dim3(256), 0, stream, d.rows, d.pitch, vec, n, dim, \
                                 b.rows8, b.norm, b.aux, d_flag, (int64_t)ntiles); break;
    switch (d.dtype) {
        FM_PREP_DEV(FM_DT_U8) FM_PREP_DEV(FM_DT_F32) FM_PREP_DEV(FM_DT_F16) FM_PREP_DEV(FM_DT_BF16)
        default: return hipErrorInvalidValue;
    }
#undef FM_PREP_DEV
    return hipGetLastError();
}

static hipError_t launch_bank_copy_dev(const DevSrc& d, int64_t n, int dim, Bank& b, hipStream_t stream)
{
    const dim3 grid((unsigned)((b.n_pad * kDim + 255) / 256));
#define FM_COPY_DEV(DT_)                                                                                                   \
    case DT_: hipLaunchKernelGGL((bank_copy_dev_kernel<DT_>), grid, dim3(256), 0, stream, d.rows, d.pitch, n, dim, b.rowsf, b.n_pad); break;
    switch (d.dtype) {
        FM_COPY_DEV(FM_DT_F32) FM_COPY_DEV(FM_DT_F16) FM_COPY_DEV(FM_DT_BF16)
        default: return hipErrorInvalidValue;
    }
#undef FM_COPY_DEV
    return hipGetLastError();
}

int fm::dev_src_absmax(fm_ctx* ctx, const DevSrc& d, int64_t n, int dim, float* vmax)
{
    int rc = ws_ensure(ctx, &ctx->ws_in, &ctx->ws_in_bytes, 64);
    if (rc != FM_OK) return rc;
    unsigned* d_max = (unsigned*)ctx->ws_in;
    HIP_TRY(ctx, hipMemsetAsync(d_max, 0, 4, ctx->stream));
    const dim3 grid((unsigned)std::min<int64_t>(1024, (n * dim + 255) / 256));
#define FM_ABSMAX_DEV(DT_)                                                                                                 \
    case DT_: hipLaunchKernelGGL((dev_src_absmax_kernel<DT_>), grid, dim3(256), 0, ctx->stream, d.rows, d.pitch, n, dim, d_max); break;
    switch (d.dtype) {
        FM_ABSMAX_DEV(FM_DT_F32) FM_ABSMAX_DEV(FM_DT_F16) FM_ABSMAX_DEV(FM_DT_BF16)
        default: return fail(ctx, FM_EINVAL, "dev_src_absmax: not a floating-point source");
    }
#undef FM_ABSMAX_DEV
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(vmax, d_max, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return FM_OK;
}

// K14: a wide float32 bank -- [n][dim] rows, 129 <= dim <= 256 -- whatever the values (wide_f32.hip).  rows: a host float32
// matrix, staged dense; dev: the caller's device rows, read in place.  Both go through the same two kernels.
static int bank_create_wide(fm_ctx* ctx, const float* rows, int64_t n, int dim, fm_bank** out, const DevSrc* dev = nullptr)
{
    if (n > (int64_t)INT32_MAX - 2 * kStageRows) return fail(ctx, FM_EUNSUPPORTED, "fm_bank_create: n too large");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    fm_bank* b = new (std::nothrow) fm_bank();
    if (!b) return fail(ctx, FM_ENOMEM, "fm_bank_create: out of host memory");
    b->kind = FM_BANK_F32W;
    b->n = n;
    b->dim = dim;
    b->n_pad = b->cap_pad = n > 0 ? pad128(n) : kStageRows;
    auto bail = [&](hipError_t e, const char* what) {
        (void)hipGetLastError();
        bank_free(b); delete b;
        return fail(ctx, e == hipErrorOutOfMemory ? FM_ENOMEM : FM_EDEVICE, std::string("fm_bank_create (wide rows): ") + what + ": " + hipGetErrorString(e));
    };
    const size_t src_bytes = dev ? 0 : (size_t)n * dim * 4;
    const size_t flag_off = (src_bytes + 15) & ~(size_t)15;
    int rc = ws_ensure(ctx, &ctx->ws_in, &ctx->ws_in_bytes, flag_off + 32);
    if (rc != FM_OK) { bank_free(b); delete b; return rc; }
    int* d_stat = (int*)((char*)ctx->ws_in + flag_off);
    hipError_t e;
    if ((e = hipMalloc((void**)&b->wrows, (size_t)b->n_pad * kWideDim * 4)) != hipSuccess) return bail(e, "rows");
    if ((e = hipMalloc((void**)&b->wrowsh, (size_t)b->n_pad * kWideDim * 2)) != hipSuccess) return bail(e, "fp16 rows");
    if ((e = hipMalloc((void**)&b->normf, (size_t)b->n_pad * 4)) != hipSuccess) return bail(e, "norms");
    if ((e = hipMalloc((void**)&b->auxf, (size_t)b->n_pad * 4)) != hipSuccess) return bail(e, "accumulator inits");
    if (src_bytes && (e = hipMemcpyAsync(ctx->ws_in, rows, src_bytes, hipMemcpyHostToDevice, ctx->stream)) != hipSuccess) return bail(e, "upload");
    if ((e = hipMemsetAsync(d_stat, 0, 16, ctx->stream)) != hipSuccess) return bail(e, "fill");
    if (dev) e = launch_wide_copy(dev->rows, dev->dtype, dev->pitch, n, dim, *b, d_stat, ctx->stream);
    else     e = launch_wide_copy(ctx->ws_in, FM_DT_F32, (int64_t)dim * 4, n, dim, *b, d_stat, ctx->stream);
    if (e != hipSuccess) return bail(e, "copy");
    int stat[2] = {0, 0};
    if ((e = hipMemcpyAsync(stat, d_stat, 8, hipMemcpyDeviceToHost, ctx->stream)) != hipSuccess) return bail(e, "copy");
    if ((e = hipStreamSynchronize(ctx->stream)) != hipSuccess) return bail(e, "copy");
    float vmax = 0.f;
    memcpy(&vmax, &stat[0], 4);
    b->vfin_max = vmax;
    b->filt_ok = stat[1] == 0;
    int ex = 0;
    if (vmax > 0.f) (void)frexpf(vmax, &ex);         // vmax = m 2^ex, m in [0.5, 1)
    b->kscale = vmax > 0.f ? 14 - ex : 0;
    // (a bank with a value that is not finite keeps its planes, written from the scaled values as they come: the filter
    // never reads them, filt_ok is false)
    if ((e = launch_wide_planes(*b, d_stat + 2, ctx->stream)) != hipSuccess) return bail(e, "planes");
    if ((e = hipMemcpyAsync(stat, d_stat + 2, 4, hipMemcpyDeviceToHost, ctx->stream)) != hipSuccess) return bail(e, "planes");
    if ((e = hipStreamSynchronize(ctx->stream)) != hipSuccess) return bail(e, "planes");
    memcpy(&b->nm_max, &stat[0], 4);
    *out = b;
    return FM_OK;
}

// map != nullptr: the bank's row i is rows[map[i]] of the n_src source rows (0 <= map[i] < n_src, checked here).
// dev != nullptr: the rows are dev's (device memory, checked by the caller; `rows` is ignored, f32 = "not uint8").
static int bank_create(fm_ctx* ctx, const void* rows, int64_t n, int dim, bool f32, fm_bank** out, bool keep_f32 = false,
                       int64_t capacity = 0, const int32_t* map = nullptr, int64_t n_src = 0, const DevSrc* dev = nullptr)
{
    if (!ctx) return fail(nullptr, FM_EINVAL, "fm_bank_create: ctx is NULL");
    if (!out) return fail(ctx, FM_EINVAL, "fm_bank_create: bank out pointer is NULL");
    *out = nullptr;
    if (n < 0 || dim < 1 || (n > 0 && !rows && !dev)) return fail(ctx, FM_EINVAL, "fm_bank_create: bad rows/n/dim");
    if (map) {
        if (n_src < 0 || n_src > INT32_MAX) return fail(ctx, FM_EINVAL, "fm_bank_create_*_gather: bad n_src");
        for (int64_t i = 0; i < n; ++i)
            if (map[i] < 0 || map[i] >= n_src) return fail(ctx, FM_EINVAL, "fm_bank_create_*_gather: src_row entry outside [0, n_src)");
    }
    // float rows of 129 .. 256 values: a wide bank (K14), whatever the values; the gather creators, the capacity creators and
    // uint8 rows stay at 128
    if (f32 && dim > kDim && dim <= kWideDim && !map && capacity == 0)
        return bank_create_wide(ctx, (const float*)rows, n, dim, out, dev);
    if (dim > kDim) return fail(ctx, FM_EUNSUPPORTED, f32 && dim > kWideDim ? "fm_bank_create: dim > 256 is not supported"
                                                                             : "fm_bank_create: dim > 128 is not supported");
    if (n > (int64_t)INT32_MAX - 2 * kStageRows) return fail(ctx, FM_EUNSUPPORTED, "fm_bank_create: n too large");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    fm_bank* b = new (std::nothrow) fm_bank();
    if (!b) return fail(ctx, FM_ENOMEM, "fm_bank_create: out of host memory");
    b->n = n;
    b->dim = dim;
    b->n_pad = ((n + kStageRows - 1) / kStageRows) * kStageRows;
    if (b->n_pad == 0) b->n_pad = kStageRows;
    b->cap_pad = b->n_pad;
    if (capacity > n) {
        // room to grow (fm_bank_append_u8): the arrays are sized, and every tile prepared as padding, for `capacity` rows
        if (capacity > (int64_t)INT32_MAX - 2 * kStageRows) { delete b; return fail(ctx, FM_EUNSUPPORTED, "fm_bank_create: capacity too large"); }
        b->cap_pad = ((capacity + kStageRows - 1) / kStageRows) * kStageRows;
    }
    b->kind = FM_BANK_I8;
    const size_t elt = f32 ? 4 : 1;
    const size_t src_bytes = dev ? 0 : (size_t)(map ? n_src : n) * dim * elt;      // (a device source is not staged)
    int rc = FM_OK;
    auto bail = [&](int code) { bank_free(b); delete b; return code; };

    const size_t flag_off = (src_bytes + 15) & ~(size_t)15;
    if ((rc = ws_ensure(ctx, &ctx->ws_in, &ctx->ws_in_bytes, flag_off + 32 + (map ? (size_t)n * 4 : 0))) != FM_OK) return bail(rc);
    int* d_flag = (int*)((char*)ctx->ws_in + flag_off);
    const int32_t* d_map = map ? (const int32_t*)((char*)ctx->ws_in + flag_off + 32) : nullptr;
#define BTRY(expr)                                                                               \
    do {                                                                                         \
        hipError_t _e = (expr);                                                                  \
        if (_e != hipSuccess) {                                                                  \
            (void)hipGetLastError();                                                             \
            return bail(fail(ctx, _e == hipErrorOutOfMemory ? FM_ENOMEM : FM_EDEVICE,            \
                             std::string(#expr " failed: ") + hipGetErrorString(_e)));           \
        }                                                                                        \
    } while (0)
    BTRY(hipMalloc((void**)&b->rows8, (size_t)b->cap_pad * kDim));
    BTRY(hipMalloc((void**)&b->norm, (size_t)b->cap_pad * 4));
    BTRY(hipMalloc((void**)&b->aux, (size_t)(b->cap_pad / kTileRows) * kAuxPerTile * 4));
    if (src_bytes) BTRY(hipMemcpyAsync(ctx->ws_in, rows, src_bytes, hipMemcpyHostToDevice, ctx->stream));
    if (map && n > 0) BTRY(hipMemcpyAsync((void*)d_map, map, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    BTRY(hipMemsetAsync(d_flag, 0, 8, ctx->stream));
    const int ntiles = (int)(b->cap_pad / kTileRows);
    if (dev)
        BTRY(launch_bank_prep_dev(*dev, n, dim, *b, d_flag, ntiles, ctx->stream));
    else if (f32)
        hipLaunchKernelGGL(bank_prep_kernel<true>, dim3(ntiles), dim3(256), 0, ctx->stream,
                           (const void*)ctx->ws_in, n, dim, b->rows8, b->norm, b->aux, d_flag, (int64_t)ntiles, d_map);
    else
        hipLaunchKernelGGL(bank_prep_kernel<false>, dim3(ntiles), dim3(256), 0, ctx->stream,
                           (const void*)ctx->ws_in, n, dim, b->rows8, b->norm, b->aux, d_flag, (int64_t)ntiles, d_map);
    BTRY(hipGetLastError());
    int flags[2] = {0, 0};
    BTRY(hipMemcpyAsync(flags, d_flag, 8, hipMemcpyDeviceToHost, ctx->stream));
    BTRY(hipStreamSynchronize(ctx->stream));
    const int flag = flags[0];
    b->usq_max = flags[1];
    if (f32 && (flag || (keep_f32 && n > 0))) {
        // not integer-valued (or the caller wants the float32 route): keep a float32 bank for the fma-chain route
        b->kind = FM_BANK_F32;
        (void)hipFree(b->rows8); b->rows8 = nullptr;
        (void)hipFree(b->aux); b->aux = nullptr;
        BTRY(hipMalloc((void**)&b->rowsf, (size_t)b->n_pad * kDim * 4));
        const int64_t tot = b->n_pad * kDim;
        if (dev)
            BTRY(launch_bank_copy_dev(*dev, n, dim, *b, ctx->stream));
        else
            hipLaunchKernelGGL(bank_copy_f32_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, ctx->stream,
                               (const float*)ctx->ws_in, n, dim, b->rowsf, b->n_pad, d_map);
        BTRY(hipGetLastError());
        // rows for the fp16 filter, scaled by the power of two that puts the largest magnitude
        // of the bank in [2^13, 2^14)
        BTRY(hipMalloc((void**)&b->rowsh, (size_t)b->n_pad * kDim * 2));
        BTRY(hipMalloc((void**)&b->normf, (size_t)b->n_pad * 4));
        BTRY(hipMalloc((void**)&b->auxf, (size_t)b->n_pad * 4));
        BTRY(hipMemsetAsync(d_flag, 0, 8, ctx->stream));
        hipLaunchKernelGGL(bank_absmax_kernel, dim3(1024), dim3(256), 0, ctx->stream, (const float*)b->rowsf, tot, d_flag);
        BTRY(hipGetLastError());
        int stat[2] = {0, 0};
        BTRY(hipMemcpyAsync(stat, d_flag, 8, hipMemcpyDeviceToHost, ctx->stream));
        BTRY(hipStreamSynchronize(ctx->stream));
        float vmax = 0.f;
        memcpy(&vmax, &stat[0], 4);
        b->vfin_max = vmax;
        b->filt_ok = stat[1] == 0;
        if (b->filt_ok) {
            int ex = 0;
            if (vmax > 0.f) (void)frexpf(vmax, &ex);         // vmax = m 2^ex, m in [0.5, 1)
            b->kscale = vmax > 0.f ? 14 - ex : 0;
            BTRY(hipMemsetAsync(d_flag, 0, 8, ctx->stream));
            hipLaunchKernelGGL(bank_prep_f16_kernel, dim3((unsigned)(b->n_pad / 16)), dim3(256), 0, ctx->stream,
                               (const float*)b->rowsf, n, b->n_pad, b->kscale, b->rowsh, b->normf, b->auxf, d_flag);
            BTRY(hipGetLastError());
            BTRY(hipMemcpyAsync(stat, d_flag, 8, hipMemcpyDeviceToHost, ctx->stream));
            BTRY(hipStreamSynchronize(ctx->stream));
            memcpy(&b->nm_max, &stat[0], 4);
        }
    }
#undef BTRY
    bank_plane6(b, ctx->stream);        // (integer-route banks of dim 128 only)
    *out = b;
    return FM_OK;
}

extern "C" int fm_bank_create_u8(fm_ctx* ctx, const uint8_t* rows, int64_t n, int dim, fm_bank** bank)
{
    return bank_create(ctx, rows, n, dim, false, bank);
}

// Banks whose rows are a gather of the caller's rows (a keypoint in several Grid_Cache cells: uploaded once).
extern "C" int fm_bank_create_u8_gather(fm_ctx* ctx, const uint8_t* rows, int64_t n_src, int dim, const int32_t* src_row, int64_t n,
                                        fm_bank** bank)
{
    if (n > 0 && !src_row) return fail(ctx, FM_EINVAL, "fm_bank_create_u8_gather: src_row is NULL");
    if (!src_row) return bank_create(ctx, rows, 0, dim, false, bank);
    return bank_create(ctx, rows, n, dim, false, bank, false, 0, src_row, n_src);
}

extern "C" int fm_bank_create_f32_gather(fm_ctx* ctx, const float* rows, int64_t n_src, int dim, int float_route, const int32_t* src_row,
                                         int64_t n, fm_bank** bank)
{
    if (n > 0 && !src_row) return fail(ctx, FM_EINVAL, "fm_bank_create_f32_gather: src_row is NULL");
    if (!src_row) return bank_create(ctx, rows, 0, dim, true, bank, float_route != 0);
    return bank_create(ctx, rows, n, dim, true, bank, float_route != 0, 0, src_row, n_src);
}

extern "C" int fm_bank_create_u8_cap(fm_ctx* ctx, const uint8_t* rows, int64_t n, int dim, int64_t capacity, fm_bank** bank)
{
    if (capacity < n) return fail(ctx, FM_EINVAL, "fm_bank_create_u8_cap: capacity < n");
    return bank_create(ctx, rows, n, dim, false, bank, false, capacity);
}

// ---- the real-row bitmap of a bank that grew with gaps (Bank::real) ------------------------------------------------------
// Bits [r0, r1) on: one thread per word (r0 < r1; no two launches in flight touch one word -- the appends are synchronous).
__global__ void bank_real_set_kernel(unsigned long long* __restrict__ real, int64_t r0, int64_t r1)
{
    const int64_t w = (r0 >> 6) + (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (w > ((r1 - 1) >> 6)) return;
    const int64_t lo = r0 > 64 * w ? r0 - 64 * w : 0, hi = r1 < 64 * (w + 1) ? r1 - 64 * w : 64;
    const unsigned long long upto_hi = hi >= 64 ? ~0ull : ((1ull << hi) - 1ull), below_lo = (1ull << lo) - 1ull;
    real[w] |= upto_hi & ~below_lo;
}

static hipError_t bank_real_set(unsigned long long* real, int64_t r0, int64_t r1, hipStream_t stream)
{
    if (r1 <= r0) return hipSuccess;
    const int64_t words = ((r1 - 1) >> 6) - (r0 >> 6) + 1;
    hipLaunchKernelGGL(bank_real_set_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, stream, real, r0, r1);
    return hipGetLastError();
}

// In front of an append at row `off` (>= bank->n): the append leaves rows [bank->n, off) as padding INSIDE the bank.  The
// first such gap gives the bank its bitmap, with the rows so far -- all real until now -- marked; a bank that never has a
// gap never gets one.  Enqueued on the context's stream; bank_real_append marks the new rows once they are in.
static int bank_real_gap(fm_ctx* ctx, fm_bank* bank, int64_t off)
{
    if (bank->real || off == bank->n || bank->n == 0) return FM_OK;
    const size_t bytes = (size_t)(bank->cap_pad / 64) * 8;
    if (!bank->real_mem) HIP_TRY(ctx, hipMalloc((void**)&bank->real_mem, bytes));
    HIP_TRY(ctx, hipMemsetAsync(bank->real_mem, 0, bytes, ctx->stream));
    HIP_TRY(ctx, bank_real_set(bank->real_mem, 0, bank->n, ctx->stream));
    bank->real = bank->real_mem;
    return FM_OK;
}

// The rows [off, off + n) of an append marked real: enqueued only, in front of the append's own synchronisation (an append
// of a grown bank stays at the host waits it had).  Bits of rows at or beyond bank->n are never read, so marking before
// the append is known to have succeeded is harmless.
static int bank_real_append(fm_ctx* ctx, fm_bank* bank, int64_t off, int64_t n)
{
    if (!bank->real) return FM_OK;
    HIP_TRY(ctx, bank_real_set(bank->real, off, off + n, ctx->stream));
    return FM_OK;
}

// Rows appended to a bank created with room for them, at the next multiple of 32 rows (whole MFMA tiles: the rows
// of the tile an earlier append ended in stay what they are, padding).  Synchronous.
extern "C" int fm_bank_append_u8(fm_ctx* ctx, fm_bank* bank, const uint8_t* rows, int64_t n, int64_t* first_row)
{
    if (!ctx || !bank) return fail(ctx, FM_EINVAL, "fm_bank_append_u8: NULL argument");
    if (int rc = refuse_bin(ctx, bank, "fm_bank_append_u8")) return rc;
    if (bank->kind != FM_BANK_I8 || !bank->rows8) return fail(ctx, FM_EINVAL, "fm_bank_append_u8: not an integer-route bank");
    if (n < 0 || (n > 0 && !rows)) return fail(ctx, FM_EINVAL, "fm_bank_append_u8: bad rows / n");
    const int64_t off = ((bank->n + kTileRows - 1) / kTileRows) * kTileRows;
    if (first_row) *first_row = off;
    if (n == 0) return FM_OK;
    if (off + n > bank->cap_pad) return fail(ctx, FM_EINVAL, "fm_bank_append_u8: the bank's capacity is used up");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t src_bytes = (size_t)n * bank->dim, flag_off = (src_bytes + 15) & ~(size_t)15;
    int rc = ws_ensure(ctx, &ctx->ws_in, &ctx->ws_in_bytes, flag_off + 32);
    if (rc != FM_OK) return rc;
    if ((rc = bank_real_gap(ctx, bank, off)) != FM_OK) return rc;
    int* d_flag = (int*)((char*)ctx->ws_in + flag_off);
    HIP_TRY(ctx, hipMemcpyAsync(ctx->ws_in, rows, src_bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(d_flag, 0, 8, ctx->stream));
    const int64_t ntiles = (n + kTileRows - 1) / kTileRows;
    hipLaunchKernelGGL(bank_prep_kernel<false>, dim3((unsigned)ntiles), dim3(256), 0, ctx->stream, (const void*)ctx->ws_in, n, bank->dim,
                       bank->rows8 + (size_t)off * kDim, bank->norm + off, bank->aux + (off / kTileRows) * kAuxPerTile, d_flag, ntiles);
    HIP_TRY(ctx, hipGetLastError());
    if ((rc = bank_real_append(ctx, bank, off, n)) != FM_OK) return rc;
    int flags[2] = {0, 0};
    HIP_TRY(ctx, hipMemcpyAsync(flags, d_flag, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (flags[1] > bank->usq_max) bank->usq_max = flags[1];
    bank_free6(bank);       // (the rows between two appends are padding inside the bank: the FP6 plane has no mark for them)
    bank->n = off + n;
    bank->n_pad = ((bank->n + kStageRows - 1) / kStageRows) * kStageRows;
    return FM_OK;
}

// Rows [off, off + n_pad) of an integer-route bank's arrays (off and n_pad multiples of 128) from n host rows (uint8, or
// float32 when f32) -- the rows behind the n real ones come out as padding rows.  flags[0]: a float32 value was not an
// integer in 0 .. 255 (the range then holds no usable rows), flags[1]: the largest |row|^2.  Synchronous.  A train
// collection (api_collection.hip) places its images with it.  dev != nullptr: the rows are dev's, read in place (`rows` and
// `f32` are ignored; only the flag words live in ws_in).
int fm::bank_prep_range(fm_ctx* ctx, const void* rows, int64_t n, int dim, bool f32, Bank& b, int64_t off, int64_t n_pad, int* flags,
                        const DevSrc* dev)
{
    const size_t src_bytes = dev ? 0 : (size_t)n * dim * (f32 ? 4 : 1), flag_off = (src_bytes + 15) & ~(size_t)15;
    int rc = ws_ensure(ctx, &ctx->ws_in, &ctx->ws_in_bytes, flag_off + 32);
    if (rc != FM_OK) return rc;
    int* d_flag = (int*)((char*)ctx->ws_in + flag_off);
    if (src_bytes) HIP_TRY(ctx, hipMemcpyAsync(ctx->ws_in, rows, src_bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(d_flag, 0, 8, ctx->stream));
    const int64_t ntiles = n_pad / kTileRows;
    if (dev) {
        Bank v = bank_rows_view(b, off, n);
        HIP_TRY(ctx, launch_bank_prep_dev(*dev, n, dim, v, d_flag, (int)ntiles, ctx->stream));
    } else if (f32)
        hipLaunchKernelGGL(bank_prep_kernel<true>, dim3((unsigned)ntiles), dim3(256), 0, ctx->stream, (const void*)ctx->ws_in, n, dim,
                           b.rows8 + (size_t)off * kDim, b.norm + off, b.aux + (off / kTileRows) * kAuxPerTile, d_flag, ntiles);
    else
        hipLaunchKernelGGL(bank_prep_kernel<false>, dim3((unsigned)ntiles), dim3(256), 0, ctx->stream, (const void*)ctx->ws_in, n, dim,
                           b.rows8 + (size_t)off * kDim, b.norm + off, b.aux + (off / kTileRows) * kAuxPerTile, d_flag, ntiles);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(flags, d_flag, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return FM_OK;
}

// ---- a float32-route bank that grows (r05: lazy targets with descriptors that are not integer valued) -----------------
// Rows of the new range: largest finite magnitude (float bits) in stat[0], stat[1] |= 1 for a value that is not finite.
__global__ __launch_bounds__(256)
void bank_append_f32_kernel(const float* __restrict__ src, int64_t n, int dim, float* __restrict__ dst, int* __restrict__ stat)
{
    float m = 0.f;
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n * kDim; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i / kDim;
        const int k = (int)(i % kDim);
        const float v = k < dim ? src[row * dim + k] : 0.f;
        dst[i] = v;
        const bool fin = fabsf(v) <= 3.0e38f;
        bad |= !fin;
        m = fin ? fmaxf(m, fabsf(v)) : m;
    }
#pragma unroll
    for (int mask = 1; mask < 64; mask <<= 1) m = fmaxf(m, __shfl_xor(m, mask));
    if (__builtin_amdgcn_ballot_w64(bad) != 0ull && (threadIdx.x & 63) == 0) atomicOr(stat + 1, 1);
    if ((threadIdx.x & 63) == 0) atomicMax(stat, (int)__float_as_uint(m));
}

// An EMPTY float32-route bank with room for `capacity` rows.  The fp16 planes of a bank are scaled by ONE power of two
// chosen from the bank's largest magnitude (filter_f16.hip); a bank that grows cannot know its own, so it takes the
// scale of `scale_like` -- the bank it will be matched against (the query image's: same extractor, same value range).
// Every row is prepared as a padding row; fm_bank_append_f32 turns ranges of them into real ones.
extern "C" int fm_bank_create_f32_cap(fm_ctx* ctx, int dim, int64_t capacity, const fm_bank* scale_like, fm_bank** out)
{
    if (!ctx) return fail(nullptr, FM_EINVAL, "fm_bank_create_f32_cap: ctx is NULL");
    if (!out) return fail(ctx, FM_EINVAL, "fm_bank_create_f32_cap: bank out pointer is NULL");
    *out = nullptr;
    if (dim < 1 || dim > kDim || capacity < 1 || capacity > (int64_t)INT32_MAX - 2 * kStageRows)
        return fail(ctx, FM_EINVAL, "fm_bank_create_f32_cap: bad dim / capacity");
    if (int rc = refuse_bin2(ctx, scale_like, "fm_bank_create_f32_cap")) return rc;
    if (!scale_like || scale_like->kind != FM_BANK_F32 || !scale_like->filt_ok)
        return fail(ctx, FM_EINVAL, "fm_bank_create_f32_cap: scale_like must be a float32-route bank of finite values");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    fm_bank* b = new (std::nothrow) fm_bank();
    if (!b) return fail(ctx, FM_ENOMEM, "fm_bank_create_f32_cap: out of host memory");
    b->kind = FM_BANK_F32;
    b->n = 0;
    b->dim = dim;
    b->n_pad = kStageRows;
    b->cap_pad = ((capacity + kStageRows - 1) / kStageRows) * kStageRows;
    b->kscale = scale_like->kscale;
    b->filt_ok = true;
    b->nm_max = 0.f;
    auto bail = [&](hipError_t e, const char* what) {
        (void)hipGetLastError();
        bank_free(b); delete b;
        return fail(ctx, e == hipErrorOutOfMemory ? FM_ENOMEM : FM_EDEVICE, std::string("fm_bank_create_f32_cap: ") + what + ": " + hipGetErrorString(e));
    };
    hipError_t e;
    if ((e = hipMalloc((void**)&b->rowsf, (size_t)b->cap_pad * kDim * 4)) != hipSuccess) return bail(e, "rows");
    if ((e = hipMalloc((void**)&b->rowsh, (size_t)b->cap_pad * kDim * 2)) != hipSuccess) return bail(e, "fp16 rows");
    if ((e = hipMalloc((void**)&b->normf, (size_t)b->cap_pad * 4)) != hipSuccess) return bail(e, "norms");
    if ((e = hipMalloc((void**)&b->auxf, (size_t)b->cap_pad * 4)) != hipSuccess) return bail(e, "aux");
    if ((e = hipMemsetAsync(b->rowsf, 0, (size_t)b->cap_pad * kDim * 4, ctx->stream)) != hipSuccess) return bail(e, "fill");
    int rc = ws_ensure(ctx, &ctx->ws_in, &ctx->ws_in_bytes, 64);
    if (rc != FM_OK) { bank_free(b); delete b; return rc; }
    // (n = 0: every row comes out as a padding row -- zero fp16 row, norm 0, accumulator init -3.4e38)
    hipLaunchKernelGGL(bank_prep_f16_kernel, dim3((unsigned)(b->cap_pad / 16)), dim3(256), 0, ctx->stream,
                       (const float*)b->rowsf, (int64_t)0, b->cap_pad, b->kscale, b->rowsh, b->normf, b->auxf, (int*)ctx->ws_in);
    if ((e = hipGetLastError()) != hipSuccess || (e = hipStreamSynchronize(ctx->stream)) != hipSuccess) return bail(e, "prepare");
    *out = b;
    return FM_OK;
}

// n more rows at the next multiple of 32 rows, as fm_bank_append_u8.  FM_EUNSUPPORTED (the bank unchanged, its rows past
// bank->n rewritten as padding) when a value is not finite or, scaled by the bank's fixed power of two, leaves fp16's range.
extern "C" int fm_bank_append_f32(fm_ctx* ctx, fm_bank* bank, const float* rows, int64_t n, int64_t* first_row)
{
    if (!ctx || !bank) return fail(ctx, FM_EINVAL, "fm_bank_append_f32: NULL argument");
    if (int rc = refuse_bin(ctx, bank, "fm_bank_append_f32")) return rc;
    if (bank->kind != FM_BANK_F32 || !bank->rowsf || !bank->rowsh || bank->cap_pad <= 0)
        return fail(ctx, FM_EINVAL, "fm_bank_append_f32: not a float32-route bank with capacity (fm_bank_create_f32_cap)");
    if (n < 0 || (n > 0 && !rows)) return fail(ctx, FM_EINVAL, "fm_bank_append_f32: bad rows / n");
    const int64_t off = ((bank->n + kTileRows - 1) / kTileRows) * kTileRows;
    if (first_row) *first_row = off;
    if (n == 0) return FM_OK;
    if (off + n > bank->cap_pad) return fail(ctx, FM_EINVAL, "fm_bank_append_f32: the bank's capacity is used up");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t src_bytes = (size_t)n * bank->dim * 4, flag_off = (src_bytes + 15) & ~(size_t)15;
    int rc = ws_ensure(ctx, &ctx->ws_in, &ctx->ws_in_bytes, flag_off + 32);
    if (rc != FM_OK) return rc;
    if ((rc = bank_real_gap(ctx, bank, off)) != FM_OK) return rc;     // (a refused append below leaves the marks of the rows so far: harmless)
    int* d_flag = (int*)((char*)ctx->ws_in + flag_off);
    HIP_TRY(ctx, hipMemcpyAsync(ctx->ws_in, rows, src_bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(d_flag, 0, 16, ctx->stream));
    float* dst = bank->rowsf + (size_t)off * kDim;
    hipLaunchKernelGGL(bank_append_f32_kernel, dim3((unsigned)std::min<int64_t>(1024, (n * kDim + 255) / 256)), dim3(256), 0, ctx->stream,
                       (const float*)ctx->ws_in, n, bank->dim, dst, d_flag);
    HIP_TRY(ctx, hipGetLastError());
    int stat[2] = {0, 0};
    HIP_TRY(ctx, hipMemcpyAsync(stat, d_flag, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    float vmax = 0.f;
    memcpy(&vmax, &stat[0], 4);
    const int64_t n16 = ((n + 15) / 16) * 16;                 // (the range's rows up to a multiple of 16: padding again)
    const bool ok = stat[1] == 0 && ldexpf(vmax, bank->kscale) < 60000.f;
    HIP_TRY(ctx, hipMemsetAsync(d_flag + 2, 0, 8, ctx->stream));
    if (!ok) HIP_TRY(ctx, hipMemsetAsync(dst, 0, (size_t)n * kDim * 4, ctx->stream));
    hipLaunchKernelGGL(bank_prep_f16_kernel, dim3((unsigned)(n16 / 16)), dim3(256), 0, ctx->stream,
                       (const float*)dst, ok ? n : (int64_t)0, n16, bank->kscale, bank->rowsh + (size_t)off * kDim, bank->normf + off,
                       bank->auxf + off, d_flag + 2);
    HIP_TRY(ctx, hipGetLastError());
    if (ok && (rc = bank_real_append(ctx, bank, off, n)) != FM_OK) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(stat, d_flag + 2, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (!ok)
        return fail(ctx, FM_EUNSUPPORTED, "fm_bank_append_f32: a value is not finite or leaves the fp16 range under the bank's scale (2^" +
                                          std::to_string(bank->kscale) + "): the growing bank cannot take these rows");
    float nmx = 0.f;
    memcpy(&nmx, &stat[0], 4);
    if (nmx > bank->nm_max) bank->nm_max = nmx;
    if (vmax > bank->vfin_max) bank->vfin_max = vmax;
    bank->n = off + n;
    bank->n_pad = ((bank->n + kStageRows - 1) / kStageRows) * kStageRows;
    return FM_OK;
}

// Float32-route rows [off, off + n_pad) of a bank's arrays (train collections): the n host rows into rowsf (zero rows behind
// them), *vmax = their largest finite magnitude, *finite = every value is finite.  Then bank_f32_range_planes: the fp16 planes of
// the range under b.kscale (rows from n on: padding), *nm_max = the largest scaled norm.  Both synchronous.  dev != nullptr:
// the rows are dev's (float32, half or bfloat16), read in place; `rows` is ignored.
int fm::bank_f32_range_rows(fm_ctx* ctx, const float* rows, int64_t n, int dim, Bank& b, int64_t off, int64_t n_pad, float* vmax, bool* finite,
                            const DevSrc* dev)
{
    const size_t src_bytes = dev ? 0 : (size_t)n * dim * 4, flag_off = (src_bytes + 15) & ~(size_t)15;
    int rc = ws_ensure(ctx, &ctx->ws_in, &ctx->ws_in_bytes, flag_off + 32);
    if (rc != FM_OK) return rc;
    int* d_flag = (int*)((char*)ctx->ws_in + flag_off);
    float* dst = b.rowsf + (size_t)off * kDim;
    HIP_TRY(ctx, hipMemsetAsync(d_flag, 0, 16, ctx->stream));
    if (dev) {
        // the typed, pitched copy writes every row of the range (zeros behind the real rows and dims); the statistics are
        // bank_absmax_kernel's over the rows just written -- the zeros change neither
        Bank v = bank_rows_view(b, off, n);
        v.n_pad = n_pad;
        HIP_TRY(ctx, launch_bank_copy_dev(*dev, n, dim, v, ctx->stream));
        hipLaunchKernelGGL(bank_absmax_kernel, dim3((unsigned)std::min<int64_t>(1024, (n * kDim + 255) / 256)), dim3(256), 0, ctx->stream,
                           (const float*)dst, n * kDim, d_flag);
    } else {
        HIP_TRY(ctx, hipMemcpyAsync(ctx->ws_in, rows, src_bytes, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(dst, 0, (size_t)n_pad * kDim * 4, ctx->stream));
        hipLaunchKernelGGL(bank_append_f32_kernel, dim3((unsigned)std::min<int64_t>(1024, (n * kDim + 255) / 256)), dim3(256), 0, ctx->stream,
                           (const float*)ctx->ws_in, n, dim, dst, d_flag);
    }
    HIP_TRY(ctx, hipGetLastError());
    int stat[2] = {0, 0};
    HIP_TRY(ctx, hipMemcpyAsync(stat, d_flag, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(vmax, &stat[0], 4);
    *finite = stat[1] == 0;
    return FM_OK;
}

int fm::bank_f32_range_planes(fm_ctx* ctx, Bank& b, int64_t off, int64_t n, int64_t n_pad, float* nm_max)
{
    int rc = ws_ensure(ctx, &ctx->ws_in, &ctx->ws_in_bytes, 64);
    if (rc != FM_OK) return rc;
    int* d_flag = (int*)ctx->ws_in;
    HIP_TRY(ctx, hipMemsetAsync(d_flag, 0, 8, ctx->stream));
    hipLaunchKernelGGL(bank_prep_f16_kernel, dim3((unsigned)(n_pad / 16)), dim3(256), 0, ctx->stream,
                       (const float*)(b.rowsf + (size_t)off * kDim), n, n_pad, b.kscale, b.rowsh + (size_t)off * kDim, b.normf + off,
                       b.auxf + off, d_flag);
    HIP_TRY(ctx, hipGetLastError());
    int stat[2] = {0, 0};
    HIP_TRY(ctx, hipMemcpyAsync(stat, d_flag, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(nm_max, &stat[0], 4);
    return FM_OK;
}

// K11: a binary bank -- [n][bytes] packed rows, 1 <= bytes <= 64 -- for NORM_HAMMING (hamming.hip) or, kind FM_BANK_BIN2, for
// NORM_HAMMING2 (K11b, hamming2.hip): the same checks in the same order, the same packed plane, the tetrahedral FP4 image.
static int bank_create_bin(fm_ctx* ctx, const uint8_t* rows, int64_t n, int bytes, fm_bank** out, const DevSrc* dev = nullptr, int kind = FM_BANK_BIN)
{
    const std::string who = kind == FM_BANK_BIN2 ? "fm_bank_create_bin2" : "fm_bank_create_bin";
    if (!ctx) return fail(nullptr, FM_EINVAL, who + ": ctx is NULL");
    if (!out) return fail(ctx, FM_EINVAL, who + ": bank out pointer is NULL");
    *out = nullptr;
    if (n < 0 || bytes < 1 || (n > 0 && !rows && !dev)) return fail(ctx, FM_EINVAL, who + ": bad rows/n/bytes");
    if (bytes > 64) return fail(ctx, FM_EUNSUPPORTED, who + ": binary rows of more than 64 bytes (512 bits) are not supported");
    if (n > (int64_t)INT32_MAX - 2 * kStageRows) return fail(ctx, FM_EUNSUPPORTED, who + ": n too large");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    fm_bank* b = new (std::nothrow) fm_bank();
    if (!b) return fail(ctx, FM_ENOMEM, who + ": out of host memory");
    b->kind = kind;
    b->n = n;
    b->dim = bytes;
    b->ksteps = (bytes + 15) / 16;
    b->ksteps4 = kind == FM_BANK_BIN2 ? ham2_fp4_steps(bytes) : b->ksteps;
    b->n_pad = ((n + kStageRows - 1) / kStageRows) * kStageRows;
    if (b->n_pad == 0) b->n_pad = kStageRows;
    b->cap_pad = b->n_pad;
    auto bail = [&](hipError_t e, const char* what) {
        (void)hipGetLastError();
        bank_free(b); delete b;
        return fail(ctx, e == hipErrorOutOfMemory ? FM_ENOMEM : FM_EDEVICE, std::string(who + ": ") + what + ": " + hipGetErrorString(e));
    };
    hipError_t e;
    if ((e = hipMalloc((void**)&b->rowsb, (size_t)b->n_pad * b->ksteps * 16)) != hipSuccess) return bail(e, "packed rows");
    if ((e = hipMalloc((void**)&b->rows4, (size_t)b->n_pad * b->ksteps4 * 64)) != hipSuccess) return bail(e, "FP4 rows");
    if (dev) {
        // (device rows: the preparation kernel reads them in place, at the caller's pitch)
        if ((e = (kind == FM_BANK_BIN2 ? launch_hamming2_prep : launch_hamming_prep)(dev->rows, n, bytes, *b, ctx->stream, dev->pitch)) != hipSuccess) return bail(e, "prepare");
    } else {
        const size_t src_bytes = (size_t)n * bytes;
        int rc = ws_ensure(ctx, &ctx->ws_in, &ctx->ws_in_bytes, src_bytes + 64);
        if (rc != FM_OK) { bank_free(b); delete b; return rc; }
        if (src_bytes && (e = hipMemcpyAsync(ctx->ws_in, rows, src_bytes, hipMemcpyHostToDevice, ctx->stream)) != hipSuccess) return bail(e, "upload");
        if ((e = (kind == FM_BANK_BIN2 ? launch_hamming2_prep : launch_hamming_prep)((const uint8_t*)ctx->ws_in, n, bytes, *b, ctx->stream, 0)) != hipSuccess) return bail(e, "prepare");
    }
    if ((e = hipStreamSynchronize(ctx->stream)) != hipSuccess) return bail(e, "prepare");
    *out = b;
    return FM_OK;
}

extern "C" int fm_bank_create_bin(fm_ctx* ctx, const uint8_t* rows, int64_t n, int bytes, fm_bank** out)
{
    return bank_create_bin(ctx, rows, n, bytes, out);
}

extern "C" int fm_bank_create_bin2(fm_ctx* ctx, const uint8_t* rows, int64_t n, int bytes, fm_bank** out)
{
    return bank_create_bin(ctx, rows, n, bytes, out, nullptr, FM_BANK_BIN2);
}

// A bank from rows that are already in device memory (include/fastmatch_hip.h: "device sources").  The preparation kernels
// read the caller's memory in place behind an event recorded on producer_stream; every creator synchronises the context's
// stream before it returns (the flag words come back), so the source is not read after the call.
extern "C" int fm_bank_create_dev(fm_ctx* ctx, const void* d_rows, int dtype, int64_t n, int dim, int64_t row_pitch_bytes,
                                  int float_route, void* producer_stream, fm_bank** bank)
{
    if (!ctx) return fail(nullptr, FM_EINVAL, "fm_bank_create_dev: ctx is NULL");
    if (!bank) return fail(ctx, FM_EINVAL, "fm_bank_create_dev: bank out pointer is NULL");
    *bank = nullptr;
    if (dtype < FM_DT_U8 || dtype > FM_DT_BIN2)
        return fail(ctx, FM_EINVAL, "fm_bank_create_dev: unknown dtype " + std::to_string(dtype) + " (FM_DT_U8 .. FM_DT_BIN2)");
    if (n < 0 || dim < 1) return fail(ctx, FM_EINVAL, "fm_bank_create_dev: bad n / dim");
    if ((dtype == FM_DT_BIN || dtype == FM_DT_BIN2) && dim > 64)
        return fail(ctx, FM_EUNSUPPORTED, "fm_bank_create_dev: binary rows of more than 64 bytes (512 bits) are not supported");
    if (dim > (dtype == FM_DT_U8 ? kDim : kWideDim))
        return fail(ctx, FM_EUNSUPPORTED, dtype == FM_DT_U8 ? "fm_bank_create_dev: dim > 128 is not supported"
                                                            : "fm_bank_create_dev: dim > 256 is not supported");
    const int64_t elt = dtype == FM_DT_F32 ? 4 : (dtype == FM_DT_F16 || dtype == FM_DT_BF16) ? 2 : 1;
    const int64_t pitch = row_pitch_bytes == 0 ? dim * elt : row_pitch_bytes;
    if (pitch < dim * elt)
        return fail(ctx, FM_EINVAL, "fm_bank_create_dev: row_pitch_bytes " + std::to_string(row_pitch_bytes) + " is below the row size " +
                                    std::to_string(dim * elt));
    if (pitch % elt != 0) return fail(ctx, FM_EINVAL, "fm_bank_create_dev: row_pitch_bytes is not a multiple of the element size");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (n > 0) {
        if (!d_rows) return fail(ctx, FM_EINVAL, "fm_bank_create_dev: d_rows is NULL");
        if ((uintptr_t)d_rows % (uintptr_t)elt != 0) return fail(ctx, FM_EINVAL, "fm_bank_create_dev: d_rows is not aligned to the element size");
        int rc;
        if ((rc = check_device_ptr(ctx, d_rows, "fm_bank_create_dev", "d_rows")) != FM_OK) return rc;
        // the rows are complete once the work producer_stream has been given so far is: no host wait for it
        if ((rc = wait_for_stream(ctx, producer_stream)) != FM_OK) return rc;
    }
    const DevSrc src{(const uint8_t*)d_rows, dtype, pitch};
    if (dtype == FM_DT_BIN) return bank_create_bin(ctx, nullptr, n, dim, bank, &src);
    if (dtype == FM_DT_BIN2) return bank_create_bin(ctx, nullptr, n, dim, bank, &src, FM_BANK_BIN2);
    return bank_create(ctx, nullptr, n, dim, dtype != FM_DT_U8, bank, float_route != 0 && dtype != FM_DT_U8, 0, nullptr, 0, &src);
}

extern "C" int fm_bank_create_f32(fm_ctx* ctx, const float* rows, int64_t n, int dim, fm_bank** bank)
{
    return bank_create(ctx, rows, n, dim, true, bank);
}

extern "C" int fm_bank_create_f32_route(fm_ctx* ctx, const float* rows, int64_t n, int dim, fm_bank** bank)
{
    return bank_create(ctx, rows, n, dim, true, bank, true);
}

// A new image's descriptors into an existing bank: no allocation, no host synchronisation.  The copy (DMA engine)
// and the preparation kernel run on the context's upload stream, beside whatever the other streams compute.
extern "C" int fm_bank_refill_u8_async(fm_ctx* ctx, fm_bank* bank, const uint8_t* rows, int64_t n)
{
    if (!ctx || !bank) return fail(ctx, FM_EINVAL, "fm_bank_refill_u8_async: NULL argument");
    if (int rc = refuse_bin(ctx, bank, "fm_bank_refill_u8_async")) return rc;
    if (bank->kind != FM_BANK_I8 || !bank->rows8) return fail(ctx, FM_EINVAL, "fm_bank_refill_u8_async: not an integer-route bank");
    if (n < 0 || (n > 0 && !rows)) return fail(ctx, FM_EINVAL, "fm_bank_refill_u8_async: bad rows / n");
    int64_t n_pad = ((n + kStageRows - 1) / kStageRows) * kStageRows;
    if (n_pad == 0) n_pad = kStageRows;
    if (n_pad > bank->cap_pad) return fail(ctx, FM_EINVAL, "fm_bank_refill_u8_async: more rows than the bank was created with");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!ctx->upload) {
        HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->upload, hipStreamNonBlocking));
        HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_upload, hipEventDisableTiming));
    }
    if (!bank->stage) HIP_TRY(ctx, hipMalloc(&bank->stage, (size_t)bank->cap_pad * kDim + 64));
    int* d_flag = (int*)((char*)bank->stage + (size_t)bank->cap_pad * kDim);
    if (n > 0) HIP_TRY(ctx, hipMemcpyAsync(bank->stage, rows, (size_t)n * bank->dim, hipMemcpyHostToDevice, ctx->upload));
    // (the flag words are scratch here: the largest row norm is not read back, see below -- no fill in front of the kernel)
    const int64_t ntiles = n_pad / kTileRows;
    const int64_t grid = ntiles < ctx->tune.refill_grid ? ntiles : ctx->tune.refill_grid;
    hipLaunchKernelGGL(bank_prep_kernel<false>, dim3((unsigned)grid), dim3(256), 0, ctx->upload,
                       (const void*)bank->stage, n, bank->dim, bank->rows8, bank->norm, bank->aux, d_flag, ntiles);
    HIP_TRY(ctx, hipGetLastError());
    bank->n = n;
    bank->n_pad = n_pad;
    bank->real = nullptr;           // (the new rows are dense: whatever gaps appends had left are gone; real_mem stays for the next one)
    if (bank->rows6) HIP_TRY(ctx, launch_prep6(*bank, ctx->tune.refill_grid, ctx->upload));       // (from the new int8 plane, behind it)
    // the largest row norm of the new rows is known on the device only: assume the float32-root guard is needed
    // (an election then launches one extra kernel that finds an empty list, ~5 us beside the next distance kernel)
    bank->usq_max = INT32_MAX / 2;
    return FM_OK;
}

extern "C" int fm_upload_fence(fm_ctx* ctx)
{
    if (!ctx) return fail(nullptr, FM_EINVAL, "fm_upload_fence: ctx is NULL");
    if (!ctx->upload) return FM_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipEventRecord(ctx->ev_upload, ctx->upload));
    HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_upload, 0));
    return FM_OK;
}

// Everything enqueued on the context -- its own stream and the tail streams the async entry points use.
void fm::sync_all_streams(fm_ctx* ctx)
{
    (void)hipSetDevice(ctx->device);
    if (ctx->upload) (void)hipStreamSynchronize(ctx->upload);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    for (hipStream_t ts : ctx->tails) if (ts) (void)hipStreamSynchronize(ts);
}

extern "C" int fm_bank_destroy(fm_ctx* ctx, fm_bank* bank)
{
    if (!bank) return FM_OK;
    if (ctx) sync_all_streams(ctx);          // (tail kernels of async calls read the bank's self distances)
    bank_free(bank);
    delete bank;
    return FM_OK;
}

extern "C" int fm_bank_info(const fm_bank* bank, int64_t* n, int* dim, int* kind)
{
    if (!bank) return fail(nullptr, FM_EINVAL, "fm_bank_info: bank is NULL");
    if (n) *n = bank->n;
    if (dim) *dim = bank->dim;
    if (kind) *kind = bank->kind;
    return FM_OK;
}

extern "C" int fm_bank_set_selfdist(fm_ctx* ctx, fm_bank* bank, const double* selfdist)
{
    if (!ctx || !bank) return fail(ctx, FM_EINVAL, "fm_bank_set_selfdist: NULL argument");
    if (int rc = refuse_bin(ctx, bank, "fm_bank_set_selfdist")) return rc;
    if (bank->n > 0 && !selfdist) return fail(ctx, FM_EINVAL, "fm_bank_set_selfdist: selfdist is NULL");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc;
    if ((rc = bank_selfdist_alloc(ctx, bank)) != FM_OK) return rc;
    bank->sdmax_rows = -1;
    if (bank->n > 0) HIP_TRY(ctx, hipMemcpyAsync(bank->selfdist, selfdist, (size_t)bank->n * 8, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = enqueue_selfdist_max(ctx, bank, ctx->stream)) != FM_OK) return rc;
    if (bank->n > 0) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return FM_OK;
}

int fm::table_host(fm_ctx* ctx, size_t bytes)
{
    if (ctx->tab_in_flight) { HIP_TRY(ctx, hipEventSynchronize(ctx->ev_tab)); ctx->tab_in_flight = false; }
    if (!ctx->ev_tab) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_tab, hipEventDisableTiming));
    if (bytes > ctx->h_tab_bytes) {
        if (ctx->h_tab) (void)hipHostFree(ctx->h_tab);
        ctx->h_tab = nullptr; ctx->h_tab_bytes = 0;
        const size_t want = bytes + bytes / 4 + 4096;
        HIP_TRY(ctx, hipHostMalloc((void**)&ctx->h_tab, want, hipHostMallocDefault));
        ctx->h_tab_bytes = want;
    }
    return FM_OK;
}

int fm::table_upload(fm_ctx* ctx, void* dst, size_t bytes)
{
    HIP_TRY(ctx, hipMemcpyAsync(dst, ctx->h_tab, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipEventRecord(ctx->ev_tab, ctx->stream));
    ctx->tab_in_flight = true;
    return FM_OK;
}

int fm::bank_selfdist_alloc(fm_ctx* ctx, fm_bank* b)
{
    if (b->selfdist) return FM_OK;
    const size_t cap = (size_t)(b->cap_pad > 0 ? b->cap_pad : 1);
    HIP_TRY(ctx, hipMalloc((void**)&b->selfdist, cap * 8 + 8));
    b->sdmax = (unsigned long long*)(b->selfdist + cap);
    b->sdmax_rows = -1;
    return FM_OK;
}

int fm::refuse_bin2(fm_ctx* ctx, const fm_bank* b, const char* who)
{
    if (!b || b->kind != FM_BANK_BIN2) return FM_OK;
    return fail(ctx, FM_EUNSUPPORTED, std::string(who) + ": NORM_HAMMING2 banks (FM_BANK_BIN2, fm_bank_create_bin2) are served by fm_knn2, fm_knn, "
                                      "fm_xcheck1, fm_knn2_ratio, fm_mutual_ratio, their _dev forms and fm_hamming_radius_match(_dev) only");
}

int fm::refuse_wide(fm_ctx* ctx, const fm_bank* b, const char* who)
{
    if (int rc = refuse_bin2(ctx, b, who)) return rc;
    if (!b || b->kind != FM_BANK_F32W) return FM_OK;
    return fail(ctx, FM_EUNSUPPORTED, std::string(who) + ": wide float banks (FM_BANK_F32W, 129 .. 256 values per row) are served by fm_knn2, "
                                          "fm_knn with k <= 2, fm_xcheck1, fm_knn2_ratio, fm_mutual_ratio, their _dev forms and the Wide Fast-Match calls (fm_wide_self_dist, "
                                          "fm_wide_set_selfdist, fm_wide_match_ratio, fm_wide_match_accepted), fm_wide_radius_match(_dev) and fm_wide_knn_masked(_dev) only");
}

int fm::refuse_bin(fm_ctx* ctx, const fm_bank* b, const char* who)
{
    if (int rc = refuse_wide(ctx, b, who)) return rc;
    if (!b || b->kind != FM_BANK_BIN) return FM_OK;
    return fail(ctx, FM_EUNSUPPORTED, std::string(who) + ": binary banks (FM_BANK_BIN, NORM_HAMMING) are served by fm_knn2, fm_knn, "
                                      "fm_xcheck1, fm_knn2_ratio, fm_hamming_radius_match and the Hamming Fast-Match calls (fm_hamming_self_dist, "
                                      "fm_hamming_set_selfdist, fm_hamming_match_ratio, fm_hamming_match_accepted) only");
}

int fm::check_pair(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, const char* who, bool bin_ok, bool bin2_ok)
{
    if (!ctx) return fail(nullptr, FM_EINVAL, std::string(who) + ": ctx is NULL");
    if (!q || !t) return fail(ctx, FM_EINVAL, std::string(who) + ": bank is NULL");
    // (NORM_HAMMING2: any other kind beside it is refused even for an empty bank -- FM_BANK_BIN of the same width included --
    // and a pair of them is served only where the entry point says so; both in front of the width check, so that the message
    // names the norm)
    if ((q->kind == FM_BANK_BIN2) != (t->kind == FM_BANK_BIN2))
        return fail(ctx, FM_EINVAL, std::string(who) + ": query/train kind mismatch (one bank is a NORM_HAMMING2 bank, FM_BANK_BIN2, the other is not)");
    if (q->kind == FM_BANK_BIN2 && !bin2_ok) return refuse_bin2(ctx, q, who);
    if (q->dim != t->dim) return fail(ctx, FM_EINVAL, std::string(who) + ": query/train dim mismatch");
    if (q->kind == FM_BANK_BIN2) return FM_OK;
    // (binary against non-binary is refused even for an empty bank: its rows would go to the L2 kernels)
    if ((q->kind == FM_BANK_BIN) != (t->kind == FM_BANK_BIN))
        return fail(ctx, FM_EINVAL, std::string(who) + ": query/train kind mismatch (one bank is binary, FM_BANK_BIN, the other is not)");
    if (!bin_ok && q->kind == FM_BANK_BIN) return refuse_bin(ctx, q, who);
    // (wide banks: the binary rule -- a dim mismatch was refused above, another kind is refused even for an empty bank: the
    // other routes index 128-wide planes)
    if ((q->kind == FM_BANK_F32W) != (t->kind == FM_BANK_F32W))
        return fail(ctx, FM_EINVAL, std::string(who) + ": query/train kind mismatch (one bank is a wide float bank, FM_BANK_F32W, the other is not)");
    if (!bin_ok && q->kind == FM_BANK_F32W) return refuse_bin(ctx, q, who);
    if (q->kind != t->kind && q->n > 0 && t->n > 0)      // (an empty bank has no kind of its own)
        return fail(ctx, FM_EINVAL, std::string(who) + ": query/train kind mismatch (one bank is integer-valued, the other is not)");
    return FM_OK;
}
