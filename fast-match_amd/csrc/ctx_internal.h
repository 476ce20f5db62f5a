// What the translation units behind the C-ABI share: the context object, error plumbing, workspace and
// device-to-host helpers.  api_ctx.hip (context, options, banks) defines the functions declared here;
// api_match.hip (2-NN, cross-check, batches, rounds), api_collection.hip and api_pairs.hip (train collections), api_expand.hip (K7 glue)
// and comm.hip (result gather) use them.  Internal: nothing here is part of include/fastmatch_hip.h.
#pragma once
#include "fm_internal.h"
#include "expand_pair.h"
#include "round_body_f32.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <initializer_list>
#include <mutex>
#include <vector>
#include <map>
#include <string>

struct fm_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev_call0 = nullptr, ev_call1 = nullptr, ev_k0 = nullptr, ev_k1 = nullptr;
    std::string err;
    std::string devname;
    // diagnostics on stderr, read from the environment ONCE when the context is created (FM_F32_DEBUG, FM_EXPAND_DEBUG,
    // FM_PARK_PROF); they print, they change nothing that is computed
    bool dbg_f32 = false, dbg_expand = false, dbg_park = false;
    // growable device workspaces
    void*  ws_partial = nullptr; size_t ws_partial_bytes = 0;
    void*  ws_out = nullptr;     size_t ws_out_bytes = 0;
    void*  ws_in = nullptr;      size_t ws_in_bytes = 0;
    // K10 (radius.hip): per-row arrays, the candidate keys of one query chunk, rocPRIM's temporary storage
    void*  ws_rrows = nullptr;   size_t ws_rrows_bytes = 0;
    void*  ws_rkeys = nullptr;   size_t ws_rkeys_bytes = 0;
    void*  ws_rtmp = nullptr;    size_t ws_rtmp_bytes = 0;
    // configuration: fm_ctx_set_option (the FM_* environment variables seed it at creation)
    fm::Tuning tune;
    int* d_counters = nullptr;   // device words of the fp16 filter (layout: fm_internal.h, launch_filter)
    unsigned* d_cut = nullptr;   // [2][kRRBatchMax] D* of the ratio test per pair of the next K1 launch (ratio_cut.h):
                                 // ratio_cut_kernel writes set `f6_set` on `stream` in front of the K1 that reads it; null: no cut
    // FP6 filter of the accepted-only sweeps (filter6.hip): the record lists and (count, need_k1) words of ONE launch's pairs,
    // twice.  fm_match_accepted_batch moves the rescoring and the guarded K1 of a launch to the last tail stream, beside the
    // NEXT launch's sweep on `stream`: consecutive launches alternate between the two sets (cut words, lists, counts), and a
    // launch waits for the rescoring that last used its set (ev_f6_done, recorded on that tail stream only; ev_f6_sweep, "the
    // sweep is done", on `stream` only).  Every other caller keeps the three kernels on `stream`.
    void*  ws_f6[2] = {nullptr, nullptr};  size_t ws_f6_bytes[2] = {0, 0};
    fm::Filter6Ws f6{nullptr, 0, nullptr};      // the set of the last launch
    int    f6_set = 0;                          // the set the last enqueue_ratio_cut chose
    hipEvent_t ev_f6_sweep[2] = {nullptr, nullptr}, ev_f6_done[2] = {nullptr, nullptr};
    bool   f6_off_stream[2] = {false, false};   // the set's last rescoring runs beside `stream`: ev_f6_done[set] orders its next user
    bool   cut_tau_ok = false;   // the last enqueue_ratio_cut had a tau that is not NaN
    int    ncu = 0;              // the device's CUs (the FP6 filter's split rule counts rounds of them)
    int    f6_last_n = 0;        // pairs of the last filter launch (options "fp6_records" / "fp6_fallbacks" read their words)
    int64_t filter_launches = 0;
    unsigned long long* h_scratch = nullptr;   // pinned host words the kernels can write (counts)
    // fm_collection_pairs_mutual_ratio: page-locked image of the call's slot tables and "its upload is done" -- a call that
    // returns without a host wait (the _dev form) leaves the copy in flight, the next call waits for it before it writes
    char*  h_tab = nullptr; size_t h_tab_bytes = 0;
    hipEvent_t ev_tab = nullptr; bool tab_in_flight = false;
    // page-locked staging for results that go to pageable caller memory (d2h below)
    char*  h_stage = nullptr; size_t h_stage_bytes = 0, h_stage_used = 0;
    struct StagedCopy { void* dst; size_t off, bytes; };
    std::vector<StagedCopy> staged;
    // calls enqueued without a synchronisation (fm_match_accepted_async): their events, read at fm_sync
    struct PendingTimer { hipEvent_t c0, c1, k0, k1; bool timed; int64_t pairs; bool call_timed = true; int64_t bytes = 0; };
    int64_t async_calls = 0;
    std::vector<PendingTimer> pending;       // in flight
    std::vector<PendingTimer> timer_pool;    // idle event sets
    // fm_match_accepted_async: K1 launches follow each other on `stream`; the small kernels behind a
    // K1 (election, decode + ratio, compaction) run on `stream_tail` and overlap the NEXT call's K1.
    // Two workspace slots alternate; a slot's tail kernels leave its bound[] and qbest[] arrays in
    // the state the next K1 / election expects, so no fill operations sit between two K1 launches.
    hipStream_t stream_tail = nullptr;      // = tails[0]
    static constexpr int kTails = 3;
    hipStream_t tails[kTails] = {nullptr, nullptr, nullptr};   // fm_match_accepted_batch spreads the pairs' tails over these
    hipStream_t rows_stream = nullptr;      // stream that produced the last device-resident rows (fm_gather_matches follows it)
    hipEvent_t ev_consumer = nullptr;
    // device sources and device results (fm_bank_create_dev, fm_knn_dev ...), created on first use: "the work this caller's
    // stream has been given so far" for the context's stream to wait on -- one event per caller stream, so that an event is
    // only ever re-recorded on the stream it was recorded on before (see ev_tail_end) -- and "the results are written", always
    // recorded on the context's stream, for the consumer stream to wait on
    std::map<hipStream_t, hipEvent_t> ev_foreign;
    hipEvent_t ev_results = nullptr;
    hipEvent_t ev_tail_end[3] = {nullptr, nullptr, nullptr};   // one per tail stream (an event re-recorded on another stream
                                                               // before its waiters ran is not a safe handshake)
    struct AsyncSlot {
        void* ws = nullptr; size_t bytes = 0;
        int64_t nq = -1, ncols_alloc = -1, partial_bytes = -1;   // layout the arrays were initialised for
        hipEvent_t tail_done = nullptr, k_done = nullptr;
        bool in_use = false;
    } aslot[2];
    int aslot_next = 0;
    std::vector<AsyncSlot> bslot;           // fm_match_accepted_batch: a ring of kBatchSlots workspaces
    static constexpr int kBatchSlots = 32;  // (two launches of up to 16 pairs in flight; a slot is re-used behind its tail's event)
    int64_t bslot_next = 0;
    // fm_mark / fm_wait: points in the enqueued work a caller can wait for without draining what follows
    static constexpr int kMarks = 8;
    struct Mark { hipEvent_t ev[1 + kTails] = {nullptr, nullptr, nullptr, nullptr}; int64_t id = -1; } marks[kMarks];
    int64_t next_mark = 0;
    void* comm = nullptr;        // RCCL communicator of the result gather (fm_comm_init)
    int   comm_ranks = 0;
    fm_stats stats{};
    int64_t stats_bytes = 0;     // fm_stats_ex::bytes_moved
    bool kernel_timed = false;
    int64_t pending_pairs = 0;
    int64_t pending_bytes = 0;   // algorithmic bytes of the launches in pending_pairs: bank rows read once
    // fm_bank_refill_u8_async / fm_upload_fence: uploads run on a stream of their own beside the kernels
    hipStream_t upload = nullptr;
    hipEvent_t ev_upload = nullptr;
    // fm_self_dist: plans of the triangular sweep by (padded rows, stages per workgroup) -- numbers only, no device memory
    std::map<std::pair<int64_t, int>, fm::TriPlan> tri_plans;
};

namespace fm {
// Algorithmic bytes of a bank in a distance-kernel launch: every row read once (128 B int8, 512 B float32, 1024 B wide
// float32, the packed row width of a binary bank).
static inline int64_t bank_bytes(const fm::Bank* b)
{
    if (!b) return 0;
    return b->n * (b->kind == FM_BANK_BIN || b->kind == FM_BANK_BIN2 ? b->dim : b->kind == FM_BANK_F32W ? 1024 : b->kind == FM_BANK_F32 ? 512 : 128);
}
}

namespace fm {      // (internal helpers live in the library's namespace: a host program may have a `fail` of its own)
int fail(fm_ctx* ctx, int code, const std::string& msg);
}

#define HIP_TRY(ctx, expr)                                                                  \
    do {                                                                                    \
        hipError_t _e = (expr);                                                             \
        if (_e != hipSuccess) {                                                             \
            char _b[512];                                                                   \
            snprintf(_b, sizeof(_b), "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                     __FILE__, __LINE__);                                                   \
            (void)hipGetLastError();                                                        \
            return fm::fail(ctx, _e == hipErrorOutOfMemory ? FM_ENOMEM : FM_EDEVICE, _b);       \
        }                                                                                   \
    } while (0)

// Ablation builds only (-DFM_ABLATE, scripts/ablate): FM_ABLATE_KEEP_BOUNDS leaves the bounds of a finished
// run in place (measures what the exact path costs).  The product build always resets them.
static inline bool ablate_keep_bounds()
{
#ifdef FM_ABLATE
    return getenv("FM_ABLATE_KEEP_BOUNDS") != nullptr;
#else
    return false;
#endif
}

namespace fm {
int ws_ensure(fm_ctx* ctx, void** p, size_t* cap, size_t need);
// The context's stream waits (on the device) for the work the caller's stream `s` has been given so far; FM_NO_STREAM: nothing.
int wait_for_stream(fm_ctx* ctx, void* s);
// p is device memory, and (same_device) on the context's device (FM_EINVAL with a message otherwise).  The accepted-rows
// entry points take any device's memory, as they always have: a peer buffer is a valid destination.
int check_device_ptr(fm_ctx* ctx, const void* p, const char* who, const char* what, bool same_device = true);
// Device-side alias of a page-locked host buffer (fm_host_alloc / hipHostMalloc), or NULL for pageable memory.
void* pinned_device_alias(const void* host);
// Device -> caller memory on the context's stream (through a copy kernel and, for pageable destinations, the
// context's page-locked staging buffer: moved to the caller by CallScope::finish()).
hipError_t d2h(fm_ctx* ctx, void* dst, const void* src, size_t bytes);
// The elements [0, n) of several columns (elem bytes per element each), copied down `piece` elements at a time, column after
// column: d2h's staging buffer grows to the largest single copy, so a large result comes down in pieces.
struct D2hColumn { void* dst; const void* src; size_t elem; };
inline hipError_t d2h_pieces(fm_ctx* ctx, size_t n, size_t piece, std::initializer_list<D2hColumn> cols)
{
    for (size_t o = 0; o < n; o += piece) {
        const size_t m = n - o < piece ? n - o : piece;
        for (const D2hColumn& c : cols) {
            const hipError_t e = d2h(ctx, (char*)c.dst + o * c.elem, (const char*)c.src + o * c.elem, m * c.elem);
            if (e != hipSuccess) return e;
        }
    }
    return hipSuccess;
}
// Account the calls that were enqueued without a synchronisation; the streams must be idle.
int drain_pending(fm_ctx* ctx);
// Everything enqueued on the context -- its own stream and the tail streams the async entry points use.
void sync_all_streams(fm_ctx* ctx);
// bin_ok: the entry point serves binary (FM_BANK_BIN) pairs; the others refuse them with FM_EUNSUPPORTED.  A binary bank
// paired with a non-binary one is FM_EINVAL, empty banks included.  Wide float banks (FM_BANK_F32W) follow the same two rules
// at the same entry points -- the bin_ok ones serve them (fm_knn: k <= 2) -- so every refusal of a wide bank is made here or
// in refuse_bin.
// NORM_HAMMING2 banks (FM_BANK_BIN2, K11b) are refused by DEFAULT: only an entry point that passes bin2_ok serves a pair of
// them (fm_knn2, fm_knn, fm_xcheck1, fm_knn2_ratio, fm_mutual_ratio, their _dev forms, fm_hamming_radius_match(_dev)); for every
// other one check_pair returns FM_EUNSUPPORTED with a message that names NORM_HAMMING2, whatever bin_ok says.  Such a bank
// paired with a bank of any other kind -- FM_BANK_BIN of the same width included -- is FM_EINVAL, empty banks included.
int check_pair(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, const char* who, bool bin_ok = false, bool bin2_ok = false);
// FM_EUNSUPPORTED for a binary or a wide float bank at an entry point that takes one bank (FM_OK otherwise)
int refuse_bin(fm_ctx* ctx, const fm_bank* b, const char* who);
// FM_EUNSUPPORTED for a wide float bank alone: the entry points that do serve binary banks (the collections' query banks).
// (A NORM_HAMMING2 bank is refused here too -- refuse_bin2 -- so every caller of refuse_wide or refuse_bin turns it away.)
int refuse_wide(fm_ctx* ctx, const fm_bank* b, const char* who);
// FM_EUNSUPPORTED, naming NORM_HAMMING2, for a FM_BANK_BIN2 bank (FM_OK otherwise): the entry points that do not go through
// check_pair, refuse_bin or refuse_wide call it in front of their own kind checks
int refuse_bin2(fm_ctx* ctx, const fm_bank* b, const char* who);
static inline bool bin_or_wide(const fm_bank* b) { return b->kind == FM_BANK_BIN || b->kind == FM_BANK_BIN2 || b->kind == FM_BANK_F32W; }
// Planes and scale terms of a (query = reduced, train = output rows) pair of float32 banks for x1_round_f32.
void fill_round_f32(fm::RoundF32* r, const fm::Bank& q, const fm::Bank& t);
// One expansion round's cross-checked 1-NN on the whole GPU (K7's delegated cross-check, api_match.hip).
// K10: radiusMatch (radius.hip); arguments checked by the entry points -- fm_radius_match(_dev) (api_match.hip),
// fm_collection_radius_match(_dev) (api_collection.hip), and their Hamming forms fm_hamming_radius_match(_dev),
// fm_collection_hamming_radius_match(_dev): two binary banks take radius_match's Hamming route; and the wide forms
// fm_wide_radius_match(_dev), fm_collection_wide_radius_match(_dev): two wide float banks (or a wide query bank and a wide
// collection's stack) take its wide route.
struct CollTab;      // coll_tab.h
struct RadiusArgs {
    const char* who;
    const float* radius; float radius_all;       // per-row radii (host; dev: device memory, read in place) or null
    int64_t cap;
    int64_t* offsets; int32_t* img; int32_t* idx; float* dist;    // host arrays; dev: the caller's device arrays (img: collections)
    int64_t* n_total;                            // host, may be null
    bool dev; void* consumer;                    // device form, and the stream it is ordered against (FM_NO_STREAM: none)
    const CollTab* tab; int64_t real_rows;       // t is a collection's stack: its lookup tables and its real rows; null: a plain bank
    const unsigned long long* mask = nullptr;    // the masked entry points: fm_mask's words [q.n][mwords] over t's padded rows,
    int64_t mwords = 0;                          // checked against q and t by the caller; null: every pair is permitted
};
int radius_match(fm_ctx* ctx, const fm::Bank& q, const fm::Bank& t, const RadiusArgs& a);
// Source rows that are already in device memory (fm_bank_create_dev, fm_collection_add_dev): n rows of FM_DT_* elements,
// `pitch` bytes apart, read in place by the *_dev_kernel variants of the preparation kernels.
struct DevSrc { const uint8_t* rows; int dtype; int64_t pitch; };
// Prepared rows of an integer-route bank's arrays from host rows -- or from dev's rows -- at a 128-row offset (api_ctx.hip;
// train collections)
int bank_prep_range(fm_ctx* ctx, const void* rows, int64_t n, int dim, bool f32, Bank& b, int64_t off, int64_t n_pad, int* flags,
                    const DevSrc* dev = nullptr);
int bank_f32_range_rows(fm_ctx* ctx, const float* rows, int64_t n, int dim, Bank& b, int64_t off, int64_t n_pad, float* vmax, bool* finite,
                        const DevSrc* dev = nullptr);
// *vmax = the largest finite magnitude of a float32 / half / bfloat16 device source (0 for none).  Synchronous: four bytes come back.
int dev_src_absmax(fm_ctx* ctx, const DevSrc& d, int64_t n, int dim, float* vmax);
int bank_f32_range_planes(fm_ctx* ctx, Bank& b, int64_t off, int64_t n, int64_t n_pad, float* nm_max);
// A bank's self distances, and its largest one (Bank::sdmax), in place: the array is allocated once, the word behind it.
int bank_selfdist_alloc(fm_ctx* ctx, fm_bank* b);
// The context's page-locked table buffer (fm_ctx::h_tab), the one protocol of every call that builds workgroup or slot tables
// on the host.  table_host: room for `bytes` bytes in it, once the last upload from it has been read (ev_tab): the caller
// then writes ctx->h_tab.  table_upload: its first `bytes` bytes to `dst` (device memory) on the context's stream; the buffer
// stays in flight until ev_tab, which the next table_host waits for -- a call may return without a host wait.
int table_host(fm_ctx* ctx, size_t bytes);
int table_upload(fm_ctx* ctx, void* dst, size_t bytes);
// Bank::sdmax of the rows [0, n) of b->selfdist, enqueued on `stream` (sets sdmax_rows).
int enqueue_selfdist_max(fm_ctx* ctx, fm_bank* b, hipStream_t stream);
int round_xcheck_dense(fm_ctx* ctx, const fm::Bank& q, const int32_t* d_rows, int64_t nq, const fm::Bank& t, int64_t t0, int64_t nt,
                       unsigned long long* d_qbest);
}

// Float32 route of a top-KTOP row-reduce (api_match.hip): K5 alone, or the fp16 filter (K8) with K5 as its conditional fallback;
// leaves the packed keys in ctx->ws_partial in *pl_out's layout.
int rowreduce_f32_route(fm_ctx* ctx, const fm_bank* cols, const fm_bank* red, int ktop, fm::RowReducePlan* pl_out, bool self = false);

// ---- one (output bank, reduced bank) pair swept on the context's stream (api_match.hip) ----------------------------------
// The tie list of the float32-root repair (tile_ops.h: kSqrtTieMin): fix[0] = count, rows from fix[4] on.
constexpr int kFixGrid = 1024;                 // workgroups of a sqrt_fix_kernel launch (each walks the list)
static inline size_t fix_bytes(int64_t rows) { return ((size_t)rows * 4 + 16 + 15) & ~(size_t)15; }

// What the small kernels behind a sweep read: the packed keys in ctx->ws_partial, laid out partial | bounds | tie list.
struct PairSweep {
    const unsigned long long* partial;   // ctx->ws_partial: [nsplit][ncols_alloc][ktop] keys, ascending per row
    int nsplit, ncols_alloc;
    int f32_keys;                        // high word = float32 distance bits (float32 route, binary) or the exact d2 (integer route)
    unsigned* fix;                       // zeroed tie list of fix_rows rows: integer-route pairs for which sqrt_tie_possible()
                                         // holds, and only when asked for; else null
    int* bound;                          // the integer route's shared bounds, [ktop][ncols_alloc] words, or null (one split, "coop" 0)
    fm::RowReducePlan rr;                // (sweep_pair_run's: the integer route's plan / K11's)
    fm::HamPlan ham;
};
enum : unsigned {
    kSweepNoEvents = 1u,   // ev_k0 / ev_k1 are the caller's: it brackets several sweeps, or none (rowreduce_f32_route still records its own)
    kSweepNoCount  = 2u,   // pending_pairs / pending_bytes are the caller's (a collection counts real rows, not the stack's)
};
// Top-ktop (1 or 2) of every row of `cols` over the rows of `red` by the route of the banks' kind: K1 / K2, the float32 route
// (rowreduce_f32_route), K11.  Sizes and carves ws_partial, re-arms the bounds, zeroes the tie list (fix_rows > 0: the rows
// the caller's merge or election may list), records ev_k0 / ev_k1 around the launch and accounts the pair.
// cut: launch_rowreduce's (integer route, top-1); stage_real: launch_hamming's.
int sweep_pair(fm_ctx* ctx, const fm::Bank& cols, const fm::Bank& red, int ktop, int64_t fix_rows, const unsigned* cut,
               const int* stage_real, unsigned flags, PairSweep* out);
// The two halves of sweep_pair, for a caller whose own kernel sits between them and fills out->bound itself (the delegated
// round's gather): plan + workspace, no stream work; then the launch.  Not for the float32 route, which sizes its own.
int sweep_pair_plan(fm_ctx* ctx, const fm::Bank& cols, const fm::Bank& red, int ktop, int64_t fix_rows, PairSweep* out);
int sweep_pair_run(fm_ctx* ctx, const fm::Bank& cols, const fm::Bank& red, int ktop, const unsigned* cut, const int* stage_real,
                   unsigned flags, const PairSweep& ps);
// D* of the ratio test for the pairs (q[i], -) of the next K1 launch on ctx->stream, into ctx->d_cut (api_match.hip); cut[i] = null
// for a pair without one.
int enqueue_ratio_cut(fm_ctx* ctx, int n, const fm_bank* const* q, double tau, const unsigned** cut);
// The FP6 filter's workspace for the next K1 launch of n pairs on ctx->stream (behind their enqueue_ratio_cut), or null: option
// "fp6_filter" 0, a NaN tau, no device memory -- K1 then runs as it always has.
const fm::Filter6Ws* filter6_ws(fm_ctx* ctx, int n);
// "The results are written": the consumer stream waits for what the context's stream has been given so far (api_match.hip).
int results_written(fm_ctx* ctx, void* consumer);
// Election of the cross-check (api_match.hip): per output row the minimum over the split partials, scatter-min into qbest.
__global__ void xcheck_scatter_kernel(const unsigned long long* __restrict__ partial, int nsplit,
                                      int ncols_alloc, int64_t nt,
                                      unsigned long long* __restrict__ qbest, unsigned t_offset, int f32,
                                      int* __restrict__ bound_reset, unsigned* __restrict__ fix);
// Lowe's ratio test on 2-NN lists (api_match.hip; api_collection.hip runs it on a collection's lists)
__global__ void lowe_kernel(const int32_t* __restrict__ idx2, const float* __restrict__ dist2, int64_t nq,
                            double tau, int32_t* __restrict__ tidx, float* __restrict__ dist,
                            double* __restrict__ ratio, uint8_t* __restrict__ pass,
                            int* __restrict__ block_counts);

// ---- ordered compaction of the accepted rows (compact_kernel, compact_rows_kernel, coll_compact_kernel) ------------------
// A 256-thread block's count of accepted rows from its ballots `m`, for the compaction behind it (256-thread blocks).
__device__ __forceinline__ void emit_block_count(unsigned long long m, int* __restrict__ block_counts)
{
    __shared__ int wave_cnt[4];
    if ((threadIdx.x & 63) == 0) wave_cnt[threadIdx.x >> 6] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) block_counts[blockIdx.x] = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
}

// The rank of this thread's flag p among the set flags of the blocks 0 .. blk in thread order (this block is number blk of
// block_counts): block b sums the counts of the blocks before it, every set flag takes offset + rank.  Deterministic (no
// atomics).  *total: the set flags up to and including this block's -- in the last block, all of them.
__device__ __forceinline__ int64_t compact_rank(const int* __restrict__ block_counts, int blk, bool p, int64_t* total)
{
    __shared__ int red[256];
    __shared__ int wave_cnt[4];
    const int tid = threadIdx.x;
    int s = 0;
    for (int b = tid; b < blk; b += 256) s += block_counts[b];
    red[tid] = s;
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) {
        if (tid < d) red[tid] += red[tid + d];
        __syncthreads();
    }
    const int64_t base = red[0];
    const unsigned long long m = __ballot(p);
    const int lane = tid & 63, wave = tid >> 6;
    if (lane == 0) wave_cnt[wave] = __popcll(m);
    __syncthreads();
    int wb = 0;
    for (int w = 0; w < wave; ++w) wb += wave_cnt[w];
    *total = base + wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
    return base + wb + __popcll(m & ((1ull << lane) - 1ull));
}

// Row q = this thread's row of pass[0 .. nq), *p: it is accepted, and then its slot in the compacted arrays (ascending row
// index): compact_rank under a grid of one block per 256 rows.
__device__ __forceinline__ int64_t compact_slot(const int* __restrict__ block_counts, const uint8_t* __restrict__ pass, int64_t nq,
                                                int64_t* q, bool* p, int64_t* total)
{
    *q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    *p = *q < nq && pass[*q];
    return compact_rank(block_counts, (int)blockIdx.x, *p, total);
}

// ---- mutual nearest neighbours + ratio test (fm_mutual_ratio, fm_collection_mutual_ratio_each; api_match.hip) -----------------
// The kernels work on entries e = image * nq + query row in one flat grid of n_images * nblk 256-thread blocks (block b:
// image b / nblk, rows from (b % nblk) * 256; nblk = ceil(nq / 256); a bank pair is one image); block counts are [image][nblk],
// the layout emit_block_count leaves under such a grid and coll_each_compact_kernel reads.  A CANDIDATE is an entry that
// passed the forward ratio test; its index is its rank among the passing entries in entry order.
// Lowe's test on per-image 2-NN lists [n_images][nq][2]: lowe_kernel's rule, word for word, per entry.
__global__ __launch_bounds__(256) void lowe_each_kernel(const int32_t* __restrict__ idx2, const float* __restrict__ dist2, int64_t nq, int nblk,
                                 double tau, int32_t* __restrict__ tidx, float* __restrict__ dist,
                                 double* __restrict__ ratio, uint8_t* __restrict__ pass, int* __restrict__ block_counts);
// cand_rows[candidate] = the train row whose reverse neighbours decide it: first_row[image] + tidx[entry] (first_row null:
// tidx itself); *n_cand = the number of candidates.
__global__ __launch_bounds__(256) void mutual_cand_kernel(const int32_t* __restrict__ tidx, const uint8_t* __restrict__ pass,
                                   const int* __restrict__ block_counts, int64_t nq, int nblk,
                                   const int32_t* __restrict__ first_row, int32_t* __restrict__ cand_rows,
                                   unsigned long long* __restrict__ n_cand);
// The join: a candidate is kept iff the nearest query row of its train row (r_idx / r_dist [n_cand][2], fm_knn2's lists of the
// gathered rows over the query bank) is its own and, symmetric != 0, the reverse ratio passes too -- ratio[entry] then
// becomes the larger of the two.  pass2 / block_counts2: the flags and counts of the final compaction.
__global__ __launch_bounds__(256) void mutual_join_kernel(const uint8_t* __restrict__ pass, const int* __restrict__ block_counts, int64_t nq, int nblk,
                                   const int32_t* __restrict__ r_idx, const float* __restrict__ r_dist, double tau, int symmetric,
                                   double* __restrict__ ratio, uint8_t* __restrict__ pass2, int* __restrict__ block_counts2);
namespace fm {
// Bytes of the gathered bank per candidate: every plane the sweeps read on the output side (integer route: rows8 + norm;
// float32 route: rowsf + rowsh + normf + auxf; wide float32: wrows + wrowsh + normf + auxf; binary: rowsb + rows4).
inline size_t mutual_row_bytes(const Bank& t)
{
    if (t.kind == FM_BANK_BIN2) return (size_t)t.ksteps * 16 + (size_t)fp4_steps(t) * 64;      // (the FP4 plane has its own step count)
    return t.kind == FM_BANK_F32W ? (size_t)kWideDim * 6 + 8 : t.kind == FM_BANK_F32 ? (size_t)kDim * 6 + 8 : t.kind == FM_BANK_BIN ? (size_t)t.ksteps * 80 : (size_t)kDim + 4;
}
constexpr size_t kMutualGatherBytes = (size_t)1 << 30;     // fm_mutual_ratio's budget for the gathered bank (a collection: "coll_ws_bytes")
// The reverse 2-NN lists of the candidates on the context's stream: the rows cand_rows[0 .. n_cand) of t's arrays gathered
// into a bank G in ws_in (in chunks of consecutive candidates of at most `budget` bytes, whole 128-row stages, at least
// one), then fm_knn2(G, q) -- the top-2 sweep of the pair's route with its float32-root repair -- into *r_idx / *r_dist
// [n_cand][2], which live in ws_in in front of G.  n_cand > 0, q->n > 0; t supplies planes and scale terms (upper bounds).
int mutual_reverse_device(fm_ctx* ctx, const Bank& t, const int32_t* cand_rows, int64_t n_cand, const fm_bank* q, size_t budget,
                          int32_t** r_idx, float** r_dist);
}

// ---- K13: k-NN under a mask (masked.hip; the collection forms in api_collection.hip) -----------------------------------------
// A mask is a device-resident bit matrix [nq][words] of 64-bit words over the PADDED rows of its train operand: a bank
// (one "image" at row 0) or a collection's physical stack (every image on its own 128-row stages, so an image's bits are
// whole words).  Bit b of word w of row i set = (query row i, train row 64 w + b) is permitted; the bits of padding rows
// are 0 always, which is why no masked kernel needs the per-stage real-row table.
struct fm_collection;
struct fm_mask {
    fm_ctx* ctx = nullptr;
    int64_t nq = 0, nt = 0;                 // query rows; REAL train rows (a collection: of all images)
    int64_t n_pad = 0, words = 0;           // padded train rows (a collection: the stack's used rows), n_pad / 64
    unsigned long long* bits = nullptr;
    size_t bytes = 0;
    const fm_collection* coll = nullptr;    // a collection's mask: the collection and its state at creation
    uint64_t coll_gen = 0;
    std::vector<int64_t> rows, phys;        // per image: real rows, first padded row
};
namespace fm {
// A zeroed mask for images of `rows` real rows at the padded rows `phys` (multiples of 128) of an operand of n_pad rows.
int mask_alloc(fm_ctx* ctx, int64_t nq, const std::vector<int64_t>& rows, const std::vector<int64_t>& phys, int64_t n_pad,
               const char* who, fm_mask** out);
// The masked k-NN lists of q over t (a bank, or a collection's stack) on the context's stream into d_idx / d_dist [nq][k]
// (rows of t; device memory): the masked MFMA sweep (integer route, k <= 2, option "masked_mfma") or the masked
// vector-ALU lists, then the merge.  q.n > 0; arguments checked by the entry points.
int knn_masked_device(fm_ctx* ctx, const Bank& q, const Bank& t, const fm_mask* m, int k, int32_t* d_idx, float* d_dist);
// The geometry / ownership checks of the masked calls that do not depend on the train operand's type.
int mask_check(fm_ctx* ctx, const fm_mask* m, const char* who);
}

// Brackets one API call: events for total time, stats accounting after the final sync.
struct CallScope {
    fm_ctx* ctx;
    ~CallScope() { ctx->staged.clear(); ctx->h_stage_used = 0; }
    explicit CallScope(fm_ctx* c) : ctx(c)
    {
        // entries left behind by a call that failed half way point at host memory that is gone
        ctx->staged.clear();
        ctx->h_stage_used = 0;
        ctx->kernel_timed = false;
        ctx->pending_pairs = 0;
        ctx->pending_bytes = 0;
        (void)hipEventRecord(ctx->ev_call0, ctx->stream);
    }
    int finish()
    {
        HIP_TRY(ctx, hipEventRecord(ctx->ev_call1, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        // (async calls still in flight finish on the tail stream: a synchronous call completes them too,
        // as the header promises; they are accounted at the next fm_sync / fm_get_stats)
        if (!ctx->pending.empty()) for (hipStream_t ts : ctx->tails) HIP_TRY(ctx, hipStreamSynchronize(ts));
        for (const auto& c : ctx->staged) memcpy(c.dst, ctx->h_stage + c.off, c.bytes);
        ctx->staged.clear();
        ctx->h_stage_used = 0;
        float ms = 0.f;
        HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev_call0, ctx->ev_call1));
        ctx->stats.total_ms += ms;
        ctx->stats.calls += 1;
        if (ctx->kernel_timed) {
            float kms = 0.f;
            HIP_TRY(ctx, hipEventElapsedTime(&kms, ctx->ev_k0, ctx->ev_k1));
            ctx->stats.kernel_ms += kms;
            ctx->stats.kernel_launches += 1;
            ctx->stats.pairs += ctx->pending_pairs;
            ctx->stats_bytes += ctx->pending_bytes;
        }
        return FM_OK;
    }
    // The end of a call whose compaction left its rows in device arrays (staged delivery): the count decides how much is
    // copied, so it is read first -- one tiny synchronous read; then m = min(count, cap) elements of every column, finish(),
    // and the full count for the caller.
    struct Column { void* dst; const void* src; size_t elem; };
    int finish_rows(const unsigned long long* d_count, int64_t cap, std::initializer_list<Column> cols, int64_t* n_accepted)
    {
        unsigned long long cnt = 0;
        HIP_TRY(ctx, hipMemcpyAsync(&cnt, d_count, 8, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        const size_t m = (size_t)((int64_t)cnt < cap ? (int64_t)cnt : cap);
        if (m) for (const Column& c : cols) HIP_TRY(ctx, fm::d2h(ctx, c.dst, c.src, m * c.elem));
        const int rc = finish();
        if (rc != FM_OK) return rc;
        if (n_accepted) *n_accepted = (int64_t)cnt;
        return FM_OK;
    }
};
