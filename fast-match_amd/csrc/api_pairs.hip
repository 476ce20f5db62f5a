// C-ABI of libfastmatch_hip.so (include/fastmatch_hip.h), part 2c: the match graph of a train collection --
// fm_collection_pairs_mutual_ratio(_dev) -- and, by the same machinery, a wide query bank against every image of a wide
// collection: fm_collection_wide_mutual_ratio_each(_dev), fm_collection_wide_knn2_each.  The collection itself, its storage
// and every call that takes one query bank against it: api_collection.hip (shared: coll_internal.h).
#include "coll_internal.h"
#include "pairs_plan.h"

#include <algorithm>

using namespace fm;

// ---------------------------------------------------------------------------------------
// image pairs INSIDE a collection (the match graph): fm_collection_pairs_mutual_ratio
// ---------------------------------------------------------------------------------------
// Pair p = (a, b), ordered: its rows are fm_mutual_ratio(bank(image a), bank(image b)).  Both images are resident bank views
// of the stack (coll_view), so a pair is two full top-2 sweeps -- slot 2j: output rows = image a, reduced = image b (the
// forward lists); slot 2j + 1: the other way round (the reverse lists of ALL rows of b: R2[t0] is a plain lookup, no gather,
// no candidate count, no host wait) -- then a join (rules 1 to 3 of fm_mutual_ratio from the two lists) and an ordered
// compaction into the packed output, fm_radius_match's layout with "pair" for "query row".
// Integer route: the slots of a whole chunk of pairs go through ONE table-driven launch of the batched top-2 kernel
// (launch_rowreduce_table2: descriptors in device memory) and ONE merge launch over per-slot row blocks; the float32-root
// repair is the existing per-slot kernel for the slots where sqrt_tie_possible holds.  Float32-route and binary
// collections: the two sweep_pair calls per pair (K8 / K5, K11), each followed by its one-slot merge, back to back.
// Every kernel behind the sweeps runs on a FLAT grid with a prefix table in device memory (table_slot_of): blockIdx.y
// cannot count slots of different sizes.  Chunks (pairs_plan.h): consecutive pairs whose partials, lists and per-row arrays
// fit the option "coll_ws_bytes" (0 = 2^30), at least one pair, enqueued back to back; a running total in device memory makes
// the offsets global.  The tables of ALL chunks are built on the host before anything is enqueued and go up in one copy.
struct PairsMergeSlot {
    const unsigned long long* partial;    // [nsplit][ncols_alloc][2] keys of the slot's sweep
    unsigned* fix;                        // tie list (fix[0] = count, rows from fix[4]) or null
    int64_t out;                          // first entry of the slot's lists
    int nsplit, ncols_alloc, nrows, pad_;
};
struct PairsJoinSlot {
    int64_t fwd, rev;                     // first list entry of the forward (rows of a) and reverse (rows of b) lists
    int64_t e0;                           // first entry of the pair in the per-row arrays of the chunk
    int32_t nq, nt;                       // rows of a (0: the pair accepts nothing and owns no block), rows of b
};

// coll_merge2_kernel for a chunk's slots: block b belongs to slot table_slot_of(blk0, n, b), rows from (b - blk0[slot]) * 256.
// kF32Keys false, the integer route: keys (d2 << 32 | row), the distance is the float32 root and the rows whose float32
// order can differ from the d2 order go on the slot's tie list (see knn2_merge_kernel).  kF32Keys true, a wide chunk
// (wide_f32.hip, part 4): keys (float32 distance bits << 32 | row inside the reduced image), one split, no tie list -- the
// key order IS the (distance, row) order.
template <bool kF32Keys>
__global__ __launch_bounds__(256)
void coll_pairs_merge_kernel(const PairsMergeSlot* __restrict__ slots, const int* __restrict__ blk0, int n,
                             int32_t* __restrict__ idx, float* __restrict__ dist)
{
    const int s = table_slot_of(blk0, n, (int)blockIdx.x);
    const PairsMergeSlot sl = slots[s];
    const int64_t i = (int64_t)((int)blockIdx.x - blk0[s]) * 256 + threadIdx.x;
    if (i >= sl.nrows) return;
    unsigned long long b0 = ~0ull, b1 = ~0ull;
    for (int sp = 0; sp < sl.nsplit; ++sp) {
        const unsigned long long* p = sl.partial + ((size_t)sp * sl.ncols_alloc + i) * 2;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const unsigned long long v = p[k];
            if (v < b0) { b1 = b0; b0 = v; }
            else if (v < b1) { b1 = v; }
        }
    }
    const int64_t o = 2 * (sl.out + i);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const unsigned long long b = k ? b1 : b0;
        idx[o + k] = (b == ~0ull) ? -1 : (int32_t)(unsigned)b;
        if constexpr (kF32Keys) dist[o + k] = (b == ~0ull) ? INFINITY : __uint_as_float((unsigned)(b >> 32));
        else dist[o + k] = (b == ~0ull) ? INFINITY : sqrtf((float)(unsigned)(b >> 32));
    }
    if constexpr (!kF32Keys) {
        if (sl.fix && b1 != ~0ull && (unsigned)(b1 >> 32) >= kSqrtTieMin) {
            const unsigned e0 = (unsigned)(b0 >> 32), e1 = (unsigned)(b1 >> 32);
            const bool paired1 = sqrt_ties_up(e1) || sqrt_ties_up(e1 - 1u);
            const bool paired0 = e0 >= kSqrtTieMin && (sqrt_ties_up(e0) || sqrt_ties_up(e0 - 1u));
            if (paired0 || paired1) sl.fix[4 + atomicAdd(sl.fix, 1u)] = (unsigned)i;
        }
    }
}

// The join of a chunk's pairs: lowe_each_kernel's forward test and mutual_join_kernel's two rules, word for word, with the
// reverse list of the first neighbour looked up in place.  Block b: pair table_slot_of(pblk0, n, b), rows of a from
// (b - pblk0[pair]) * 256.
__global__ __launch_bounds__(256)
void coll_pairs_join_kernel(const PairsJoinSlot* __restrict__ ps, const int* __restrict__ pblk0, int n,
                            const int32_t* __restrict__ l_idx, const float* __restrict__ l_dist, double tau, int symmetric,
                            int32_t* __restrict__ tidx, float* __restrict__ dist, double* __restrict__ ratio,
                            uint8_t* __restrict__ pass, int* __restrict__ block_counts)
{
    const int j = table_slot_of(pblk0, n, (int)blockIdx.x);
    const PairsJoinSlot s = ps[j];
    const int64_t q = (int64_t)((int)blockIdx.x - pblk0[j]) * 256 + threadIdx.x;
    bool keep = false;
    if (q < s.nq) {
        const int64_t f = 2 * (s.fwd + q);
        const int32_t t0 = l_idx[f];
        const float d1 = l_dist[f], d2 = l_dist[f + 1];
        double r = (l_idx[f + 1] >= 0) ? (double)d1 / (double)d2 : NAN;
        if (r < tau) {
            const int64_t g = 2 * (s.rev + t0);
            keep = l_idx[g] == (int32_t)q;             // mutual: the train row's nearest query row (lowest index on ties)
            if (keep && symmetric) {
                const double rr = (l_idx[g + 1] >= 0) ? (double)l_dist[g] / (double)l_dist[g + 1] : NAN;
                keep = rr < tau;
                if (keep && rr > r) r = rr;
            }
        }
        const int64_t e = s.e0 + q;
        tidx[e] = t0;
        dist[e] = d1;
        ratio[e] = r;
        pass[e] = keep ? 1 : 0;
    }
    emit_block_count(__ballot(keep), block_counts);
}

// One workgroup: the exclusive prefix of a chunk's block counts on top of the running total of the chunks before it
// (block_base, global ranks), the chunk's pair offsets -- offsets points at the chunk's first pair; a pair's offset is the
// base of its first block, the end for a pair without blocks behind the last one -- and the new running total.  No atomics:
// the result does not depend on any order of execution.
__global__ __launch_bounds__(256)
void coll_pairs_scan_kernel(const int* __restrict__ block_counts, int nblocks, const int* __restrict__ pblk0, int npairs,
                            long long* carry, long long* block_base, long long* offsets)
{
    __shared__ int sc[256];
    __shared__ long long run;
    const int tid = threadIdx.x;
    if (tid == 0) run = *carry;
    __syncthreads();
    for (int b0 = 0; b0 < nblocks; b0 += 256) {
        const int b = b0 + tid;
        const int v = b < nblocks ? block_counts[b] : 0;
        sc[tid] = v;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {
            const int t = tid >= d ? sc[tid - d] : 0;
            __syncthreads();
            sc[tid] += t;
            __syncthreads();
        }
        const long long base = run;
        if (b < nblocks) block_base[b] = base + sc[tid] - v;
        __syncthreads();
        if (tid == 255) run = base + sc[255];
        __syncthreads();
    }
    const long long end = run;
    for (int j = tid; j <= npairs; j += 256) {
        const int fb = j < npairs ? pblk0[j] : nblocks;
        offsets[j] = fb < nblocks ? block_base[fb] : end;
    }
    if (tid == 0) *carry = end;
}

// Ordered compaction of a chunk's accepted rows at their global ranks: the rows of a pair are written iff the pair ends
// within cap (the longest prefix of whole pairs: the offsets ascend).  Four columns (o_rows null) or 12-byte rows.
__global__ __launch_bounds__(256)
void coll_pairs_compact_kernel(const PairsJoinSlot* __restrict__ ps, const int* __restrict__ pblk0, int n,
                               const int32_t* __restrict__ tidx, const float* __restrict__ dist, const double* __restrict__ ratio,
                               const uint8_t* __restrict__ pass, const long long* __restrict__ block_base,
                               const long long* __restrict__ offsets, int64_t cap, int32_t* __restrict__ o_q,
                               int32_t* __restrict__ o_t, float* __restrict__ o_d, double* __restrict__ o_r, int32_t* __restrict__ o_rows)
{
    __shared__ int wave_cnt[4];
    const int j = table_slot_of(pblk0, n, (int)blockIdx.x);
    const PairsJoinSlot s = ps[j];
    const int64_t q = (int64_t)((int)blockIdx.x - pblk0[j]) * 256 + threadIdx.x;
    const bool p = q < s.nq && pass[s.e0 + q];
    const unsigned long long m = __ballot(p);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) wave_cnt[wave] = __popcll(m);
    __syncthreads();
    int wb = 0;
    for (int w = 0; w < wave; ++w) wb += wave_cnt[w];
    if (!p || offsets[j + 1] > cap) return;
    const int64_t dst = block_base[blockIdx.x] + wb + __popcll(m & ((1ull << lane) - 1ull));
    const int64_t e = s.e0 + q;
    if (o_rows) {
        o_rows[3 * dst] = (int32_t)q;
        o_rows[3 * dst + 1] = tidx[e];
        o_rows[3 * dst + 2] = (int32_t)__float_as_uint(dist[e]);
    } else {
        o_q[dst] = (int32_t)q; o_t[dst] = tidx[e]; o_d[dst] = dist[e]; o_r[dst] = ratio[e];
    }
}

struct CollPairsArgs {
    const char* who;
    double tau; int symmetric; int64_t cap;
    int64_t* offsets; int32_t* qidx; int32_t* tidx; float* dist; double* ratio;     // host form
    bool to_dev; int64_t* d_offsets; int32_t* d_rows; void* consumer;               // device form
    int64_t* n_total;
    // fm_collection_wide_*_each: "pair" p is (q, image p) -- a is the wide query bank, outside the stack -- for every image;
    // knn2: the forward slots alone, their merged lists [n_images][nq][2] copied to k_idx / k_dist (host), no join
    const fm::Bank* q = nullptr; bool knn2 = false; int32_t* k_idx = nullptr; float* k_dist = nullptr;
    // knn2 with k_votes (fm_collection_wide_votes, mode 1): the lists stay on the device; tau's ratio test on every list,
    // counted per image into k_votes [n_images] (host)
    int64_t* k_votes = nullptr;
};

// One chunk of consecutive pairs [p0, p1): what its kernels cover (PairsSpan) and where its tables lie in the call's table image.
struct PairsChunk : PairsSpan {
    size_t o_rr = 0, o_ms = 0, o_mb = 0, o_js = 0, o_jb = 0;     // batched-sweep table | merge slots | their first blocks | join slots | theirs
    // wide collections: the route, the record list's size, the filter's grid, and the slot table | first workgroups | first rows
    bool filt = false; unsigned cap = 0; int fwg = 0;
    size_t o_ws = 0, o_ww = 0, o_wr = 0;
};

// Integer route: a slot under the plan of its own sizes with the bytes it takes of the chunk's workspace, and a slot whose
// merge may list rows for the float32-root repair.
struct PairsSlotPlan { RowReducePlan pl; size_t part, bound, fix; };
struct PairsFixJob { size_t chunk; unsigned* fix; int ia, ib; int64_t out; };

// One call of the match graph: what the phases below hand to each other.
struct PairsCall {
    fm_ctx* ctx; fm_collection* c; const CollPairsArgs& a; const std::string who;
    const int32_t* pairs; int64_t n_pairs;          // the pairs in order (null with a.q: pair p is (q, image p))
    std::vector<int32_t> all;                       // ... spelled out when the caller passed NULL for every i < j
    const int64_t ni; const bool qm; const int64_t nq;      // images; the query bank is a.q, outside the stack, of nq rows
    const int ndir;                                 // sweeps per live pair (knn2: the forward one alone)
    // the route: the integer table launch, the wide filter + exact table launch, or (neither) sweep_pair pair by pair
    bool i8 = false, wide = false, wide_filter_on = false;
    Tuning shaped;                                  // the integer route's plans: the batched shape
    size_t budget = 0;                              // bytes of a chunk ("coll_ws_bytes")
    std::vector<PairsChunk> chunks;
    // the largest chunk's needs, and all chunks' tables and per-row entries
    size_t tab_bytes = 0, max_part = 0, max_bound = 0, max_fix = 0, max_cap = 0;
    int64_t max_lists = 0, max_entries = 0, max_jblocks = 0, sum_entries = 0;
    // ws_partial of one chunk.  Integer route: partials | bounds (p_bound) | tie lists (p_fix).  Wide: partial [rows][2] | count
    // (w_cnt) | bounds [rows] (w_bound) | records (w_list) | their scores (w_score).
    size_t p_bound = 0, p_fix = 0, w_cnt = 0, w_bound = 0, w_list = 0, w_score = 0;
    // ws_out: offsets | carry | lists | per-row arrays | block arrays | packed columns (host form: ccap rows)
    int64_t ccap = 0;
    size_t o_off = 0, o_carry = 0, o_li = 0, o_ld = 0, o_tidx = 0, o_dist = 0, o_ratio = 0, o_pass = 0, o_bc = 0, o_bb = 0;
    size_t o_cq = 0, o_ct = 0, o_cd = 0, o_cr = 0;
    char* b = nullptr; char* wp = nullptr;          // ws_out, ws_partial
    char* h = nullptr; const char* d = nullptr;     // the table image on the host (h_tab) and on the device (ws_in)
    long long* d_off = nullptr; long long* d_carry = nullptr;
    int32_t* l_idx = nullptr; float* l_dist = nullptr;      // the merged lists
    std::vector<PairsFixJob> fixes; size_t next_fix = 0;    // in slot order; the first of the next chunk
    bool timed = false;                             // ev_k0 is recorded

    PairsCall(fm_ctx* ctx_, fm_collection* c_, const int32_t* pairs_, int64_t n_pairs_, const CollPairsArgs& a_)
        : ctx(ctx_), c(c_), a(a_), who(a_.who), pairs(pairs_), n_pairs(n_pairs_), ni((int64_t)c_->rows.size()), qm(a_.q != nullptr),
          nq(a_.q ? a_.q->n : 0), ndir(a_.knn2 ? 1 : 2) {}
    // rows of the pair's two sides: a = the output rows of its forward slot, b = of its reverse slot
    int64_t rows_a(int64_t p) const { return qm ? nq : c->rows[(size_t)pairs[2 * p]]; }
    int64_t rows_b(int64_t p) const { return qm ? c->rows[(size_t)p] : c->rows[(size_t)pairs[2 * p + 1]]; }
    bool live(int64_t p) const { return rows_a(p) > 0 && rows_b(p) > 0; }
    PairsSlotPlan slot_plan(int ia, int ib) const      // integer route: output rows = image ia, reduced = image ib
    {
        PairsSlotPlan s;
        const fm::Bank va = coll_view(c, ia), vb = coll_view(c, ib);
        s.pl = plan_rowreduce(va.n_pad, vb.n_pad, shaped);
        s.part = align256(s.pl.partial_bytes(2));
        s.bound = (ctx->tune.coop != 0 && s.pl.nsplit > 1) ? align256(s.pl.bound_bytes()) : 0;
        s.fix = sqrt_tie_possible(va, vb) ? align256(fix_bytes(va.n)) : 0;
        return s;
    }
};

// Phase 1: the arguments and the empty cases, in the header's order of refusals.  *done: the call is complete (FM_OK).
// (With a.q the caller has checked q and passes pairs = NULL, n_pairs = n_images.)
static int pairs_check(fm_ctx* ctx, fm_collection* c, const int32_t* pairs, int64_t n_pairs, const CollPairsArgs& a, bool* done)
{
    const std::string who(a.who);
    int rc = coll_check(ctx, c, a.who);
    if (rc != FM_OK) return rc;
    const int64_t ni = (int64_t)c->rows.size(), cap = a.cap;
    const bool qm = a.q != nullptr;
    const int64_t nq = qm ? a.q->n : 0;
    if (n_pairs < 0) return fail(ctx, FM_EINVAL, who + ": n_pairs < 0");
    if (!qm && !pairs && n_pairs != ni * (ni - 1) / 2)
        return fail(ctx, FM_EINVAL, who + ": pairs is NULL (every i < j) and n_pairs is not n_images (n_images - 1) / 2");
    if (n_pairs > 0x7fffffff) return fail(ctx, FM_EUNSUPPORTED, who + ": n_pairs exceeds 2^31 - 1");
    for (int64_t p = 0; pairs && p < n_pairs; ++p)
        if (pairs[2 * p] < 0 || pairs[2 * p] >= ni || pairs[2 * p + 1] < 0 || pairs[2 * p + 1] >= ni)
            return fail(ctx, FM_EINVAL, who + ": pair " + std::to_string(p) + " names an image outside [0, n_images)");
    if (cap < 0) return fail(ctx, FM_EINVAL, who + ": cap is negative");
    *done = true;
    if (a.knn2) {
        if (!a.k_votes && ni * nq > 0 && (!a.k_idx || !a.k_dist)) return fail(ctx, FM_EINVAL, who + ": idx / dist is NULL");
        if (ni * nq == 0) return FM_OK;
    } else if (a.to_dev) {
        if (!a.d_offsets) return fail(ctx, FM_EINVAL, who + ": d_offsets is NULL");
        if (cap > 0 && !a.d_rows) return fail(ctx, FM_EINVAL, who + ": d_rows is NULL with cap > 0");
    } else {
        if (!a.offsets) return fail(ctx, FM_EINVAL, who + ": offsets is NULL");
        if (cap > 0 && (!a.qidx || !a.tidx || !a.dist || !a.ratio)) return fail(ctx, FM_EINVAL, who + ": qidx / tidx / dist / ratio is NULL with cap > 0");
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (a.to_dev) {
        if ((rc = check_device_ptr(ctx, a.d_offsets, a.who, "d_offsets")) != FM_OK) return rc;
        if (cap > 0 && (rc = check_device_ptr(ctx, a.d_rows, a.who, "d_rows")) != FM_OK) return rc;
    }
    if (a.n_total) *a.n_total = 0;
    if (n_pairs == 0) {
        if (a.to_dev) {
            if ((rc = wait_for_stream(ctx, a.consumer)) != FM_OK) return rc;
            HIP_TRY(ctx, hipMemsetAsync(a.d_offsets, 0, 8, ctx->stream));
            return results_written(ctx, a.consumer);
        }
        a.offsets[0] = 0;
        return FM_OK;
    }
    *done = false;
    return FM_OK;
}

// The pair list (NULL: every i < j, lexicographic), the route, the integer route's shape and the budget.
static int pairs_resolve(PairsCall& k)
{
    fm_ctx* ctx = k.ctx;
    const fm_collection* c = k.c;
    try {
        if (!k.pairs && !k.qm) {
            k.all.reserve((size_t)k.n_pairs * 2);
            for (int32_t i = 0; i < (int32_t)k.ni; ++i) for (int32_t j = i + 1; j < (int32_t)k.ni; ++j) { k.all.push_back(i); k.all.push_back(j); }
            k.pairs = k.all.data();
        }
    } catch (const std::bad_alloc&) { return fail(ctx, FM_ENOMEM, k.who + ": out of host memory"); }
    k.wide = coll_is_wide(c);
    k.i8 = c->stack.kind == FM_BANK_I8 && !k.wide;
    // Wide collections (wide_f32.hip, part 4): a chunk's slots lie side by side in one output-row space, swept by ONE filter
    // launch + ONE rescoring + ONE guarded exact launch (or the exact launch alone) and merged by one launch, whatever the
    // number of pairs.
    k.wide_filter_on = k.wide && ctx->tune.f32_filter != 0 && ctx->d_counters && c->stack.filt_ok && c->stack.wrowsh &&
                       (!k.qm || wide_filter_usable(*k.a.q, c->stack));
    // Plans of the integer route: the batched shape, every slot under the plan of its own sizes.  Splits exist to fill the
    // chip from ONE pair; a call whose slots fill it without them takes one split per slot (no shared bounds, the smallest
    // partials).
    k.shaped = ctx->tune;
    k.shaped.nb = 4; k.shaped.nw = 8; k.shaped.nbuf = 0; k.shaped.nsplit = 0; k.shaped.k1_order = 0;
    if (k.i8) {
        int64_t wg1 = 0;
        for (int64_t p = 0; p < k.n_pairs && wg1 < 2048; ++p)
            if (k.live(p)) wg1 += (pad128(c->rows[(size_t)k.pairs[2 * p]]) + 511) / 512 + (pad128(c->rows[(size_t)k.pairs[2 * p + 1]]) + 511) / 512;
        if (wg1 >= 2048) k.shaped.nsplit = 1;
    }
    k.budget = (size_t)ctx->tune.coll_ws_bytes;
    if (k.budget == 0) k.budget = (size_t)1 << 30;
    return FM_OK;
}

// Phase 2: what pair p takes of a chunk, one function per route.  A pair with an empty side: nothing.
static PairsCost pairs_cost_i8(const PairsCall& k, int64_t p)
{
    PairsCost n;
    if (!k.live(p)) return n;
    n.ra = k.rows_a(p); n.rb = k.rows_b(p);
    const int ia = k.pairs[2 * p], ib = k.pairs[2 * p + 1];
    const PairsSlotPlan f = k.slot_plan(ia, ib), r = k.slot_plan(ib, ia);
    n.part = f.part + r.part; n.bound = f.bound + r.bound; n.fix = f.fix + r.fix;
    n.wg = (int64_t)rowreduce_grid(f.pl) + rowreduce_grid(r.pl);
    n.mblocks = (n.ra + 255) / 256 + (n.rb + 255) / 256;
    n.jblocks = (n.ra + 255) / 256;
    return n;
}

static PairsCost pairs_cost_wide(const PairsCall& k, int64_t p)
{
    PairsCost n;
    if (!k.live(p)) return n;
    n.ra = k.rows_a(p); n.rb = k.rows_b(p);
    const int64_t rr = k.a.knn2 ? 0 : n.rb;             // output rows of the reverse slot
    const int64_t pr = pad128(n.ra) + (rr ? pad128(rr) : 0);
    // partial [rows][2], bounds [rows], and 256 records of 12 bytes per output row where the filter may run
    n.part = (size_t)pr * 16; n.bound = (size_t)pr * 4; n.fix = k.wide_filter_on ? (size_t)(n.ra + rr) * 256 * 12 : 0;
    n.wg = pr / kStageRows;
    n.wrows = pr;
    n.mblocks = (n.ra + 255) / 256 + (rr + 255) / 256;
    n.jblocks = k.a.knn2 ? 0 : (n.ra + 255) / 256;
    return n;
}

static PairsCost pairs_cost_pairwise(const PairsCall& k, int64_t p)
{
    PairsCost n;
    if (!k.live(p)) return n;
    n.ra = k.rows_a(p); n.rb = k.rows_b(p);             // (sweep_pair sizes its own partials, pair by pair)
    n.jblocks = (n.ra + 255) / 256;
    return n;
}

// A planned chunk's tables in the call's table image (carve), and its share of the call's maxima.
static void pairs_chunk_tables(PairsCall& k, PairsChunk& ch)
{
    const int np = (int)(ch.p1 - ch.p0);
    if (k.i8 && ch.nslots > 0) {
        ch.o_rr = carve(k.tab_bytes, rowreduce_table_bytes(ch.nslots));
        ch.o_ms = carve(k.tab_bytes, (size_t)ch.nslots * sizeof(PairsMergeSlot));
        ch.o_mb = carve(k.tab_bytes, ((size_t)ch.nslots + 1) * 4);
    }
    if (k.wide && ch.nslots > 0) {
        ch.o_ws = carve(k.tab_bytes, (size_t)ch.nslots * sizeof(WideSlot));
        ch.o_ww = carve(k.tab_bytes, ((size_t)ch.nslots + 1) * 4);
        ch.o_wr = carve(k.tab_bytes, ((size_t)ch.nslots + 1) * 4);
        ch.o_ms = carve(k.tab_bytes, (size_t)ch.nslots * sizeof(PairsMergeSlot));
        ch.o_mb = carve(k.tab_bytes, ((size_t)ch.nslots + 1) * 4);
        // wide_route's rule on the chunk's work; the list: 256 records per output row, plan_wide_filter's figure
        ch.filt = k.wide_filter_on && (k.ctx->tune.f32_filter >= 2 || ch.work >= 4.0e6);
        if (ch.filt) {
            ch.cap = (unsigned)std::min<int64_t>(std::max<int64_t>(256 * ch.lists, 1 << 20), (int64_t)1 << 28);
            k.max_cap = std::max<size_t>(k.max_cap, ch.cap);
        }
    }
    ch.o_js = carve(k.tab_bytes, (size_t)np * sizeof(PairsJoinSlot));
    ch.o_jb = carve(k.tab_bytes, ((size_t)np + 1) * 4);
    k.max_part = std::max(k.max_part, ch.part); k.max_bound = std::max(k.max_bound, ch.bound); k.max_fix = std::max(k.max_fix, ch.fix);
    k.max_lists = std::max(k.max_lists, ch.lists); k.max_entries = std::max(k.max_entries, ch.entries);
    k.max_jblocks = std::max(k.max_jblocks, ch.jblocks);
    k.sum_entries += ch.entries;
}

// Phase 3: the chunks (pairs_plan.h) of the pairs' costs.
static int pairs_chunks(PairsCall& k)
{
    try {
        std::vector<PairsCost> cost((size_t)k.n_pairs);
        for (int64_t p = 0; p < k.n_pairs; ++p)
            cost[(size_t)p] = k.i8 ? pairs_cost_i8(k, p) : k.wide ? pairs_cost_wide(k, p) : pairs_cost_pairwise(k, p);
        std::vector<PairsSpan> spans;
        int64_t bad = 0;
        switch (pairs_plan(cost.data(), k.n_pairs, k.budget, k.ndir, &spans, &bad)) {
        case kPairsPlanWorkgroups: return fail(k.ctx, FM_EUNSUPPORTED, k.who + ": one pair needs more than 2^31 - 1 workgroups");
        case kPairsPlanWideRows: return fail(k.ctx, FM_EUNSUPPORTED, k.who + ": one pair of a wide collection has more than 2^30 rows");
        case kPairsPlanOk: break;
        }
        k.chunks.reserve(spans.size());
        for (const PairsSpan& s : spans) {
            PairsChunk ch;
            static_cast<PairsSpan&>(ch) = s;
            pairs_chunk_tables(k, ch);
            k.chunks.push_back(ch);
        }
    } catch (const std::bad_alloc&) { return fail(k.ctx, FM_ENOMEM, k.who + ": out of host memory"); }
    return FM_OK;
}

// Phase 4: the workspaces, all before anything is enqueued: ws_out (the layout in PairsCall), ws_partial for the largest chunk
// (the integer and the wide route; sweep_pair sizes its own), ws_in and its page-locked host image for the tables.
static int pairs_carve(PairsCall& k)
{
    fm_ctx* ctx = k.ctx;
    int rc;
    k.ccap = k.a.to_dev ? 0 : std::min<int64_t>(k.a.cap, k.sum_entries);
    if (k.a.knn2) k.max_lists = k.ni * k.nq;       // the lists ARE the result: every image's, [n_images][nq][2]
    size_t off = 0;
    k.o_off = carve(off, ((size_t)k.n_pairs + 1) * 8); k.o_carry = carve(off, 16);
    k.o_li = carve(off, (size_t)k.max_lists * 8); k.o_ld = carve(off, (size_t)k.max_lists * 8);
    k.o_tidx = carve(off, (size_t)k.max_entries * 4); k.o_dist = carve(off, (size_t)k.max_entries * 4); k.o_ratio = carve(off, (size_t)k.max_entries * 8);
    k.o_pass = carve(off, (size_t)k.max_entries); k.o_bc = carve(off, (size_t)k.max_jblocks * 4); k.o_bb = carve(off, (size_t)k.max_jblocks * 8);
    k.o_cq = carve(off, (size_t)k.ccap * 4); k.o_ct = carve(off, (size_t)k.ccap * 4); k.o_cd = carve(off, (size_t)k.ccap * 4); k.o_cr = carve(off, (size_t)k.ccap * 8);
    if ((rc = ws_ensure(ctx, &ctx->ws_out, &ctx->ws_out_bytes, off + 64)) != FM_OK) return rc;
    // (every slot's partials, bounds and tie lists are multiples of 256 bytes: so are the sums)
    k.p_bound = k.max_part; k.p_fix = k.p_bound + k.max_bound;
    if (k.i8 && k.max_part > 0 && (rc = ws_ensure(ctx, &ctx->ws_partial, &ctx->ws_partial_bytes, k.p_fix + k.max_fix + 64)) != FM_OK) return rc;
    k.w_cnt = align256(k.max_part); k.w_bound = k.w_cnt + 256; k.w_list = k.w_bound + align256(k.max_bound); k.w_score = k.w_list + align256(k.max_cap * 8);
    if (k.wide && k.max_part > 0 && (rc = ws_ensure(ctx, &ctx->ws_partial, &ctx->ws_partial_bytes, k.w_score + align256(k.max_cap * 4) + 64)) != FM_OK) return rc;
    if ((rc = ws_ensure(ctx, &ctx->ws_in, &ctx->ws_in_bytes, k.tab_bytes + 64)) != FM_OK) return rc;
    if ((rc = table_host(ctx, k.tab_bytes)) != FM_OK) return rc;
    k.b = (char*)ctx->ws_out;
    k.h = ctx->h_tab;
    k.d = (const char*)ctx->ws_in;
    k.wp = (char*)ctx->ws_partial;
    k.d_off = k.a.to_dev ? (long long*)k.a.d_offsets : (long long*)(k.b + k.o_off);
    k.d_carry = (long long*)(k.b + k.o_carry);
    k.l_idx = (int32_t*)(k.b + k.o_li); k.l_dist = (float*)(k.b + k.o_ld);
    return FM_OK;
}

// Phase 5: the tables, now that every address is known.  Where a chunk's tables stand: the next slot, its first workgroup
// and merge block, the next pair's first join block, list entry and per-row entry.
struct PairsCursor {
    int slot = 0, wg = 0, mb = 0, jb = 0;
    int64_t list = 0, entry = 0;
};

// The join slot of pair p at the cursor, which moves behind the pair's lists, entries and join blocks.  False: a side of the
// pair is empty -- a zero slot without blocks, and no sweeps.
static bool pairs_join_slot(const PairsCall& k, int64_t p, PairsJoinSlot* s, PairsCursor* at)
{
    *s = PairsJoinSlot{};
    if (!k.live(p)) return false;
    const int64_t ra = k.rows_a(p), rb = k.rows_b(p);
    s->fwd = k.a.knn2 ? p * k.nq : at->list; s->rev = at->list + ra; s->e0 = at->entry; s->nq = (int32_t)ra; s->nt = (int32_t)rb;
    if (k.a.knn2) return true;                     // (the forward lists are the result, image by image: nothing to join)
    at->list += ra + rb; at->entry += ra; at->jb += (int)((ra + 255) / 256);
    return true;
}

// The pairwise route has the join's tables alone.
static int pairs_tables_join(PairsCall& k, size_t kc)
{
    const PairsChunk& ch = k.chunks[kc];
    PairsJoinSlot* js = (PairsJoinSlot*)(k.h + ch.o_js);
    int* jb0 = (int*)(k.h + ch.o_jb);
    PairsCursor at;
    for (int64_t p = ch.p0; p < ch.p1; ++p) { jb0[p - ch.p0] = at.jb; (void)pairs_join_slot(k, p, &js[p - ch.p0], &at); }
    jb0[ch.p1 - ch.p0] = at.jb;
    return FM_OK;
}

static int pairs_tables_i8(PairsCall& k, size_t kc)
{
    const PairsChunk& ch = k.chunks[kc];
    const fm_collection* c = k.c;
    const int np = (int)(ch.p1 - ch.p0);
    PairsMergeSlot* ms = (PairsMergeSlot*)(k.h + ch.o_ms);
    int* mb0 = (int*)(k.h + ch.o_mb);
    PairsJoinSlot* js = (PairsJoinSlot*)(k.h + ch.o_js);
    int* jb0 = (int*)(k.h + ch.o_jb);
    PairsCursor at;
    size_t at_p = 0, at_b = k.p_bound, at_f = k.p_fix;
    for (int j = 0; j < np; ++j) {
        const int64_t p = ch.p0 + j;
        PairsJoinSlot& s = js[j];
        jb0[j] = at.jb;
        if (!pairs_join_slot(k, p, &s, &at)) continue;
        const int ia = k.pairs[2 * p], ib = k.pairs[2 * p + 1];
        for (int dir = 0; dir < 2; ++dir) {
            const int io = dir ? ib : ia, ir = dir ? ia : ib;
            const fm::Bank vo = coll_view(c, io), vr = coll_view(c, ir);
            const PairsSlotPlan sp = k.slot_plan(io, ir);
            unsigned long long* part = (unsigned long long*)(k.wp + at_p);
            int* bound = sp.bound ? (int*)(k.wp + at_b) : nullptr;
            unsigned* fix = sp.fix ? (unsigned*)(k.wp + at_f) : nullptr;
            at_p += sp.part; at_b += sp.bound; at_f += sp.fix;
            const int g = rowreduce_table_set(k.h + ch.o_rr, ch.nslots, at.slot, at.wg, vo, vr, sp.pl, part, bound);
            if (g < 1) return fail(k.ctx, FM_EDEVICE, k.who + ": internal: a slot's plan is not in the batched shape");
            PairsMergeSlot& m = ms[at.slot];
            m.partial = part; m.fix = fix; m.out = dir ? s.rev : s.fwd;
            m.nsplit = sp.pl.nsplit; m.ncols_alloc = sp.pl.ncols_alloc; m.nrows = (int)vo.n; m.pad_ = 0;
            mb0[at.slot] = at.mb;
            if (fix) k.fixes.push_back(PairsFixJob{kc, fix, io, ir, m.out});
            at.wg += g; at.mb += (int)((vo.n + 255) / 256);
            ++at.slot;
        }
    }
    jb0[np] = at.jb;
    if (ch.nslots > 0) { rowreduce_table_end(k.h + ch.o_rr, ch.nslots, at.wg); mb0[ch.nslots] = at.mb; }
    return FM_OK;
}

static int pairs_tables_wide(PairsCall& k, size_t kc)
{
    PairsChunk& ch = k.chunks[kc];
    fm_ctx* ctx = k.ctx;
    const fm_collection* c = k.c;
    const CollPairsArgs& a = k.a;
    const bool qm = k.qm;
    const int np = (int)(ch.p1 - ch.p0);
    WideSlot* wsl = (WideSlot*)(k.h + ch.o_ws);
    int* ww0 = (int*)(k.h + ch.o_ww);
    int* wr0 = (int*)(k.h + ch.o_wr);
    int wrow = 0;
    // a chunk whose slots fill the chip without splits takes one split per slot
    const bool one_split = ch.wg >= 512 && ctx->tune.f32_nsplit == 0;
    PairsMergeSlot* ms = (PairsMergeSlot*)(k.h + ch.o_ms);
    int* mb0 = (int*)(k.h + ch.o_mb);
    PairsJoinSlot* js = (PairsJoinSlot*)(k.h + ch.o_js);
    int* jb0 = (int*)(k.h + ch.o_jb);
    PairsCursor at;
    for (int j = 0; j < np; ++j) {
        const int64_t p = ch.p0 + j;
        PairsJoinSlot& s = js[j];
        jb0[j] = at.jb;
        if (!pairs_join_slot(k, p, &s, &at)) continue;
        const int ia = qm ? -1 : k.pairs[2 * p], ib = qm ? (int)p : k.pairs[2 * p + 1];
        const int64_t ra = k.rows_a(p), rb = k.rows_b(p);
        for (int dir = 0; dir < k.ndir; ++dir) {
            const int io = dir ? ib : ia, ir = dir ? ia : ib;           // (-1: the query bank, whose first row is 0)
            const int64_t no = dir ? rb : ra, nr = dir ? ra : rb;
            WideSlot& w = wsl[at.slot];
            w.col0 = io < 0 ? 0 : (int)c->phys[(size_t)io]; w.ncols = (int)no;
            w.red0 = ir < 0 ? 0 : (int)c->phys[(size_t)ir]; w.nred = (int)nr;
            // the slot's scale terms (launch_wide_filter's): the stack's scale is read here, at the call -- a later add may
            // lift it -- the query's was fixed at its creation
            const int dk = !qm ? 0 : dir ? a.q->kscale - c->stack.kscale : c->stack.kscale - a.q->kscale;      // kred - kcol
            w.outside = !qm ? 0 : dir ? kWideOutRed : kWideOutCols;
            w.cscale = ldexpf(1.f, dk); w.nscale = ldexpf(1.f, 2 * dk);
            w.red_nm_max = (qm && dir) ? a.q->nm_max : c->stack.nm_max;
            const WideFilterPlan fp = plan_wide_filter(pad128(no), no, pad128(nr), ctx->tune);
            w.ntiles = fp.ntiles;
            w.nsplit = one_split ? 1 : fp.nsplit;
            w.tiles_per_split = one_split ? fp.ntiles : fp.tiles_per_split;
            w.row0 = wrow;
            ww0[at.slot] = at.wg; wr0[at.slot] = wrow;
            PairsMergeSlot& m = ms[at.slot];
            m.partial = (unsigned long long*)k.wp + (size_t)wrow * 2; m.fix = nullptr; m.out = dir ? s.rev : s.fwd;
            m.nsplit = 1; m.ncols_alloc = (int)pad128(no); m.nrows = (int)no; m.pad_ = 0;
            mb0[at.slot] = at.mb;
            at.wg += fp.nchunks * w.nsplit; wrow += (int)pad128(no); at.mb += (int)((no + 255) / 256);
            ++at.slot;
        }
    }
    if (ch.nslots > 0) { ww0[ch.nslots] = at.wg; wr0[ch.nslots] = wrow; mb0[ch.nslots] = at.mb; ch.fwg = at.wg; }
    jb0[np] = at.jb;
    return FM_OK;
}

// The call's accounting, the tables' one copy up, the running total, and (knn2) the lists of the images without rows.
static int pairs_upload(PairsCall& k)
{
    fm_ctx* ctx = k.ctx;
    const fm_collection* c = k.c;
    for (int64_t p = 0; p < k.n_pairs; ++p) {
        if (!k.live(p)) continue;
        const int64_t ra = k.rows_a(p), rb = k.rows_b(p);
        ctx->pending_pairs += k.ndir * ra * rb;
        ctx->pending_bytes += k.ndir * (ra + rb) * (k.i8 ? 128 : k.wide ? 1024 : c->stack.kind == FM_BANK_BIN ? c->stack.dim : 512);
    }
    if (int rc = table_upload(ctx, ctx->ws_in, k.tab_bytes)) return rc;
    HIP_TRY(ctx, hipMemsetAsync(k.d_carry, 0, 16, ctx->stream));
    if (k.a.knn2) {
        // an image without rows keeps its slot: -1 / +inf, fm_knn2's lists over an empty bank
        bool any_empty = false;
        for (int64_t p = 0; p < k.n_pairs && !any_empty; ++p) any_empty = !k.live(p);
        if (any_empty) {
            HIP_TRY(ctx, hipMemsetAsync(k.l_idx, 0xff, (size_t)k.ni * k.nq * 8, ctx->stream));
            HIP_TRY(ctx, hipMemsetD32Async((hipDeviceptr_t)k.l_dist, 0x7f800000, (size_t)k.ni * k.nq * 2, ctx->stream));
        }
    }
    return FM_OK;
}

// Phase 6: one chunk's sweeps and merge.  Integer route: ONE table launch, ONE merge, the float32-root repair per listed slot.
static int pairs_enqueue_i8(PairsCall& k, size_t kc)
{
    const PairsChunk& ch = k.chunks[kc];
    fm_ctx* ctx = k.ctx;
    if (ch.bound) HIP_TRY(ctx, hipMemsetD32Async((hipDeviceptr_t)(k.wp + k.p_bound), (int)0x80000000, ch.bound / 4, ctx->stream));
    if (ch.fix) HIP_TRY(ctx, hipMemsetAsync(k.wp + k.p_fix, 0, ch.fix, ctx->stream));
    if (!k.timed) HIP_TRY(ctx, hipEventRecord(ctx->ev_k0, ctx->stream));
    k.timed = true;
    HIP_TRY(ctx, launch_rowreduce_table2(k.d + ch.o_rr, ch.nslots, (int)ch.wg, ctx->stream));
    hipLaunchKernelGGL(coll_pairs_merge_kernel<false>, dim3((unsigned)ch.mblocks), dim3(256), 0, ctx->stream,
                       (const PairsMergeSlot*)(k.d + ch.o_ms), (const int*)(k.d + ch.o_mb), ch.nslots, k.l_idx, k.l_dist);
    HIP_TRY(ctx, hipGetLastError());
    for (; k.next_fix < k.fixes.size() && k.fixes[k.next_fix].chunk == kc; ++k.next_fix) {
        const PairsFixJob& fj = k.fixes[k.next_fix];
        const fm::Bank vo = coll_view(k.c, fj.ia), vr = coll_view(k.c, fj.ib);
        HIP_TRY(ctx, launch_coll_sqrt_fix((const unsigned*)fj.fix, (const int8_t*)vo.rows8, (const int32_t*)vo.norm, (const int8_t*)vr.rows8,
                                          (const int32_t*)vr.norm, (int)vr.n, CollTab{nullptr, nullptr, nullptr}, fj.out, (int32_t*)nullptr,
                                          k.l_idx, k.l_dist, ctx->stream));
    }
    return FM_OK;
}

// Wide: the filter, its rescoring and the guarded exact launch over the chunk's output-row space (or the exact launch alone),
// then ONE merge.
static int pairs_enqueue_wide(PairsCall& k, size_t kc)
{
    const PairsChunk& ch = k.chunks[kc];
    fm_ctx* ctx = k.ctx;
    const fm::Bank& stack = k.c->stack;
    char* wp = k.wp;
    unsigned long long* part = (unsigned long long*)wp;
    const WideTableLaunch tl{(const WideSlot*)(k.d + ch.o_ws), (const int*)(k.d + ch.o_ww), (const int*)(k.d + ch.o_wr), ch.nslots, ch.fwg, ch.wrows, k.a.q};
    if (!k.timed) HIP_TRY(ctx, hipEventRecord(ctx->ev_k0, ctx->stream));
    k.timed = true;
    if (ch.filt) {
        HIP_TRY(ctx, hipMemsetAsync(part, 0xff, (size_t)ch.wrows * 16, ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(wp + k.w_cnt, 0, 256 + (size_t)ch.wrows * 4, ctx->stream));     // (the count and the bounds are neighbours)
        HIP_TRY(ctx, hipMemsetAsync(ctx->d_counters, 0, 8, ctx->stream));
        HIP_TRY(ctx, launch_wide_filter_table(stack, tl, ch.cap, (uint2*)(wp + k.w_list), (float*)(wp + k.w_score), (unsigned*)(wp + k.w_bound),
                                              (unsigned long long*)(wp + k.w_cnt), ctx->d_counters, part, ctx->stream));
        HIP_TRY(ctx, launch_wide_exact_table(stack, tl, part, ctx->d_counters, ctx->stream));
        ctx->filter_launches += 1;
    } else {
        HIP_TRY(ctx, launch_wide_exact_table(stack, tl, part, nullptr, ctx->stream));
    }
    hipLaunchKernelGGL(coll_pairs_merge_kernel<true>, dim3((unsigned)ch.mblocks), dim3(256), 0, ctx->stream,
                       (const PairsMergeSlot*)(k.d + ch.o_ms), (const int*)(k.d + ch.o_mb), ch.nslots, k.l_idx, k.l_dist);
    HIP_TRY(ctx, hipGetLastError());
    return FM_OK;
}

// Float32 route, binary: the pair's two sweeps by the existing route, each followed by its one-slot merge.
static int pairs_enqueue_pairwise(PairsCall& k, size_t kc)
{
    const PairsChunk& ch = k.chunks[kc];
    fm_ctx* ctx = k.ctx;
    const fm_collection* c = k.c;
    const int np = (int)(ch.p1 - ch.p0);
    const PairsJoinSlot* js = (const PairsJoinSlot*)(k.h + ch.o_js);
    int rc;
    if (!k.timed && c->stack.kind == FM_BANK_BIN) HIP_TRY(ctx, hipEventRecord(ctx->ev_k0, ctx->stream));
    k.timed = true;
    for (int j = 0; j < np; ++j) {
        const int64_t p = ch.p0 + j;
        if (!k.live(p)) continue;
        const fm::Bank va = coll_view(c, k.pairs[2 * p]), vb = coll_view(c, k.pairs[2 * p + 1]);
        const CollTab none{nullptr, nullptr, nullptr};
        PairSweep ps;
        if ((rc = sweep_pair(ctx, va, vb, 2, 0, nullptr, nullptr, kSweepNoEvents | kSweepNoCount, &ps)) != FM_OK) return rc;
        if ((rc = coll_merge_one(ctx, &ps, none, va.n, js[j].fwd, nullptr, k.l_idx, k.l_dist)) != FM_OK) return rc;
        if ((rc = sweep_pair(ctx, vb, va, 2, 0, nullptr, nullptr, kSweepNoEvents | kSweepNoCount, &ps)) != FM_OK) return rc;
        if ((rc = coll_merge_one(ctx, &ps, none, vb.n, js[j].rev, nullptr, k.l_idx, k.l_dist)) != FM_OK) return rc;
    }
    return FM_OK;
}

// Phase 7: the tail of a chunk: the join of its merged lists, the scan of its block counts on top of the running total, and
// the compaction of its accepted rows.
static int pairs_join_scan_compact(PairsCall& k, size_t kc)
{
    const PairsChunk& ch = k.chunks[kc];
    fm_ctx* ctx = k.ctx;
    const CollPairsArgs& a = k.a;
    const int np = (int)(ch.p1 - ch.p0);
    char* b = k.b;
    int rc;
    if (ch.jblocks > 0) {
        hipLaunchKernelGGL(coll_pairs_join_kernel, dim3((unsigned)ch.jblocks), dim3(256), 0, ctx->stream,
                           (const PairsJoinSlot*)(k.d + ch.o_js), (const int*)(k.d + ch.o_jb), np, (const int32_t*)k.l_idx, (const float*)k.l_dist,
                           a.tau, a.symmetric, (int32_t*)(b + k.o_tidx), (float*)(b + k.o_dist), (double*)(b + k.o_ratio),
                           (uint8_t*)(b + k.o_pass), (int*)(b + k.o_bc));
        HIP_TRY(ctx, hipGetLastError());
    }
    // (device form: the first scan is the first kernel that writes the caller's buffers)
    if (a.to_dev && kc == 0 && (rc = wait_for_stream(ctx, a.consumer)) != FM_OK) return rc;
    hipLaunchKernelGGL(coll_pairs_scan_kernel, dim3(1), dim3(256), 0, ctx->stream, (const int*)(b + k.o_bc), (int)ch.jblocks,
                       (const int*)(k.d + ch.o_jb), np, k.d_carry, (long long*)(b + k.o_bb), k.d_off + ch.p0);
    HIP_TRY(ctx, hipGetLastError());
    if (ch.jblocks > 0 && a.cap > 0) {
        hipLaunchKernelGGL(coll_pairs_compact_kernel, dim3((unsigned)ch.jblocks), dim3(256), 0, ctx->stream,
                           (const PairsJoinSlot*)(k.d + ch.o_js), (const int*)(k.d + ch.o_jb), np, (const int32_t*)(b + k.o_tidx),
                           (const float*)(b + k.o_dist), (const double*)(b + k.o_ratio), (const uint8_t*)(b + k.o_pass),
                           (const long long*)(b + k.o_bb), (const long long*)(k.d_off + ch.p0), a.cap, (int32_t*)(b + k.o_cq),
                           (int32_t*)(b + k.o_ct), (float*)(b + k.o_cd), (double*)(b + k.o_cr), a.to_dev ? a.d_rows : (int32_t*)nullptr);
        HIP_TRY(ctx, hipGetLastError());
    }
    return FM_OK;
}

// Phase 8: the result.  knn2: the merged forward lists of every image, as they are.
static int pairs_deliver_knn2(PairsCall& k, CallScope& cs)
{
    // (copies of up to 128 MB each)
    HIP_TRY(k.ctx, d2h_pieces(k.ctx, (size_t)k.ni * k.nq * 2, (size_t)32 << 20, {{k.a.k_idx, k.l_idx, 4}, {k.a.k_dist, k.l_dist, 4}}));
    return cs.finish();
}

// knn2 with k_votes: the ratio test on the merged lists where they lie, counted per image (coll_votes_kernel's per-image form).
// The counts take the offsets' place in ws_out ([n_images + 1] words that a knn2 call does not use).
static int pairs_deliver_votes(PairsCall& k, CallScope& cs)
{
    fm_ctx* ctx = k.ctx;
    unsigned long long* d_votes = (unsigned long long*)(k.b + k.o_off);
    HIP_TRY(ctx, hipMemsetAsync(d_votes, 0, (size_t)k.ni * 8, ctx->stream));
    HIP_TRY(ctx, launch_coll_votes(nullptr, k.l_idx, k.l_dist, k.nq, k.ni, k.a.tau, d_votes, ctx->stream));
    HIP_TRY(ctx, d2h(ctx, k.a.k_votes, d_votes, (size_t)k.ni * 8));
    return cs.finish();
}

// Device form: the rows and offsets are in the caller's memory behind "the results are written".
static int pairs_deliver_dev(PairsCall& k)
{
    fm_ctx* ctx = k.ctx;
    int rc;
    if ((rc = results_written(ctx, k.a.consumer)) != FM_OK) return rc;
    ctx->rows_stream = ctx->stream;
    if (!k.a.n_total) return FM_OK;            // (enqueued: nothing waits for the device)
    long long total = 0;                       // the caller asked for a host number: the call's one synchronisation
    HIP_TRY(ctx, hipMemcpyAsync(&total, k.d_carry, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *k.a.n_total = (int64_t)total;
    return FM_OK;
}

// Host form: the offsets decide how much is copied: they come down first, then the rows of the longest prefix of whole pairs.
static int pairs_deliver_host(PairsCall& k, CallScope& cs)
{
    fm_ctx* ctx = k.ctx;
    const CollPairsArgs& a = k.a;
    const int64_t n_pairs = k.n_pairs;
    char* b = k.b;
    std::vector<long long> ho;
    try { ho.resize((size_t)n_pairs + 1); } catch (const std::bad_alloc&) { return fail(ctx, FM_ENOMEM, k.who + ": out of host memory"); }
    HIP_TRY(ctx, hipMemcpyAsync(ho.data(), k.d_off, ((size_t)n_pairs + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    size_t m = 0;
    if (a.cap > 0) m = (size_t)*(std::upper_bound(ho.begin(), ho.end(), (long long)a.cap) - 1);
    HIP_TRY(ctx, d2h_pieces(ctx, m, (size_t)32 << 20, {{a.qidx, b + k.o_cq, 4}, {a.tidx, b + k.o_ct, 4}, {a.dist, b + k.o_cd, 4}, {a.ratio, b + k.o_cr, 8}}));
    const int rc = cs.finish();
    if (rc != FM_OK) return rc;
    for (int64_t p = 0; p <= n_pairs; ++p) a.offsets[p] = (int64_t)ho[(size_t)p];
    if (a.n_total) *a.n_total = (int64_t)ho[(size_t)n_pairs];
    return FM_OK;
}

static int coll_pairs_mutual(fm_ctx* ctx, fm_collection* c, const int32_t* pairs, int64_t n_pairs, const CollPairsArgs& a)
{
    bool done = false;
    int rc = pairs_check(ctx, c, pairs, n_pairs, a, &done);
    if (rc != FM_OK || done) return rc;
    PairsCall k(ctx, c, pairs, n_pairs, a);
    if ((rc = pairs_resolve(k)) != FM_OK) return rc;
    if ((rc = pairs_chunks(k)) != FM_OK) return rc;                     // pass 1
    if ((rc = pairs_carve(k)) != FM_OK) return rc;
    for (size_t kc = 0; kc < k.chunks.size(); ++kc) {                   // pass 2
        rc = k.i8 ? pairs_tables_i8(k, kc) : k.wide ? pairs_tables_wide(k, kc) : pairs_tables_join(k, kc);
        if (rc != FM_OK) return rc;
    }
    CallScope cs(ctx);
    if ((rc = pairs_upload(k)) != FM_OK) return rc;
    for (size_t kc = 0; kc < k.chunks.size(); ++kc) {
        if (k.chunks[kc].nslots > 0) {
            rc = k.i8 ? pairs_enqueue_i8(k, kc) : k.wide ? pairs_enqueue_wide(k, kc) : pairs_enqueue_pairwise(k, kc);
            if (rc != FM_OK) return rc;
        }
        if (a.knn2) continue;                      // (the merged forward lists are the result)
        if ((rc = pairs_join_scan_compact(k, kc)) != FM_OK) return rc;
    }
    if (k.timed) {
        if (c->stack.kind != FM_BANK_F32) HIP_TRY(ctx, hipEventRecord(ctx->ev_k1, ctx->stream));   // (the float32 route brackets its sweeps itself)
        ctx->kernel_timed = true;
    }
    if (a.knn2) return a.k_votes ? pairs_deliver_votes(k, cs) : pairs_deliver_knn2(k, cs);
    if (a.to_dev) return pairs_deliver_dev(k);
    return pairs_deliver_host(k, cs);
}

extern "C" int fm_collection_pairs_mutual_ratio(fm_ctx* ctx, fm_collection* c, const int32_t* pairs, int64_t n_pairs, double tau,
                                                int32_t symmetric, int64_t cap, int64_t* offsets, int32_t* qidx, int32_t* tidx,
                                                float* dist, double* ratio, int64_t* n_total)
{
    const CollPairsArgs a{"fm_collection_pairs_mutual_ratio", tau, symmetric, cap, offsets, qidx, tidx, dist, ratio,
                          false, nullptr, nullptr, FM_NO_STREAM, n_total};
    return coll_pairs_mutual(ctx, c, pairs, n_pairs, a);
}

extern "C" int fm_collection_pairs_mutual_ratio_dev(fm_ctx* ctx, fm_collection* c, const int32_t* pairs, int64_t n_pairs, double tau,
                                                    int32_t symmetric, int64_t cap, int64_t* d_offsets, int32_t* d_rows,
                                                    int64_t* n_total, void* consumer_stream)
{
    const CollPairsArgs a{"fm_collection_pairs_mutual_ratio_dev", tau, symmetric, cap, nullptr, nullptr, nullptr, nullptr, nullptr,
                          true, d_offsets, d_rows, consumer_stream, n_total};
    return coll_pairs_mutual(ctx, c, pairs, n_pairs, a);
}

// ---------------------------------------------------------------------------------------
// a wide query bank against every image of a wide collection: fm_collection_wide_mutual_ratio_each, _wide_knn2_each
// ---------------------------------------------------------------------------------------
// The match graph's machinery with "pair" p = (q, image p): the forward slot's output rows are the query bank's -- an operand
// outside the stack, with its own planes and fp16 scale (wide_f32.hip, part 5) -- the reverse slot's reduced rows are.  The
// chunks, tables, merge, join, scan and compaction are coll_pairs_mutual's (CollPairsArgs::q).
// The checks in front of it, in the header's order: handles, the collection's kind, the query's kind and width.
static int coll_wide_query_check(fm_ctx* ctx, fm_collection* c, const fm_bank* q, const char* who, const char* narrow)
{
    int rc = coll_check(ctx, c, who);
    if (rc != FM_OK) return rc;
    if (!q) return fail(ctx, FM_EINVAL, std::string(who) + ": query bank is NULL");
    if ((rc = refuse_bin2(ctx, q, who)) != FM_OK) return rc;
    if (!c->rows.empty() && !coll_is_wide(c))
        return fail(ctx, FM_EINVAL, std::string(who) + ": the collection holds images of another kind (not wide ones, fm_collection_add_wide); "
                                    "it is served by " + narrow);
    if (q->kind != FM_BANK_F32W)
        return fail(ctx, FM_EINVAL, std::string(who) + ": the query bank is not a wide float bank (FM_BANK_F32W, 129 <= dim <= 256)");
    if (c->dim != 0 && q->dim != c->dim) return fail(ctx, FM_EINVAL, std::string(who) + ": the query's width differs from the collection's");
    return FM_OK;
}

static int coll_wide_each(fm_ctx* ctx, fm_collection* c, const fm_bank* q, const char* narrow, CollPairsArgs a)
{
    const int rc = coll_wide_query_check(ctx, c, q, a.who, narrow);
    if (rc != FM_OK) return rc;
    a.q = q;
    return coll_pairs_mutual(ctx, c, nullptr, (int64_t)c->rows.size(), a);
}

extern "C" int fm_collection_wide_knn2_each(fm_ctx* ctx, fm_collection* c, const fm_bank* q, int32_t* idx, float* dist)
{
    CollPairsArgs a{"fm_collection_wide_knn2_each", 0.0, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, false, nullptr, nullptr, FM_NO_STREAM, nullptr};
    a.knn2 = true; a.k_idx = idx; a.k_dist = dist;
    return coll_wide_each(ctx, c, q, "fm_collection_knn2_each", a);
}

// fm_collection_wide_votes, mode 1 (api_collection.hip checks the arguments): the sweep above with the lists left on the device,
// the per-image ratio test counted there.  n_images > 0 and q->n > 0.
int coll_wide_each_votes(fm_ctx* ctx, fm_collection* c, const fm_bank* q, double tau, int64_t* votes)
{
    CollPairsArgs a{"fm_collection_wide_votes", tau, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, false, nullptr, nullptr, FM_NO_STREAM, nullptr};
    a.knn2 = true; a.k_votes = votes;
    return coll_wide_each(ctx, c, q, "fm_collection_votes", a);
}

extern "C" int fm_collection_wide_mutual_ratio_each(fm_ctx* ctx, fm_collection* c, const fm_bank* q, double tau, int32_t symmetric, int64_t cap,
                                                    int64_t* offsets, int32_t* qidx, int32_t* tidx, float* dist, double* ratio, int64_t* n_total)
{
    const CollPairsArgs a{"fm_collection_wide_mutual_ratio_each", tau, symmetric, cap, offsets, qidx, tidx, dist, ratio,
                          false, nullptr, nullptr, FM_NO_STREAM, n_total};
    return coll_wide_each(ctx, c, q, "fm_collection_mutual_ratio_each", a);
}

extern "C" int fm_collection_wide_mutual_ratio_each_dev(fm_ctx* ctx, fm_collection* c, const fm_bank* q, double tau, int32_t symmetric,
                                                        int64_t cap, int64_t* d_offsets, int32_t* d_rows, int64_t* n_total,
                                                        void* consumer_stream)
{
    const CollPairsArgs a{"fm_collection_wide_mutual_ratio_each_dev", tau, symmetric, cap, nullptr, nullptr, nullptr, nullptr, nullptr,
                          true, d_offsets, d_rows, consumer_stream, n_total};
    return coll_wide_each(ctx, c, q, "fm_collection_mutual_ratio_each", a);
}
