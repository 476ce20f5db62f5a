// Internal declarations shared by the HIP translation units of libfastmatch_hip.so.
// gfx950 (MI355X / CDNA4) only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>
#include "../../include/fastmatch_hip.h"
#include "ratio_cut.h"

namespace fm {

// ---- bank layout in HBM -------------------------------------------------------------
// rows8 : int8 [n_pad][128]   descriptor bytes XOR 0x80 (u8 -> i8 shift by 128; L2 is
//                             shift invariant), zero rows for padding, n_pad % 128 == 0
// norm  : int32 [n_pad]       nm = sum of squares of the int8 row (<= 2^21)
// aux   : int32 [n_pad/32][64] per 32-row unit = two 16-row MFMA tiles (sub = 0, 1), in the
//         accumulator order of v_mfma_i32_16x16x64_i8 (tile row rr: lane group rr >> 2,
//         register rr & 3):
//           aux[unit][32*sub +      rr] = -(nm >> 1)                       ("cinit")
//           aux[unit][32*sub + 16 + rr] = (1 - (nm & 1)) << 4 | (15 - id)  ("low": parity
//                                         npar and inverted in-lane order id = 4*sub + (rr&3))
//         Padding rows carry cinit = -2^25 (far below any real accumulator value, and
//         (cinit << 5) still fits int32) so they never beat a real row.
constexpr int kDim        = 128;
constexpr int kStageRows  = 128;                 // rows staged into LDS per pipeline step
constexpr int kTileRows   = 32;                  // one MFMA M-tile
constexpr int kAuxPerTile = 64;
constexpr int kPadCinit   = -(1 << 25);

struct Bank {
    int      kind   = 0;       // FM_BANK_I8 / FM_BANK_F32 / FM_BANK_BIN / FM_BANK_F32W
    int64_t  n      = 0;
    int      dim    = 0;
    int64_t  n_pad  = 0;       // multiple of kStageRows (>= kStageRows so empty banks stage)
    int64_t  cap_pad = 0;      // n_pad the arrays were allocated for (fm_bank_refill_u8_async keeps within it)
    void*    stage  = nullptr; // refill staging: cap_pad * 128 source bytes + the preparation kernel's flag words
    int8_t*  rows8  = nullptr;
    int32_t* norm   = nullptr;
    int32_t* aux    = nullptr;
    int32_t  usq_max = 0;      // FM_BANK_I8: largest |row|^2 of the uint8 rows (sqrt_tie_possible below)
    float*   rowsf  = nullptr; // FM_BANK_F32: [n_pad][128] float32, zero padded
    // FM_BANK_F32, for the fp16 filter (filter_f16.hip); "scaled" = times 2^kscale:
    uint16_t* rowsh = nullptr; // [n_pad][128] fp16 of the scaled rows
    float*   normf  = nullptr; // [n_pad] |scaled row|^2
    float*   auxf   = nullptr; // [n_pad] accumulator init -|scaled row|^2 / 2 (padding rows: -3.4e38)
    float    nm_max = 0.f;     // max |scaled row|^2
    int      kscale = 0;       // largest scaled magnitude lies in [2^13, 2^14)
    bool     filt_ok = false;  // every value is finite
    float    vfin_max = 0.f;   // FM_BANK_F32: largest finite magnitude (a float32 train collection refuses one above 2^57)
    double*  selfdist = nullptr;
    // the largest self distance, as the bits of the double (the maximum of the bit patterns: a pattern at or above +inf's --
    // inf, NaN, a sign bit -- means no ratio cut, ratio_cut.h); a device word behind selfdist[cap], valid for the rows
    // [0, sdmax_rows) of the array (fm_bank_set_selfdist, fm_self_dist_batch; -1: none)
    unsigned long long* sdmax = nullptr;
    int64_t  sdmax_rows = -1;
    // FM_BANK_BIN (K11, hamming.hip): dim = bytes per row (1 .. 64), ksteps = ceil(dim / 16) MFMA K steps of 128 bits
    int      ksteps = 0;
    uint8_t* rowsb  = nullptr; // [n_pad][16 ksteps] packed rows, zero padded
    uint8_t* rows4  = nullptr; // [n_pad][64 ksteps] FP4 image: bit 1 -> +1, bit 0 -> -1, padding 0
    // FM_BANK_BIN2 (K11b, hamming2.hip): dim and ksteps (the packed plane's 16-byte pieces) as for FM_BANK_BIN; the FP4 plane is
    // the tetrahedral image, 12 dim values in ksteps4 = ceil(12 dim / 128) K steps: rows4 is [n_pad][64 ksteps4] (fp4_steps below)
    int      ksteps4 = 0;
    // FM_BANK_I8 of dim 128, for the FP6 filter of the accepted-only sweep (filter6.hip, fp6_filter.h); all null: K1 only
    uint8_t* rows6  = nullptr; // [n_pad][128] e2m3 codes of the raw uint8 rows: four K-chunks of 32 codes (24 bytes) in 32-byte slots
    float*   aux6   = nullptr; // [n_pad / 128][256] accumulator start -floor(|m|^2 / 32) / 64 of a stage's rows (padding -3.4e38), the largest start among its real rows, 127 unused words
    int32_t* stat6  = nullptr; // [n_pad][4] |row|^2, |image|^2, |row - image|^2 (uint8 values), 0
    int32_t* max6   = nullptr; // [2] device words: the bank's largest |row|^2 and |row - image|^2
    // FM_BANK_F32W (K14, wide_f32.hip): dim = 129 .. 256; normf, auxf, nm_max, kscale, filt_ok and vfin_max as for FM_BANK_F32,
    // every 128-wide plane null
    float*    wrows  = nullptr; // [n_pad][256] float32, zero padded
    uint16_t* wrowsh = nullptr; // [n_pad][256] fp16 of the scaled rows
    // A bank that grew by appends (fm_bank_append_u8 / _f32) and has padding rows INSIDE it, below n (an append starts on a
    // 32-row tile): the bitmap of its real rows, one 64-bit device word per 64 rows of cap_pad (fm_mask's word layout: bit b
    // of word w = row 64 w + b).  Null for every bank without such gaps -- the kernels that mask padding by index (row < n)
    // test it only when it is there; the matrix-core sweeps need nothing (a padding row's accumulator start keeps it out).
    // A view (bank_rows_view) carries none: it is taken of one append's rows.
    unsigned long long* real = nullptr;
    unsigned long long* real_mem = nullptr;   // the allocation behind `real` (kept across fm_bank_refill_u8_async, which ends the gaps)
};

// Is row m a real row under a bank's `real` bitmap (see Bank)?  For the kernels that take it as an optional pointer.
__device__ __forceinline__ bool real_row(const unsigned long long* __restrict__ real, int m)
{
    return (real[m >> 6] >> (m & 63)) & 1ull;
}

// K steps (64 bytes each) per row of a binary bank's FP4 plane: the packed pieces for NORM_HAMMING, where the two coincide
inline int fp4_steps(const Bank& b) { return b.kind == FM_BANK_BIN2 ? b.ksteps4 : b.ksteps; }

// rows rounded up to whole 128-row stages
inline int64_t pad128(int64_t n) { return ((n + kStageRows - 1) / kStageRows) * kStageRows; }
inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
// Workspace layouts: the offset of a piece of `bytes` bytes behind `off`, which moves on by the bytes rounded up to `align`
// (a power of two).
inline size_t carve(size_t& off, size_t bytes, size_t align = 256)
{
    const size_t o = off;
    off += (bytes + align - 1) & ~(align - 1);
    return o;
}

// The rows [r0, r0 + n) of a bank's arrays as a bank of their own, for every kind: each plane that exists moves on by r0
// rows, the scale terms are the bank's (usq_max and nm_max stay upper bounds), n_pad = cap_pad = pad128(n) clipped to the
// rows the arrays have left.  The aux words exist per 32-row tile: a view that starts inside a tile has none and can only
// be the output side of an integer sweep, which does not read them.  No self distances: they belong to the whole bank.
inline Bank bank_rows_view(const Bank& b, int64_t r0, int64_t n)
{
    Bank v;
    v.kind = b.kind; v.n = n; v.dim = b.dim;
    v.ksteps = b.ksteps; v.ksteps4 = b.ksteps4; v.kscale = b.kscale; v.filt_ok = b.filt_ok; v.nm_max = b.nm_max; v.usq_max = b.usq_max; v.vfin_max = b.vfin_max;
    const int64_t room = (b.cap_pad > 0 ? b.cap_pad : b.n_pad) - r0;
    v.n_pad = v.cap_pad = pad128(n) < room ? pad128(n) : room;
    if (b.rows8) v.rows8 = b.rows8 + (size_t)r0 * kDim;
    if (b.norm)  v.norm = b.norm + r0;
    if (b.aux && r0 % kTileRows == 0) v.aux = b.aux + (r0 / kTileRows) * kAuxPerTile;
    if (b.rowsf) v.rowsf = b.rowsf + (size_t)r0 * kDim;
    if (b.rowsh) v.rowsh = b.rowsh + (size_t)r0 * kDim;
    if (b.normf) v.normf = b.normf + r0;
    if (b.auxf)  v.auxf = b.auxf + r0;
    if (b.rowsb) v.rowsb = b.rowsb + (size_t)r0 * b.ksteps * 16;
    if (b.rows4) v.rows4 = b.rows4 + (size_t)r0 * fp4_steps(b) * 64;
    if (b.wrows)  v.wrows = b.wrows + (size_t)r0 * 256;
    if (b.wrowsh) v.wrowsh = b.wrowsh + (size_t)r0 * 256;
    return v;
}

// OpenCV orders candidates by the float32 root of d2; the integer route orders by d2, which is the same
// order unless a d2 reaches 4 197 200, where two integers start to share a float32 root (kSqrtTieMin,
// tile_ops.h).  Rows are non-negative, so d2(a, b) <= |a|^2 + |b|^2: a bank pair whose largest row
// norms stay below that can skip every repair step (all SIFT banks: |d|^2 ~ 2.6e5).
inline bool sqrt_tie_possible(const Bank& a, const Bank& b)
{
    return (int64_t)a.usq_max + (int64_t)b.usq_max >= 4197200;
}

// ---- per-context tuning (fm_ctx_set_option; the FM_* environment variables only seed the defaults
// when a context is created) -------------------------------------------------------------------
struct Tuning {
    int nb = 0, nsplit = 0, nw = 0;   // K1 launch shape overrides, 0 = the built-in rule
    int nbuf = 0;                     // K1 / K2 LDS stage buffers: 0 = 3 (top-2 shapes other than 4 blocks per wave: 2)
    int prio = 1;                     // s_setprio around a unit's MFMA burst (three-buffer kernel)
    int glds = 1;                     // LDS-DMA staging (0: through registers)
    int coop = 1;                     // cross-workgroup K-th-best bounds
    int f32_filter = 1;               // float32 route: 0 = K5 only, 1 = fp16 filter for large calls, 2 = always
    int f32_nw = 0, f32_nsplit = 0;   // K8 launch shape overrides
    int f32_fused = -1;               // K8: rescoring inside the filter (-1 = when the plan has one split)
    int f32_lpc = 0;                  // K8 rescoring: lanes per output row (0 = rule)
    int f32_bound_every = 4;          // K8: re-read the shared bounds every n-th stage once a sweep is 8 stages old (a power of two)
    int batch_group = 8;              // fm_match_accepted_batch: most pairs per distance-kernel launch (<= kRRBatchMax)
    int batch_tail = 2;               // ... pairs of the short launch a run ends with (0 = none)
    int async_time_every = 4;         // async calls: every n-th call carries kernel timing events (0 = none)
    int expand_big = 1;               // K7: re-run pairs that overflow the 2048-row round in the 4096-row variant
    int expand_huge = 1;              // K7: re-run pairs that still overflow in the variant that chunks a radius subset of any size
    int delegated_rounds = 0;         // (counter, saturating) rounds whose cross-check the dense kernels ran since it was last set to 0
    int expand_delegate = 1500000;    // K7: a chunked round of at least this many descriptor pairs is parked and its cross-check run
                                      // by the dense kernels on the whole GPU (0 = never: the round's own workgroup does it)
    int expand_grow = 2;              // K7: how often a run that fills its stack / result list / table is repeated in a
                                      // state four times as large (0 = never: the status goes to the caller)
    int expand_prof = 0;              // K7: per-phase timers of pair 0 on stderr
    int bound_every = 16;             // K1 / K2: re-read the shared bounds every n-th stage once a sweep is 8 stages old (a power of
                                      // two; r04 A/B on two boxes, ms per pair in the 12-pair launch: 1 -> 0.8356 / 0.8501, 8 -> 0.8290 /
                                      // 0.8399, 32 -> 0.8277, 1024 -> 0.8340: profiles/r04c_k1_bound_every_*)
    int refill_grid = 128;            // fm_bank_refill_u8_async: workgroups of the preparation kernel (each walks its share of the tiles)
    int self_tri = 1;                 // fm_self_dist: 1 = the triangular sweep (every distance once) from 32768 rows on (integer banks) /
                                      // 65536 (float32-route banks, r06), 0 = the masked full sweep always, 2 = the triangular sweep always (tests)
    int tri_stages = 0;               // ... stages (128 rows) per slice of the triangular sweep (0 = plan_tri's search)
    int k1_order = 0;                 // K1: workgroup -> (chunk, split) mapping (rowreduce.hip, map_block): 0 split major,
                                      // 1 an XCD owns output chunks, 2 an XCD owns a contiguous share of the split-major order
    int radius_ws_bytes = 1 << 30;    // K10: device bytes for the candidate keys of one query chunk (radius.hip); a single
                                      // query row whose list needs more still runs, in a chunk of its own
    int fp6_filter = 1;               // accepted-only sweeps with a ratio cut: 1 = FP6 filter + exact rescoring (filter6.hip), 0 = K1
    int fp6_cap = 1 << 20;            // ... records per pair of the filter's list; a pair that needs more is redone by K1
    int fp6_nsplit = 0;               // ... the filter's splits of a streamed bank (0 = fp6_plan.h's rule, or a forced "nsplit")
    int masked_mfma = 1;              // K13: fm_knn_masked on the integer route with k <= 2: 1 = the masked MFMA sweep, 0 = the masked K9 kernel
    int mask_pack_words = (1 << 26) - 4;  // K13: mask words one launch of the pack / fill kernels covers (64 work-items per word: < 2^32 per launch)
    int coll_ws_bytes = 0;            // fm_collection_match_accepted_each / _xcheck1_each: device bytes for the per-(image, query row)
                                      // arrays of one chunk of images (25 / 17 per entry); 0 = a quarter of the free device memory;
                                      // fm_collection_pairs_mutual_ratio: partials, lists and per-row arrays of one chunk of pairs (0 = 2^30)
};

// ---- K1: row-reduce kernel launcher ---------------------------------------------------
// For every row c of bank `cols`, reduce over all rows m of bank `red` the key
// (d2(c,m), m) lexicographically and keep the KTOP smallest.  Writes, per split of the
// reduction range, packed candidates  (uint64)d2 << 32 | m  (~0 = none) to
// partial[(split*ncols_alloc + c)*KTOP + k].
struct RowReducePlan {
    int nb;            // blocks of 16 output rows per wave (4 or 8)
    int nw = 4;        // waves per workgroup (4, 8 or 16)
    int ncols_alloc;   // columns covered by the grid (multiple of 16*nb*nw)
    int nchunks;
    int nsplit;
    int stages_per_split;
    int nbuf = 0;      // stage buffers (0 = rule: rowreduce.hip nbuf_choice)
    int prio = 1;      // s_setprio around the MFMA burst
    int order = 0;     // Tuning::k1_order
    int bound_every = 1;   // Tuning::bound_every
    size_t partial_bytes(int ktop) const { return (size_t)nsplit * ncols_alloc * ktop * 8; }
    size_t bound_bytes() const { return (size_t)ncols_alloc * 4 * 2; }   // (top-2 launches keep two arrays)
};
RowReducePlan plan_rowreduce(int64_t ncols_pad, int64_t nred_pad, const Tuning& tn);
// cut (top-1 only): device word D* of the ratio test (ratio_cut.h); candidates at d2 >= D* may be dropped (their rows may
// then keep the empty key).  Only the accepted-only calls pass one: every reported row there passes the test.
// f6 (with a cut, top-1): the FP6 filter's workspace; a pair that qualifies (filter6_usable, K1's batched shape) is swept by
// the filter with exact rescoring and K1 only as its guarded fallback (filter6.hip)
struct Filter6Ws {
    uint2*    rec;     // [pairs of a launch][cap] records (output row, 32-row unit of the streamed bank)
    unsigned  cap;
    unsigned* cnt;     // [pairs of a launch][2]: records appended (may exceed cap), need_k1
    int       nsplit = 0;      // the filter's splits of a streamed bank: 0 = its own rule for the launch (fp6_plan.h), > 0 this
                               // many (option "fp6_nsplit"), < 0 K1's plan (a forced "nsplit" governs both sweeps)
    int       resident = 256;  // workgroups of the filter the device holds at a time: its CUs
    // set: the rescoring and the guarded K1 run on `side`, behind ev_sweep (recorded on the sweep's stream behind the filter),
    // and ev_done is recorded on `side` behind them; null: all three kernels follow each other on the sweep's stream
    hipStream_t side = nullptr;
    hipEvent_t  ev_sweep = nullptr, ev_done = nullptr;
};
hipError_t launch_rowreduce(const Bank& cols, const Bank& red, int ktop, const RowReducePlan& plan,
                            unsigned long long* partial, int* bound, bool use_glds, hipStream_t stream,
                            const unsigned* cut = nullptr, const Filter6Ws* f6 = nullptr);
// ---- K12: FP6 filter of the accepted-only sweep (filter6.hip) ----
bool filter6_usable(const Bank& cols, const Bank& red);     // both banks carry the FP6 plane
hipError_t launch_prep6(const Bank& b, int grid_max, hipStream_t stream);     // the plane of rows [0, n_pad) from rows8 (grid_max 0: no limit)
hipError_t launch_filter6(int n, const Bank* const* cols, const Bank* const* red, const RowReducePlan* plans,
                          unsigned long long* const* partial, const unsigned* const* cut, const Filter6Ws& ws, hipStream_t stream);
int rowreduce_grid(const RowReducePlan& plan);      // workgroups per bank pair (padded under orders 1 and 2)
// fm_self_dist: top-1 of every row over the OTHER rows of its own bank (masked diagonal)
RowReducePlan plan_rowreduce_self(int64_t n_pad, const Tuning& tn);
hipError_t launch_rowreduce_self(const Bank& bank, const RowReducePlan& plan, unsigned long long* partial, int* bound,
                                 bool use_glds, hipStream_t stream);

// fm_self_dist on large integer banks: the triangular sweep (rowreduce.hip, "TRI") -- every distance of a bank
// against itself once, bound[] carries the result (d2(i) = norm[i] + 1 - bound[i]; <= kTriNoBoundHost: none).
struct TriPlan {
    int nchunks = 0, ncols_alloc = 0, npieces = 0, stages = 0;
    int ndiag = 0;                     // the first ndiag workgroups of the table are launch A (the diagonal blocks)
    int bound_every = 16;              // Tuning::bound_every (a power of two)
};
TriPlan plan_tri(int64_t n_pad, int target_stages, std::vector<int>* table);
constexpr int64_t kTriMaxRows = (int64_t)1 << 26;      // banks beyond this take the masked full sweep (the workgroup count of
                                                        // the triangular one grows with the square of the rows: int32 from ~75M on)
hipError_t launch_rowreduce_tri(int n, const Bank* const* banks, const TriPlan* plans, int* const* bound, bool prio, hipStream_t stream);
constexpr int kTriNoBoundHost = -(1 << 25);     // (a real pair's word is >= -3 * 2^21, a padding row's or the masked diagonal's ~ -2^26)

// ---- K5: float32 route (dist_f32.hip); partial keys carry float32 distance bits ----------
// run_flag: device word; the kernel returns at once when *run_flag == 0 (null = always run) and
// counts its runs in run_flag[2].
RowReducePlan plan_rowreduce_f32(int64_t ncols_pad, int64_t nred_pad, int force_nsplit);
hipError_t launch_rowreduce_f32(const Bank& cols, const Bank& red, int ktop, const RowReducePlan& plan,
                                unsigned long long* partial, const int* run_flag, hipStream_t stream, bool self = false);

// ---- K8: fp16 MFMA filter + exact rescoring for the float32 route (filter_f16.hip) --------
// Writes the same keys as K5 into split 0 of `partial` (the caller presets the other splits to
// ~0).  flag: device words [0] K5 must redo the call, [1] output rows rescanned in full,
// [2] K5 runs, [3] rescans in total, [4 .. 4 + 256) the rescanned rows, then tickets + rescan scratch
// (filter_flag_bytes() in all); [0] and [1] are reset per call.
struct FilterPlan {
    int nw;            // waves per workgroup (4 or 8)
    int nc;            // blocks of 16 output rows per wave (2 or 4)
    int ncols_alloc;
    int nchunks;
    int nsplit;
    int stages_per_split;   // 128-row stages
    int fused = -1, lpc = 0; // Tuning::f32_fused / f32_lpc
    int bound_every = 4;     // Tuning::f32_bound_every
    int64_t aux_elems = 0;   // floats of the rescaled accumulator inits (banks of different scales)
    size_t slots_bytes() const { return (size_t)nsplit * ncols_alloc * 16 * 8; }
    size_t aux_bytes() const { return ((size_t)aux_elems * 4 + 255) & ~(size_t)255; }
    size_t bound_bytes() const { return (size_t)ncols_alloc * 8; }   // best and 2nd best
};
FilterPlan plan_filter(int64_t ncols_pad, int64_t nred_pad, const Tuning& tn);
int filter_empty_bound();
size_t filter_flag_bytes();       // size of the device words launch_filter's `flag` points at
bool filter_usable(const Bank& cols, const Bank& red);   // both banks carry filter planes of compatible scale
hipError_t launch_filter(const Bank& cols, const Bank& red, int ktop, const FilterPlan& plan,
                         unsigned long long* slots, int* bound, int* flag,
                         unsigned long long* partial, hipStream_t stream, bool self = false, float* aux_scratch = nullptr);

// fm_self_dist of a float32-route bank by the triangular sweep (filter_f16.hip, TRI): every distance once
size_t filter_tri_bytes(int ncols_alloc);
hipError_t launch_filter_tri(const Bank& bank, const TriPlan& plan, int bound_every, void* ws, int* bound, int* flag,
                             unsigned long long* partial, hipStream_t stream);

// ---- K9: exact k-NN lists for k up to 8 on the vector ALUs (knn_k.hip; the reference's own calls -- k = 1, 2 -- stay on K1 / K8)
size_t knnk_partial_bytes(int64_t nq, int64_t nt, int k);
hipError_t launch_knnk(const Bank& q, const Bank& t, int k, unsigned long long* partial, int32_t* d_idx, float* d_dist, hipStream_t stream);
int knnk_splits(int64_t nq, int64_t nt);
// K9 under a bit mask (K13): mask[q][mwords] 64-bit words, bit b of word w = train row 64 w + b is permitted; 1 <= k <= 8
hipError_t launch_knnk_masked(const Bank& q, const Bank& t, int k, unsigned long long* partial, int32_t* d_idx, float* d_dist,
                              hipStream_t stream, const unsigned long long* mask, int64_t mwords);
// merge of the per-split lists (keys: float32 distance bits << 32 | row) into idx / dist [nq][k]
hipError_t launch_knnk_merge(const unsigned long long* partial, int nsplit, int nq, int k, int32_t* d_idx, float* d_dist, hipStream_t stream);

// ---- K11: Hamming distance of binary banks (hamming.hip) --------------------------------------------------------------------
// Top-KTOP (1 or 2) of every row of `cols` over the rows of `red` on the FP4 matrix cores; per split of the reduction range
// the keys (float32 bits of h << 32 | row of red), ascending, at partial[(split * ncols_alloc + c) * KTOP + k].
struct HamPlan {
    int nchunks = 0, ncols_alloc = 0, nstages = 0, nsplit = 0, stages_per_split = 0;
    size_t partial_bytes(int ktop) const { return (size_t)nsplit * ncols_alloc * ktop * 8; }
};
HamPlan plan_hamming(int64_t ncols_pad, int64_t nred_pad);
// stage_real (train collections): real rows per 128-row stage of `red`, an index mask per stage; null = a plain bank
hipError_t launch_hamming(const Bank& cols, const Bank& red, int ktop, const HamPlan& plan, unsigned long long* partial, hipStream_t stream,
                          const int* stage_real = nullptr);
// Hamming self distances (fm_hamming_self_dist(_batch)): the top-1 sweep of up to kHamSelfMax banks of ONE ksteps against
// themselves, the diagonal dropped, in one launch.  table (device, int4 per workgroup): {bank of the launch, chunk, split, 0};
// bank j's keys go to b[j].partial in its plan's layout ([nsplit][ncols_alloc]), every word written.  The merge takes the
// minimum over the splits and writes b[j].out[i] = (double)h, +inf where no candidate exists (a bank of one row).
constexpr int kHamSelfMax = 16;
struct HamSelfBank {
    const uint8_t* rows4;                // the bank's FP4 image
    unsigned long long* partial;
    double* out;                         // [n]
    int n, W;                            // real rows, bits per row
    HamPlan plan;                        // plan_hamming(n_pad, n_pad)
};
struct HamSelfArgs { HamSelfBank b[kHamSelfMax]; };
hipError_t launch_hamming_self(const HamSelfArgs& a, int nbanks, int ksteps, const void* d_table, int n_workgroups, hipStream_t stream);
hipError_t launch_hamming_self_merge(const HamSelfArgs& a, int nbanks, hipStream_t stream);
// packed rows + FP4 image of n device rows of `bytes` bytes, `pitch` bytes apart (0 = dense: an uploaded [n][bytes] matrix)
// (b.n_pad, b.ksteps, b.rowsb, b.rows4 set by the caller)
hipError_t launch_hamming_prep(const uint8_t* d_src, int64_t n, int bytes, const Bank& b, hipStream_t stream, int64_t pitch = 0);
// k-NN lists for 1 <= k <= 8 on the vector ALUs (partial: knnk_partial_bytes)
// mask (K13): the bit mask of fm_knn_masked, [q.n][mwords] words, or null
hipError_t launch_hamming_knnk(const Bank& q, const Bank& t, int k, unsigned long long* partial, int32_t* d_idx, float* d_dist, hipStream_t stream,
                               const int* stage_real = nullptr, const unsigned long long* mask = nullptr, int64_t mwords = 0);

// ---- K11b: NORM_HAMMING2 on binary banks of 2-bit cells (hamming2.hip) --------------------------------------------------------
// K11's launchers for FM_BANK_BIN2 pairs: the same plans (plan_hamming), the same key layout, h2 for h.
inline int ham2_fp4_steps(int bytes) { return (12 * bytes + 127) / 128; }
// packed rows + tetrahedral FP4 image (b.n_pad, b.ksteps, b.ksteps4, b.rowsb, b.rows4 set by the caller)
hipError_t launch_hamming2_prep(const uint8_t* d_src, int64_t n, int bytes, const Bank& b, hipStream_t stream, int64_t pitch = 0);
hipError_t launch_hamming2(const Bank& cols, const Bank& red, int ktop, const HamPlan& plan, unsigned long long* partial, hipStream_t stream,
                           const int* stage_real = nullptr);
// k-NN lists for 3 <= k <= 8 on the vector ALUs (partial: knnk_partial_bytes)
hipError_t launch_hamming2_knnk(const Bank& q, const Bank& t, int k, unsigned long long* partial, int32_t* d_idx, float* d_dist, hipStream_t stream);
// radiusMatch (radius.hip's r_sweep launches these): thr[i] = the least dot product of a hit of query row i
// (ham2_radius_dot_min, ham_radius.h)
hipError_t launch_hamming2_radius_limits(const float* radius, float radius_all, int nq, int P, float* thr, hipStream_t stream);
struct Ham2RSweep {
    const uint8_t* q4; const uint8_t* t4;   // the FP4 planes, from this launch's first query row on / the train bank's
    int ks, P3;                             // FP4 K steps per row (1 .. 6), 3 * cells per row
    int nq, nt, per;                        // query rows of the launch, train rows, train rows per split (whole 128-row stages)
    const float* thr;                       // per query row of the launch
    unsigned* cnt;                          // count sweep: hit counts; fill sweep: cursors (zeroed)
    const int64_t* off; int64_t base;       // fill sweep: segment offsets of the launch's query rows, minus `base`
    unsigned long long* keys;               // fill sweep: (float32 bits of h2 << 32 | train row)
};
hipError_t launch_hamming2_radius(const Ham2RSweep& p, bool fill, int nsplit, hipStream_t stream);

// ---- K14: wide float32 banks, 129 .. 256 values per row (wide_f32.hip) ------------------------------------------------------
constexpr int kWideDim = 256;
// b.wrows from n source rows of FM_DT_F32 / F16 / BF16 elements `pitch` bytes apart (device memory: a staged host matrix or
// the caller's tensor); stat[0] = largest finite magnitude (float bits), stat[1] = a value is not finite (zeroed by the caller)
hipError_t launch_wide_copy(const void* src, int dtype, int64_t pitch, int64_t n, int dim, const Bank& b, int* stat, hipStream_t stream);
// b.wrowsh, normf, auxf from b.wrows and b.kscale; stat[0] = largest |scaled row|^2 (float bits; zeroed by the caller)
hipError_t launch_wide_planes(const Bank& b, int* stat, hipStream_t stream);
// K5's kernel at the wide row: plan_rowreduce_f32's plans, K5's keys, K5's run_flag protocol
// self (fm_wide_self_dist; cols and red are one bank, ktop 1): row n is no candidate of output row n
hipError_t launch_wide_exact(const Bank& cols, const Bank& red, int ktop, const RowReducePlan& plan, unsigned long long* partial,
                             const int* run_flag, hipStream_t stream, bool self = false);
// fp16 matrix-core filter + exact rescoring into split 0 of `partial` (preset to ~0 by the caller, as the 64-bit *cnt, flag[0] and
// gbound[0 .. cols.n_pad) to 0); flag[0] = 1 afterwards: the record list overflowed and launch_wide_exact must redo the call
struct WideFilterPlan {
    int nchunks = 0, ntiles = 0, nsplit = 0, tiles_per_split = 0;
    unsigned cap = 0;                                    // records of the list
    size_t list_bytes() const { return (size_t)cap * 8; }       // (and cap * 4 for the records' scores)
};
bool wide_filter_usable(const Bank& cols, const Bank& red);
WideFilterPlan plan_wide_filter(int64_t ncols_pad, int64_t ncols, int64_t nred_pad, const Tuning& tn);
hipError_t launch_wide_filter(const Bank& cols, const Bank& red, int ktop, const WideFilterPlan& plan, uint2* list, float* lscore,
                              unsigned* gbound, unsigned long long* cnt, int* flag, unsigned long long* partial, hipStream_t stream,
                              bool self = false);
// launch_wide_filter's second kernel alone: the records of `list` rescored exactly into split 0 of `partial` (the masked filter
// of wide_masked.hip leaves records in the same form)
hipError_t launch_wide_rescore(const Bank& cols, const Bank& red, int ktop, unsigned cap, const uint2* list, const float* lscore,
                               const unsigned* gbound, const unsigned long long* cnt, int* flag, unsigned long long* partial, hipStream_t stream,
                               bool self = false);
// ---- K14 under a mask (wide_masked.hip): fm_wide_knn_masked's two sweeps.  mask: fm_mask's words [q.n][mwords], mwords =
// t.n_pad / 64; partial: [plan.nsplit][q.n][ktop] keys, K9's layout (launch_knnk_merge merges it) ----
// the masked filter + launch_wide_rescore (presets as for launch_wide_filter); ktop 1 or 2
hipError_t launch_wide_masked_filter(const Bank& q, const Bank& t, int ktop, const WideFilterPlan& plan, const unsigned long long* mask,
                                     int64_t mwords, uint2* list, float* lscore, unsigned* gbound, unsigned long long* cnt, int* flag,
                                     unsigned long long* partial, hipStream_t stream);
// the masked exact kernel under K5's run_flag protocol; writes every key of `partial`
hipError_t launch_wide_masked_exact(const Bank& q, const Bank& t, int ktop, const RowReducePlan& plan, const unsigned long long* mask,
                                    int64_t mwords, unsigned long long* partial, const int* run_flag, hipStream_t stream);
// ---- K14 over a wide collection's stack (wide_stack.hip): the top-2 sweeps of fm_collection_wide_knn and its kin.  stack: the
// collection's stack as one bank (n = n_pad = whole 128-row stages); st_real: the real rows per stage (coll_tab.h), which the
// kernels test every reduced row against; keys carry PHYSICAL rows.  Plans: plan_wide_filter / plan_rowreduce_f32 over
// (q.n_pad, stack.n_pad); partial: [plan.nsplit][plan.ncols_alloc][2] ----
// the stack filter + launch_wide_rescore (presets as for launch_wide_filter)
hipError_t launch_wide_stack_filter(const Bank& q, const Bank& stack, const int32_t* st_real, const WideFilterPlan& plan, uint2* list,
                                    float* lscore, unsigned* gbound, unsigned long long* cnt, int* flag, unsigned long long* partial,
                                    hipStream_t stream);
// the stack exact kernel under K5's run_flag protocol; writes every key of `partial`
hipError_t launch_wide_stack_exact(const Bank& q, const Bank& stack, const int32_t* st_real, const RowReducePlan& plan,
                                   unsigned long long* partial, const int* run_flag, hipStream_t stream);
// Table forms (top-2) for a chunk of image pairs of one wide stack (fm_collection_pairs_mutual_ratio): a slot is one direction
// of one pair, both operands views of `stack` that start on a 128-row stage -- or, with WideTableLaunch::outside, one of them
// rows of a bank outside the stack (fm_collection_wide_mutual_ratio_each: a query bank).  The slots lie side by side in the chunk's
// output-row space -- slot s owns [row0, row0 + pad128(ncols)) -- which indexes gbound, partial [rows][2] and the records.
struct WideSlot {
    int col0, ncols;                        // output rows: first physical row of the stack, real rows (>= 1)
    int red0, nred;                         // reduced rows: the same
    int ntiles, tiles_per_split, nsplit;    // the filter's shape for this slot (plan_wide_filter's fields)
    int row0;                               // the slot's first row in the chunk's output-row space (a multiple of 128)
    // an operand outside the stack (WideTableLaunch::outside; part 5 of wide_f32.hip): which side it is -- that side's first
    // row is 0 -- and the slot's scale terms, WideFilterParams' fields of the same names.  Without one: 0, 1, 1, the stack's.
    int outside;
    float cscale, nscale, red_nm_max;
};
constexpr int kWideOutCols = 1, kWideOutRed = 2;      // WideSlot::outside
struct WideTableLaunch {
    const WideSlot* d_slots;                // [n]
    const int* d_wg0;                       // [n + 1] first workgroup of each slot in the filter's grid (nchunks * nsplit each), then the total
    const int* d_rowp;                      // [n + 1] row0 of each slot, then the chunk's rows
    int n, fwg;                             // slots, the filter's grid
    int64_t rows;                           // the chunk's rows (a multiple of 128)
    const Bank* outside = nullptr;          // the bank the slots' `outside` sides are rows of (same dim as the stack), or null
};
// the filter and the rescoring into `partial` (preset to ~0, *cnt, flag[0] and gbound[0 .. rows) to 0); flag[0] = 1 afterwards:
// the chunk's list (cap records, a multiple of 64) overflowed and launch_wide_exact_table must redo the chunk
hipError_t launch_wide_filter_table(const Bank& stack, const WideTableLaunch& tl, unsigned cap, uint2* list, float* lscore, unsigned* gbound,
                                    unsigned long long* cnt, int* flag, unsigned long long* partial, hipStream_t stream, int ktop = 2);
// the exact kernel over the same table, one split per slot, under K5's run_flag protocol; writes every row of `partial`
// ktop 1 (both launches; needs WideTableLaunch::outside): the top-1 forms, partial [rows] -- fm_collection_wide_match_accepted_each
hipError_t launch_wide_exact_table(const Bank& stack, const WideTableLaunch& tl, unsigned long long* partial, const int* run_flag,
                                   hipStream_t stream, int ktop = 2);

// ---- K13: k-NN under a bit mask (masked.hip) ------------------------------------------------------------------------------
// Integer route, k = 1 or 2, on the matrix cores: the masked top-k of every row of q over the rows of t (t may be a
// collection's stack: the mask's bits of padding rows are 0), merged into d_idx / d_dist [q.n][k].
size_t masked_i8_partial_bytes(int64_t nq, int64_t nt, int k);
hipError_t launch_masked_i8(const Bank& q, const Bank& t, int k, const unsigned long long* mask, int64_t mwords,
                            unsigned long long* partial, int32_t* d_idx, float* d_dist, hipStream_t stream);

// ---- K4: one workgroup per expansion round (rounds.hip) --------------------------------
hipError_t launch_rounds(const Bank& q, const Bank& t, const int32_t* d_q_rows, const int64_t* d_q_off,
                         const int64_t* d_t_off, int64_t n_rounds, int32_t* d_tidx, float* d_dist,
                         double* d_ratio, hipStream_t stream);
int round_qcap();
struct RoundF32;   // round_body_f32.h
hipError_t launch_rounds_f32(const RoundF32& rf, const double* q_selfdist, const int32_t* d_q_rows, const int64_t* d_q_off,
                             const int64_t* d_t_off, int64_t n_rounds, int32_t* d_tidx, float* d_dist,
                             double* d_ratio, hipStream_t stream);

// ---- K7: device-resident expansion loop (expand.hip) ------------------------------------
constexpr int kRRBatchMax = 16;           // bank pairs per batched row-reduce launch
hipError_t launch_rowreduce_batch(int n, const Bank* const* cols, const Bank* const* red, const RowReducePlan* plans,
                                  unsigned long long* const* partial, int* const* bound, hipStream_t stream, bool self = false,
                                  const unsigned* const* cut = nullptr,       // (cut[i]: as launch_rowreduce's, per pair; not for self)
                                  const Filter6Ws* f6 = nullptr,              // (with a cut for every pair: launch_rowreduce's)
                                  bool* off_stream = nullptr);     // out: the keys are complete at f6->ev_done, not on `stream`
// top-2 form of the batched launch (fm_collection_knn2_each): bound[i] = pair i's two bound arrays ([2 * ncols_alloc]) or null
hipError_t launch_rowreduce_batch2(int n, const Bank* const* cols, const Bank* const* red, const RowReducePlan* plans,
                                   unsigned long long* const* partial, int* const* bound, hipStream_t stream);
// table-driven form of the batched top-2 launch (fm_collection_pairs_mutual_ratio): any number of slots, descriptors and the
// prefix array of first workgroups in device memory.  A table of n slots is rowreduce_table_bytes(n) bytes, the same on the
// host, where it is built -- rowreduce_table_set: slot i under its plan in the batched shape, owning the workgroups from
// first_wg on; returns how many (> 0; -1: a plan in another shape) -- then _end with the grid -- and on the device, where the
// caller has copied it before the launch.  Every slot has at least one workgroup.
size_t rowreduce_table_bytes(int n);
int rowreduce_table_set(void* h, int n, int i, int first_wg, const Bank& cols, const Bank& red, const RowReducePlan& plan,
                        unsigned long long* partial, int* bound);
void rowreduce_table_end(void* h, int n, int total_wg);
hipError_t launch_rowreduce_table2(const void* d_table, int n, int total_wg, hipStream_t stream);
hipError_t launch_expand(const void* d_pairs, int n_pairs, bool f32, int tier, hipStream_t stream);   // all pairs of one kind / capacity tier (expand.hip)
int expand_cand_cap();
int expand_cand_cap_big();

// ---- result gather over RCCL (comm.hip; RCCL is dlopen'ed on first use) -----------------------
int comm_unique_id(void* id128, std::string* err);
int comm_init(int device, int nranks, int rank, const void* id128, void** comm_out, std::string* err);
int comm_destroy(void* comm);
int comm_gather(void* comm, const int32_t* d_rows, const int64_t* d_count, int64_t cap,
                int32_t* d_all_rows, int64_t* d_all_counts, hipStream_t stream, std::string* err);

}  // namespace fm

struct fm_bank : fm::Bank {};
