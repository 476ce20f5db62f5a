// What the translation units behind the train collections share: the collection object, the limits its padding rows rest on,
// and the helpers of api_collection.hip (which defines them) that api_pairs.hip (the match graph) calls.
// Internal: nothing here is part of include/fastmatch_hip.h.
#pragma once
#include "ctx_internal.h"
#include "coll_tab.h"

constexpr int kCollPadNorm = 1 << 26;
constexpr float kCollPadF32 = 1.0e18f;           // 128 * (1e18 + kCollF32Max)^2 = 1.7e38 stays finite in float32
// Masking by value holds while a padding row is farther from every query row than every real row is.  With all finite
// magnitudes <= L, per dimension |q - pad| >= 1e18 - L and |q - t| <= 2 L, so 3 L < 1e18 suffices (for every width: the
// dimensions beyond `dim` hold 0 in q and t and 1e18 in a padding row).  L = FM_COLLECTION_F32_MAX = 2^57 = 1.44e17
// (3 L = 4.3e17).  Images and query banks beyond it are refused (FM_EUNSUPPORTED), never answered differently: at
// 9e17 a query row is nearer to the padding rows (1.1e18) than to real rows of 1e16 (1.0e19), K5 and K9 would list
// padding (-> -1 / inf) where the filter path lists real rows.  Non-finite values are outside the limit's reach and
// harmless: their distances are inf or NaN to real and padding rows alike, and no kernel lists those.
constexpr float kCollF32Max = 144115188075855872.0f;      // 2^57
static_assert(3.0 * kCollF32Max < kCollPadF32, "padding rows must stay behind every real row");

struct fm_collection {
    fm_ctx* ctx = nullptr;
    fm::Bank stack;                       // kind = the collection's; n = n_pad = used rows, cap_pad = allocated rows
    int dim = 0;                          // 0: no non-empty image yet
    int src = 0;                          // 1: images came as uint8, 2: as float32, 3: as binary rows, 4: as wide rows (0: none yet)
    float wvmax = 0.f;                    // wide: the largest finite magnitude added so far
    bool wscale = false;                  // wide: stack.kscale was chosen (from the first magnitude above 0)
    int64_t used = 0, total = 0;          // physical rows in use (a multiple of 128), real rows
    std::vector<int64_t> rows, phys;      // per image
    std::vector<int32_t> usq;             // per image: largest |row|^2 (sqrt_tie_possible)
    int32_t* d_tab = nullptr;             // stage image [nstages] | stage real rows [nstages] | first row [n_images]
    size_t tab_bytes = 0;
    bool dirty = true;
    uint64_t gen = 0;                     // changes with every add and clear, unique across collections (fm_mask_create_coll remembers it)
    int64_t nstages() const { return used / fm::kStageRows; }
    const int32_t* st_img() const { return d_tab; }
    const int32_t* st_real() const { return d_tab + nstages(); }
    const int32_t* img_phys() const { return d_tab + 2 * nstages(); }
};

// ---- api_collection.hip ----------------------------------------------------------------------------------------------------
// The handles of a collection call: ctx and c are set and belong together (FM_EINVAL with a message otherwise).
int coll_check(fm_ctx* ctx, const fm_collection* c, const char* who);
inline bool coll_is_wide(const fm_collection* c) { return c->src == 4; }
// A bank view of image i (rows of the stack's arrays; nm_max stays the collection's largest norm: an upper bound).  Inline: the
// match graph takes a dozen views per pair while it builds its tables.
inline fm::Bank coll_view(const fm_collection* c, int i)
{
    fm::Bank v = fm::bank_rows_view(c->stack, c->phys[(size_t)i], c->rows[(size_t)i]);
    v.usq_max = c->usq[(size_t)i];
    return v;
}
// One-slot merge of a sweep's partials into the lists from entry `out` on (CollSlot::out); ps = null: no reduced rows, every
// entry -1 / +inf.
int coll_merge_one(fm_ctx* ctx, const PairSweep* ps, fm::CollTab tab, int64_t nq, int64_t out, int32_t* d_img, int32_t* d_idx, float* d_dist);
// One launch of coll_sqrt_fix_kernel (kFixGrid workgroups) on `stream`: the kernel's arguments, in its order.  (The kernel
// lives in api_collection.hip and the build links no device code across units: another unit launches it through this.)
hipError_t launch_coll_sqrt_fix(const unsigned* fix, const int8_t* col_rows, const int32_t* col_norm, const int8_t* red_rows,
                                const int32_t* red_norm, int nred, fm::CollTab tab, int64_t out, int32_t* img, int32_t* idx, float* dist,
                                hipStream_t stream);
// One launch of coll_votes_kernel on `stream`: the ratio test d0 / d1 < tau on 2-NN lists, counted per image into votes.
// img set: stacked lists [nq][2], counted at the first neighbour's image (ny = 1); img null: per-image lists [ny][nq][2].
hipError_t launch_coll_votes(const int32_t* img, const int32_t* idx, const float* dist, int64_t nq, int64_t ny, double tau,
                             unsigned long long* votes, hipStream_t stream);

// ---- api_pairs.hip ---------------------------------------------------------------------------------------------------------
// fm_collection_wide_votes, mode 1: the per-image 2-NN sweep of fm_collection_wide_knn2_each with the lists left on the device
// and tau's ratio test counted per image into votes [n_images] (host).  The caller has checked the handles, the kinds and the
// widths; n_images > 0 and q->n > 0.
int coll_wide_each_votes(fm_ctx* ctx, fm_collection* c, const fm_bank* q, double tau, int64_t* votes);
