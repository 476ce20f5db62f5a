// The match graph's chunks (api_pairs.hip): which consecutive pairs of one call share a set of launches.
//
// A call's pairs are served in order.  A chunk is a run of consecutive pairs whose kernels run as one set of table-driven
// launches over one carve of the workspaces, so a chunk is closed in front of the pair that would take it over
//   * the byte budget (option "coll_ws_bytes"): partials, bounds, tie lists, the lists and the per-row arrays of its pairs,
//   * 2^31 - 1 workgroups of the sweep, blocks of the merge or blocks of the join (the grids are int32),
//   * 2^24 slots (the tables count slots in int32, two per pair), or
//   * 2^30 - 1 rows of a wide chunk's output-row space.
// A chunk holds at least one pair, whatever that pair costs in bytes; a single pair beyond the workgroup or the wide-row
// limit cannot be served and is reported with its index.  A pair with an empty side costs nothing and owns no slot.
// Plain arithmetic only, no HIP types: the host test compiles it on its own (tests/test_pairs_plan_host.py).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>

namespace fm {

constexpr int64_t kPairsMaxGrid = 0x7fffffff;
constexpr int64_t kPairsMaxSlots = 1 << 24;
constexpr int64_t kPairsMaxWideRows = 0x3fffffff;

// What one pair needs under its route (api_pairs.hip: pairs_cost_*).  All zero: a side of the pair has no rows.
struct PairsCost {
    size_t part = 0, bound = 0, fix = 0;       // bytes of its slots' partials, shared bounds and tie lists (wide: record lists)
    int64_t wg = 0, mblocks = 0, jblocks = 0;  // workgroups of its sweeps, blocks of its merges and of its join
    int64_t ra = 0, rb = 0;                    // rows of its two sides: the output rows of the forward and of the reverse slot
    int64_t wrows = 0;                         // wide: its share of the chunk's output-row space
    bool live() const { return ra > 0 && rb > 0; }
    // bytes against the budget: the above, 16 per list entry, 17 per row of a and 12 per block of the join
    size_t bytes() const { return live() ? part + bound + fix + (size_t)(ra + rb) * 16 + (size_t)ra * 17 + (size_t)jblocks * 12 : 0; }
};

// The pairs [p0, p1) and the sums of what their kernels cover.
struct PairsSpan {
    int64_t p0 = 0, p1 = 0;
    int nslots = 0;                            // sweeps (ndir per pair of non-empty images)
    int64_t wg = 0, mblocks = 0;               // workgroups of the table sweep, blocks of the merge
    int64_t jblocks = 0, entries = 0, lists = 0;      // blocks and per-row entries of the join, list entries
    size_t part = 0, bound = 0, fix = 0;       // bytes of the slots' partials, shared bounds and tie lists
    int64_t wrows = 0;                         // wide: the chunk's output-row space (every slot pad128 of its rows)
    double work = 0;                           // ndir * sum rows(a) rows(b)
};

enum PairsPlanStatus { kPairsPlanOk = 0, kPairsPlanWorkgroups = 1, kPairsPlanWideRows = 2 };

// The chunks of the n pairs c[0 .. n), appended to *out.  ndir: sweeps per live pair -- 2, or 1 for the forward lists alone
// (no join: such a pair has no per-row entries and lists only rows(a)).  Not kPairsPlanOk: *bad is the first pair that no
// chunk can hold, and the status says why.
inline PairsPlanStatus pairs_plan(const PairsCost* c, int64_t n, size_t budget, int ndir, std::vector<PairsSpan>* out, int64_t* bad)
{
    if (n <= 0) return kPairsPlanOk;
    PairsSpan ch;
    size_t used = 0;
    for (int64_t p = 0; p < n; ++p) {
        const PairsCost& k = c[p];
        const size_t need = k.bytes();
        const bool full = ch.p0 < p && (used + need > budget || ch.wg + k.wg > kPairsMaxGrid || ch.jblocks + k.jblocks > kPairsMaxGrid ||
                                        ch.mblocks + k.mblocks > kPairsMaxGrid || ch.nslots + 2 > kPairsMaxSlots ||
                                        ch.wrows + k.wrows > kPairsMaxWideRows);
        if (full) {
            ch.p1 = p;
            out->push_back(ch);
            ch = PairsSpan{};
            ch.p0 = p;
            used = 0;
        }
        if (k.wg > kPairsMaxGrid) { *bad = p; return kPairsPlanWorkgroups; }
        if (k.wrows > kPairsMaxWideRows) { *bad = p; return kPairsPlanWideRows; }
        used += need;
        if (!k.live()) continue;
        ch.nslots += ndir; ch.wg += k.wg; ch.mblocks += k.mblocks; ch.jblocks += k.jblocks;
        ch.entries += ndir == 1 ? 0 : k.ra;
        ch.lists += ndir == 1 ? k.ra : k.ra + k.rb;
        ch.part += k.part; ch.bound += k.bound; ch.fix += k.fix;
        ch.wrows += k.wrows;
        ch.work += (double)ndir * (double)k.ra * (double)k.rb;
    }
    ch.p1 = n;
    out->push_back(ch);
    return kPairsPlanOk;
}

}  // namespace fm
