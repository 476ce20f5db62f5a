// K12 -- how the FP6 filter sweep (filter6.hip) splits the streamed banks of one launch.
//
// A workgroup of the filter fills a CU, so a launch runs in rounds of R workgroups (R = the device's CUs).  A workgroup that
// streams L stages (128 rows each) costs L + P stage-times: P is what it pays around its stage loop -- the stationary
// operand, the thresholds, the presets of its key slices, the first two stages' latency, the flush of its records
// (profiles/k12_wg_overhead.log fits P = 1.5).  One stage count L serves the whole launch: pair i, with chunks_i workgroups
// per split and stages_i stages, gets ceil(stages_i / L) splits, and the launch costs
//     ceil(sum_i chunks_i * ceil(stages_i / L) / R) * (L + P)
// stage-times; L in [8, largest stages_i] minimises it, ties go to the larger L (fewer workgroups).  A pair below 8 stages
// then has one split.  The sum is a step function of L that only falls where some ceil(stages_i / L) does, and on a step the
// cost grows with L: only the first L of every step is tried.
// Plain arithmetic only, no HIP types: the host test compiles it on its own (tests/test_fp6_plan_host.py).
#pragma once
#include <stdint.h>

namespace fm {

constexpr int    kFp6PlanMinStages = 8;
constexpr double kFp6PlanOverhead  = 1.5;      // P, in stage-times

struct Fp6PlanPair {
    int chunks;       // the filter's workgroups per split: ceil(K1 chunks / 2)
    int stages;       // stages of the streamed bank
};

inline int64_t fp6_plan_ceil(int64_t a, int64_t b) { return (a + b - 1) / b; }

// workgroups of the launch at L stages per workgroup
inline int64_t fp6_plan_workgroups(const Fp6PlanPair* p, int n, int L)
{
    int64_t w = 0;
    for (int i = 0; i < n; ++i)
        if (p[i].chunks > 0 && p[i].stages > 0) w += (int64_t)p[i].chunks * fp6_plan_ceil(p[i].stages, L);
    return w;
}

inline int64_t fp6_plan_rounds(const Fp6PlanPair* p, int n, int resident, int L)
{
    return fp6_plan_ceil(fp6_plan_workgroups(p, n, L), resident > 0 ? resident : 1);
}

inline double fp6_plan_cost(const Fp6PlanPair* p, int n, int resident, double overhead, int L)
{
    return (double)fp6_plan_rounds(p, n, resident, L) * ((double)L + overhead);
}

// the launch's L
inline int fp6_plan_stages(const Fp6PlanPair* p, int n, int resident, double overhead)
{
    int lmax = kFp6PlanMinStages;
    for (int i = 0; i < n; ++i) if (p[i].stages > lmax) lmax = p[i].stages;
    int best = kFp6PlanMinStages;
    double best_cost = fp6_plan_cost(p, n, resident, overhead, best);
    for (int L = kFp6PlanMinStages; L < lmax;) {
        // the next L at which some pair loses a split: the first L with ceil(stages / L) = q - 1 is ceil(stages / (q - 1))
        int next = lmax;
        for (int i = 0; i < n; ++i) {
            const int64_t q = fp6_plan_ceil(p[i].stages, L);
            if (p[i].stages <= 0 || q <= 1) continue;
            const int64_t l1 = fp6_plan_ceil(p[i].stages, q - 1);
            if (l1 < next) next = (int)l1;
        }
        L = next;
        const double c = fp6_plan_cost(p, n, resident, overhead, L);
        if (c <= best_cost) { best_cost = c; best = L; }
    }
    return best;
}

// a pair's share: K1's normalisation of (stages per split, splits) -- the last split is never empty
inline void fp6_plan_split(int stages, int L, int* nsplit, int* per)
{
    if (stages < 1) { *nsplit = 1; *per = 1; return; }
    if (L < 1) L = 1;
    const int64_t n0 = fp6_plan_ceil(stages, L);
    const int64_t pr = fp6_plan_ceil(stages, n0);
    *per = (int)pr;
    *nsplit = (int)fp6_plan_ceil(stages, pr);
}

// from a forced split count (option "fp6_nsplit"), as K1's plan treats a forced "nsplit": clamped to the stages there are
inline void fp6_plan_split_forced(int stages, int force, int* nsplit, int* per)
{
    if (stages < 1) { *nsplit = 1; *per = 1; return; }
    if (force > stages) force = stages;
    if (force < 1) force = 1;
    const int64_t pr = fp6_plan_ceil(stages, force);
    *per = (int)pr;
    *nsplit = (int)fp6_plan_ceil(stages, pr);
}

}  // namespace fm
