// The ratio test's distance cut: the smallest integer d2 from which on no match can pass.
//
// The accepted-only calls keep a query row q with winner t iff  ratio = (double)sqrtf(d2) / selfdist[q] < tau  (float64,
// xcheck_finalize_kernel).  With sd_max = max over the query rows of selfdist[q] and
//   D* = the smallest integer d2 with  !((double)sqrtf((float)d2) / sd_max < tau),
// every d2 >= D* fails for EVERY query row (sqrtf and a correctly rounded division are monotone, selfdist[q] <= sd_max,
// selfdist[q] = 0 gives inf or NaN), so K1 may drop any candidate at d2 >= D* (the seeded sweep).
// Plain arithmetic only, no HIP types: the host test compiles it on its own (tests/test_ratio_cut.py).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FM_HD __host__ __device__
#else
#define FM_HD
#endif

namespace fm {

constexpr uint32_t kNoRatioCut = 0xffffffffu;     // no cut: every d2 may still pass

// d2 fails the ratio test against a query row whose self distance is sd_max (the largest one), in the arithmetic of
// xcheck_finalize_kernel: float32 root of the float32 image of d2, float64 division, strict "< tau".
FM_HD inline bool ratio_cut_fails(uint32_t d2, double sd_max, double tau)
{
    return !((double)sqrtf((float)d2) / sd_max < tau);
}

// D* for (sd_max, tau), or kNoRatioCut.  No cut for a NaN tau, and for an sd_max that is NaN, infinite or carries the sign
// bit (-0.0 and negative values come only from a caller's self distances; d / -0.0 = -inf passes any tau).  sd_max = +0
// and tau <= 0 let nothing pass: D* = 0.  Binary search over [0, 2^32): the failing set is an upward-closed range.
FM_HD inline uint32_t ratio_cut_d2(double sd_max, double tau)
{
    if (tau != tau || sd_max != sd_max || signbit(sd_max) || isinf(sd_max)) return kNoRatioCut;
    if (!ratio_cut_fails(0xffffffffu, sd_max, tau)) return kNoRatioCut;
    uint64_t lo = 0, hi = 0xffffffffull;          // fails(hi); D* in [lo, hi]
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (ratio_cut_fails((uint32_t)mid, sd_max, tau)) hi = mid;
        else lo = mid + 1;
    }
    return (uint32_t)lo;
}

}  // namespace fm
