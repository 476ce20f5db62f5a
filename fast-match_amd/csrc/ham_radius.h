// Hamming radiusMatch: what a float32 radius means for an integer distance, and for the matrix cores' dot product.
//
// Train row j is in query row i's list iff  (float)h(i, j) < r_i  (strict, float32; fm_radius_match's rule), h = popcount(q XOR t)
// an integer of [0, W], W = 8 * bytes <= 512 -- every h is exact in float32.  So the test is  h <= H_i  with
//   H_i = the largest integer of [0, W] with (float)H_i < r_i, or -1 where there is none (r <= 0, NaN).
// The sweep (radius_ham_kernel, radius.hip) never forms h in its test: the FP4 dot product of two encoded rows is
// dot = W - 2 h (hamming.hip), so  h <= H  <=>  dot >= W - 2 H; H = -1 gives +inf, which no dot product reaches.
// Plain arithmetic only, no HIP types: the host test compiles it on its own (tests/test_hamming_radius_host.py).
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FM_HR_HD __host__ __device__
#else
#define FM_HR_HD
#endif

namespace fm {

// H for radius r and W bits per row, in [-1, W].  r in (0, W]: an integer r = k admits k - 1, anything between k and k + 1
// admits k -- ceil(r) - 1 in both cases (a denormal: ceil = 1, H = 0); ceilf is exact, and r <= 512 fits an int.
FM_HR_HD inline int ham_radius_limit(float r, int W)
{
    if (!(r > 0.f)) return -1;                 // (NaN included)
    if (r > (float)W) return W;                // (+inf included)
    return (int)ceilf(r) - 1;
}

// The threshold on the accumulator: a pair is a hit iff dot >= the value returned here.
FM_HR_HD inline float ham_radius_dot_min(int H, int W)
{
    return H < 0 ? INFINITY : (float)(W - 2 * H);
}

// NORM_HAMMING2 (hamming2.hip): h2 counts the 2-bit cells that differ, an integer of [0, P], P = 4 * bytes <= 256 cells per row;
// the limit is ham_radius_limit(r, P), and the tetrahedral FP4 image gives dot = 3 P - 4 h2, so  h2 <= H  <=>  dot >= 3 P - 4 H.
FM_HR_HD inline float ham2_radius_dot_min(int H, int P)
{
    return H < 0 ? INFINITY : (float)(3 * P - 4 * H);
}

}  // namespace fm
