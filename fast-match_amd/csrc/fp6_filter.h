// The accepted-only sweep's FP6 filter (filter6.hip): code table, accumulator scaling and the static threshold.
//
// The accepted-only calls can only report candidates at d2 <= D* - 1 (ratio_cut.h).  The filter sweeps the pair on the FP6
// matrix cores (v_mfma_scale_f32_16x16x128_f8f6f4, e2m3 operands, unit scales) over a lossy image of the RAW uint8 rows and
// keeps every (output row, 32-row unit) that may hold such a candidate; the exact arithmetic is redone on the kept units
// only.  With c, m the uint8 rows and c^, m^ their images (value = 32 x the e2m3 value, below):
//   d2 <= D* - 1   <=>   c.m - |m|^2 / 2  >=  (|c|^2 - D* + 1) / 2
//   |c.m - c^.m^| = |(c - c^).m + c^.(m - m^)|  <=  E_c = ||c - c^|| max_m ||m||  +  ||c^|| max_m ||m - m^||      (Cauchy-Schwarz)
// so every such candidate has  c^.m^ - |m|^2 / 2  >=  T_c = (|c|^2 - D* + 1) / 2 - E_c.
//
// The accumulator is exact in any summation order.  An e2m3 magnitude is a multiple of 1/8 up to 7.5, so every product is
// a multiple of 1/64 (one "step") up to 56.25 = 3600 steps, a row's 128 products sum to at most 460 800 steps, and the
// accumulator starts at -floor(|m|^2 / 32) steps (|m|^2 <= 128 x 255^2: at most 260 100 steps).  Every term and every
// partial sum is an integer number of steps of magnitude below 2^20 < 2^24: float32 holds each of them exactly whatever the
// order of the additions.  One step is 1024 / 64 = 16 units of c^.m^; the start value rounds |m|^2 / 2 DOWN to a step, so
// the accumulator is never below (c^.m^ - |m|^2 / 2) / 1024 and the test  acc >= T_c / 1024  (threshold rounded down to a
// float) keeps every candidate the inequality above keeps.  The sweep adds the start value LAST, and only where a block
// passes a screen that needs no start (fp6_screen_threshold below): products summed from zero are the same integers of steps,
// so acc + start is the same float32, bit for bit.
// Plain arithmetic only, no HIP types: the host test compiles it on its own (tests/test_fp6_filter.py).
#pragma once
#include "ratio_cut.h"

namespace fm {

// e2m3 code (2 exponent bits, 3 mantissa bits, sign bit clear) -> 32 x its value: 0 .. 28 step 4 (subnormals), 32 .. 60
// step 4, 64 .. 120 step 8, 128 .. 240 step 16
FM_HD inline int fp6_value32(int code)
{
    const int e = (code >> 3) & 3, mant = code & 7;
    return e == 0 ? 4 * mant : (8 + mant) << (e + 1);
}

// uint8 value -> the code of the nearest representable value of v / 32 (the lower one of two equally near; values above
// 240 clamp to 7.5).  The codes are ascending in value, so the scan stops at the first one that is not nearer.
FM_HD inline int fp6_code(int v)
{
    int best = 0, err = v;
    for (int c = 1; c < 32; ++c) {
        const int x = fp6_value32(c), e = x > v ? x - v : v - x;
        if (e < err) { best = c; err = e; }
    }
    return best;
}

// accumulator start of a streamed row with squared norm usq (raw uint8 values): -floor(usq / 32) steps of 1/64
FM_HD inline float fp6_acc_init(int usq) { return -(float)(usq >> 5) * (1.0f / 64.0f); }
constexpr float kFp6PadInit = -3.4e38f;        // padding rows: below every threshold
constexpr float kF6Never = 3.0e38f;            // threshold of an output row beyond the bank: no accumulator reaches it

// E_c of an output row (squared norms of its image and of its error) against a streamed bank (largest squared row norm,
// largest squared error norm), rounded UP: the float64 roots and products are correct to 1 part in 2^50, the margin is 2^-20
// relative + 2^-10 absolute.
FM_HD inline double fp6_error_bound(int hatsq_c, int errsq_c, int usq_max_m, int errsq_max_m)
{
    const double e = sqrt((double)errsq_c) * sqrt((double)usq_max_m) + sqrt((double)hatsq_c) * sqrt((double)errsq_max_m);
    return e * (1.0 + 1.0 / 1048576.0) + 1.0 / 1024.0;
}

// T_c in units of c^.m^, rounded down to an integer (float64: every term is below 2^33)
FM_HD inline double fp6_threshold(int usq_c, int hatsq_c, int errsq_c, int usq_max_m, int errsq_max_m, uint32_t dstar)
{
    return floor(((double)usq_c - (double)dstar + 1.0) * 0.5 - fp6_error_bound(hatsq_c, errsq_c, usq_max_m, errsq_max_m));
}

// the same as the accumulator sees it: T_c / 1024 rounded DOWN to a float32
FM_HD inline float fp6_threshold_acc(double t)
{
    const double x = t * (1.0 / 1024.0);
    float f = (float)x;
    if ((double)f > x) f = nextafterf(f, -INFINITY);
    return f;
}

// The sweep's screen (filter6.hip).  Its accumulators start at zero, so they lack the streamed row's start value; a block
// is first tested against  thr_s = thr - smax, smax the LARGEST start among the real rows of the streamed stage (the word
// prep6_kernel leaves behind the stage's starts; kFp6PadInit for a stage without a real row).  With start(m) <= smax:
//   acc + start(m) >= thr   =>   acc >= thr - start(m) >= thr - smax >= thr_s       (acc + start(m) is exact, see above)
// so a lane that the exact test keeps always passes the screen, provided thr_s is rounded DOWN: the largest float32 not
// above thr - smax.  The operands are finite and never both huge with one sign except Never - PadInit, which rounds down to
// the largest finite float: no infinity, no NaN.  On the device the subtraction runs under the round-down mode; on the host
// the rounding error of the nearest result is recovered exactly (Knuth's two-sum) and a result above the difference steps down.
FM_HD inline float fp6_screen_threshold(float thr, float smax)
{
#if defined(__HIP_DEVICE_COMPILE__)
    // (bits 1:0 of the MODE register: the float32 rounding, 2 = towards -infinity, 0 = nearest even, the kernel's own.  One
    // statement, so that nothing else runs under the mode; two writes of one hardware register stand two states apart)
    float d;
    asm("s_setreg_imm32_b32 hwreg(HW_REG_MODE, 0, 2), 2\n\t"
        "v_sub_f32 %0, %1, %2\n\t"
        "s_nop 1\n\t"
        "s_setreg_imm32_b32 hwreg(HW_REG_MODE, 0, 2), 0\n\t"
        "s_nop 1" : "=v"(d) : "v"(thr), "v"(smax));
    return d;
#else
    const volatile float s = thr - smax;
    if (isinf(s)) return s > 0.f ? 3.402823466e38f : s;
    const volatile float bb = s - thr;
    const volatile float ra = thr - (s - bb), rb = -smax - bb;
    const float err = ra + rb;                  // thr - smax = s + err exactly
    return err < 0.f ? nextafterf(s, -INFINITY) : s;
#endif
}

}  // namespace fm
