// p3d_cull_band.hpp — the band of raw sigma around the cull / binarize threshold inside which p3d_apply_masks (p3d_decode.hpp) still
// evaluates the contract's activation, and outside which it decides from sigma alone.  Host code only (no HIP headers):
// tests/test_cull_band_cpu.py compiles it into a plain host program.
//
// The decision is  a(s) < thresh  with the contract's  a(s) = 1 - exp_nonpos(-softplus(s - 1))  (include/p3d_numerics.h), an f32
// approximation of  A(s) = 1 / (1 + e^-(s - 1)).  a is not monotone in s as computed, so one compare against a critical sigma is not
// bit-identical.  But  |a(s) - A(s)| <= E  for every float s, and A is monotone, so with delta > E
//     s < s_lo = 1 + logit(thresh - delta)   =>   A(s) < thresh - delta   =>   a(s) < thresh
//     s > s_hi = 1 + logit(thresh + delta)   =>   A(s) > thresh + delta   =>   !(a(s) < thresh)
// and only sigma in [s_lo, s_hi] (or NaN) needs the full evaluation.
#pragma once
#include <math.h>

// E: the largest |a(s) - A(s)| of the sweep of tests/test_cull_band_cpu.py against the CPU oracle (every float within 2^21 floats of
// the band edges of six thresholds, every 2048th bit pattern of the whole range, the special values), measured 2026-10-19:
// E = 9.93e-8 (at thresh = 0.5, near s = 1; 7.8e-8 elsewhere).  E comes from a sweep, not from a proof, hence the margin:
// delta = 16 E.  The test fails when a later sweep finds E above delta / 8.
#define P3D_CULL_BAND_E 9.93e-8
#define P3D_CULL_BAND_DELTA (16.0 * P3D_CULL_BAND_E)  // 1.5888e-6: at thresh = 0.5 a band of 161 floats around s = 1

// 1 + logit(p) in double, rounded to float towards -inf (up = false) or +inf (up = true); -inf / +inf when p is not inside (0, 1)
// (a NaN threshold included): that side of the band is then open and the full evaluation runs.
static inline float p3d_cull_band_edge(double p, bool up) {
    if (!(p > 0.0 && p < 1.0)) return up ? INFINITY : -INFINITY;
    const double s = 1.0 + (log(p) - log1p(-p));
    float f = (float)s;
    if (up ? (double)f < s : (double)f > s) f = nextafterf(f, up ? INFINITY : -INFINITY);
    return f;
}

static inline void p3d_cull_band(float thresh, float* s_lo, float* s_hi) {
    *s_lo = p3d_cull_band_edge((double)thresh - P3D_CULL_BAND_DELTA, false);
    *s_hi = p3d_cull_band_edge((double)thresh + P3D_CULL_BAND_DELTA, true);
}
