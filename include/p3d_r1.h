/* p3d_r1.h — C ABI of the R1 penalty's device operators (MI355X / gfx950): what the second differentiation of the dual
 * discriminator adds to the first-order pieces of p3d_discriminator.h and p3d_synthesis_grad.h (ops.py's recorded backward,
 * DESIGN.md §4.21).
 *
 * Conventions of panic3d_hip.h: raw DEVICE pointers, the stream last, 0 / negative P3D_E_* / positive hipError_t, no allocation,
 * every argument checked before any launch.  Every sum is taken in a fixed order (no atomics), so every result is bitwise
 * reproducible run to run for the same sizes.
 */
#ifndef P3D_R1_H
#define P3D_R1_H
#include "panic3d_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The tangent layer of a convolution layer, in one launch: the layer's linear part applied to h, under the layer's bias_act mask,
 *   z[n][co][oy][ox]   = sum over t < taps, ci < Ci of h[n][ci][stride*oy + ty - pad][stride*ox + tx - pad] * wk[t][ci][co]
 *   out[n][co][oy][ox] = 0                                       where clamp >= 0 and not |pre| < clamp
 *                      = z * gain (* alpha where act == 1 and not pre > 0)      elsewhere
 * with pre[n][co][oy][ox] the layer's forward output before its residual — the rule and rounding order of
 * p3d_bias_act_backward_f32, on the sums of p3d_conv2d_act_f32 — products on v_mfma_f32_16x16x4_f32, the same tile loop: the result
 * equals, bit for bit, p3d_conv2d_act_f32 with act 0, no bias, gain 1, no clamp and no residual, followed by
 * p3d_bias_act_backward_f32.
 * h [N][Ci][Hi][Wi]; wk [taps][Ci][Co]; pre, out [N][Co][Ho][Wo] with Ho = (Hi + 2 pad - k) / stride + 1 (k = 3 for taps 9, 1 for
 * taps 1; likewise Wo), else P3D_E_RANGE.  taps 1 or 9, stride 1 or 2, pad 0..2, act 0 or 1.  out may alias pre. */
int p3d_conv2d_mask_f32(const float* h, int N, int Ci, int Hi, int Wi, const float* wk, int taps, int Co, int Ho, int Wo, int stride,
                        int pad, const float* pre, int act, float alpha, float gain, float clamp, float* out, void* stream);

/* The backward of p3d_mbstd_backward_f32: the double backward of the minibatch standard deviation.  Notation of p3d_discriminator.h:
 * G = min(group, N), M = N / G, c = C / F, E = c * HW, kE = 1 / (G * E); per (m, ch, p): mu the group's mean, d_g = x_g - mu,
 * sd = sqrt((sum over g of d_g^2) / G + 1e-8); gs[m][f] = the sum of g_extra over the group's samples and pixels (as in
 * p3d_mbstd_backward_f32, whose result is g_x_g = kE * gs * d_g / sd).  For a cotangent h of g_x, with hbar = (sum over g of h_g) / G
 * and s = sum over g of (h_g - hbar) * d_g (= sum h_g d_g: the differences are centred before they are multiplied):
 *   g_gextra[g*M + m][f][p] = kE * sum over the E values (ch, p) of f of s / sd              (one value per (m, f), broadcast)
 *   g_x2[g*M + m][ch][p]    = kE * gs * ((h_g - hbar) / sd - d_g * s / (G * sd^3))
 * x, h, g_x2 [N][C][HW]; g_extra as p3d_mbstd_backward_f32 takes it (first statistic channel of sample 0, g_extra_stride floats between
 * samples); g_gextra [N][F][HW].  The heavy cancellation in d, h - hbar and the bracket is why every per-value expression and both
 * sums (lane-strided, then a fixed tree) are evaluated in binary64 from the binary32 inputs and rounded once on the store.
 * One workgroup per (m, f). */
int p3d_mbstd_backward2_f32(const float* x, const float* g_extra, int64_t g_extra_stride, const float* h, int N, int C, int64_t HW,
                            int group, int F, float* g_gextra, float* g_x2, void* stream);

/* The R1 penalty: out[n] = sum over a[n][..] of a^2 + sum over b[n][..] of b^2, one workgroup per sample, both tensors in one launch:
 * binary64 lane-strided sums (a's values, then b's), a fixed tree, one rounding.  a [N][Ea]; b [N][Eb] or NULL with Eb = 0. */
int p3d_r1_sumsq_f32(const float* a, int64_t Ea, const float* b, int64_t Eb, int N, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
