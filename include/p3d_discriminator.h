/* p3d_discriminator.h — C ABI of the dual discriminator's layers (MI355X / gfx950): the forward of Conv2dLayer with its epilogue
 * (networks_stylegan2.py:141-189, after any resampling) and MinibatchStdLayer (:848-869) forward and backward.  The host composes
 * them with p3d_upfirdn2d_f32 (the down-sampling layers' FIR) and with the backward pieces of p3d_synthesis_grad.h
 * (ops.conv2d_act / ops.minibatch_std under autograd).
 *
 * Conventions of panic3d_hip.h: raw DEVICE pointers, the stream last, 0 / negative P3D_E_* / positive hipError_t, no allocation,
 * every argument checked before any launch.  Arithmetic: binary32 operands, products on v_mfma_f32_16x16x4_f32 (exact f32 products,
 * f32 accumulation); every sum is taken in a fixed order (no atomics), so every result is bitwise reproducible run to run for the
 * same sizes.
 */
#ifndef P3D_DISCRIMINATOR_H
#define P3D_DISCRIMINATOR_H
#include "panic3d_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Forward of a convolution layer with its epilogue in one launch:
 *   z[n][co][oy][ox]   = sum over t < taps, ci < Ci of x[n][ci][stride*oy + ty - pad][stride*ox + tx - pad] * wk[t][ci][co]
 *   pre                = clamp(act(z + bias[co]) * gain)          (act 0 linear / 1 lrelu with slope alpha; clamp < 0: none)
 *   out[n][co][oy][ox] = pre + res[n][co][oy][ox]                 (res NULL: pre)
 * (out-of-range positions read 0; t = 3 ty + tx for taps = 9, ty = tx = 0 for taps = 1: a correlation, the weights as they are.)
 * x [N][Ci][Hi][Wi]; wk [taps][Ci][Co] (the layer's weight * weight_gain, transposed); bias [Co] or NULL; res, out [N][Co][Ho][Wo]
 * with Ho = (Hi + 2 pad - k) / stride + 1, k = 3 for taps 9 and 1 for taps 1 (likewise Wo), else P3D_E_RANGE.  taps 1 or 9, stride 1
 * or 2, pad 0..2.  pre_out (optional, [N][Co][Ho][Wo]): the value before the residual, which is what p3d_bias_act_backward_f32 takes
 * its mask from; only a layer with a residual needs it.  out may alias res (each value is read, then written, by one lane). */
int p3d_conv2d_act_f32(const float* x, int N, int Ci, int Hi, int Wi, const float* wk, int taps, int Co, int Ho, int Wo, int stride,
                       int pad, const float* bias, int act, float alpha, float gain, float clamp, const float* res, float* pre_out,
                       float* out, void* stream);

/* Minibatch standard deviation.  G = min(group, N) must divide N and F must divide C; M = N / G groups, sample n = g * M + m belongs
 * to group m (the reference's reshape(G, -1, F, c, H, W)), c = C / F channels per statistic.
 *   mu[m][ch][p]  = (sum over g < G, in order, of x[g*M + m][ch][p]) / G
 *   sd[m][ch][p]  = sqrt((sum over g of (x - mu)^2) / G + 1e-8)
 *   stat[m][f]    = (sum over the c * HW values (ch in f*c .. f*c + c - 1, p) of sd, lane-strided then a fixed tree) / (c * HW)
 * x [N][C][HW].  y: concat != 0: [N][C + F][HW], channels < C copied from x and channel C + f of every sample of group m = stat[m][f];
 * concat == 0: [N][F][HW], the statistic channels alone.  sd [M][C][HW]: kept for the backward.  One workgroup per (m, f). */
int p3d_mbstd_f32(const float* x, int N, int C, int64_t HW, int group, int F, int concat, float* y, float* sd, void* stream);

/* Backward of the statistic channels: with gs[m][f] = sum over g < G (in order), p < HW (lane-strided, fixed tree) of
 * g_extra[g*M + m][f][p],
 *   g_x[g*M + m][ch][p] = gs[m][f] * (x[g*M + m][ch][p] - mu[m][ch][p]) / (G * sd[m][ch][p] * c * HW)
 * — the statistic's contribution to the gradient of x (the caller adds the cotangent of the copied channels).  g_extra points at the
 * first statistic channel of sample 0 and g_extra_stride is the distance in floats between samples (F * HW for a tensor of its own,
 * (C + F) * HW inside the concatenated cotangent).  x, g_x [N][C][HW]; sd from the forward. */
int p3d_mbstd_backward_f32(const float* x, const float* sd, const float* g_extra, int64_t g_extra_stride, int N, int C, int64_t HW,
                           int group, int F, float* g_x, void* stream);

#ifdef __cplusplus
}
#endif
#endif
