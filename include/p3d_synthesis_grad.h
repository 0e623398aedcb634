/* p3d_synthesis_grad.h — C ABI of the backward pass of the synthesis network's layers (MI355X / gfx950).
 *
 * The pieces of the backward of one SynthesisLayer (modulated 3x3 convolution, plain or up-sampling, fused with noise, bias,
 * lrelu, gain and clamp: networks_stylegan2.py:299-360) and of one ToRGBLayer (1x1, :363-383).  The host composes them
 * (ops.modulated_conv2d / ops.torgb under autograd); the FIR adjoints of the up-sampling layers and of the skip
 * connection run on p3d_upfirdn2d_f32 with the flipped filter.
 *
 * Conventions of panic3d_hip.h: raw DEVICE pointers, the stream last, 0 / negative P3D_E_* / positive hipError_t, no allocation,
 * caller-owned workspace (size from the matching *_workspace_bytes query, 256-byte aligned), every argument checked before any
 * launch.  Arithmetic: binary32 operands, products on v_mfma_f32_16x16x4_f32 (exact f32 products, f32 accumulation); every sum is
 * taken in a fixed order (no atomics), so every result is bitwise reproducible run to run for the same sizes.
 */
#ifndef P3D_SYNTHESIS_GRAD_H
#define P3D_SYNTHESIS_GRAD_H
#include "panic3d_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Backward of y = clamp(act(z) * gain) (bias_act.py; the reference CUDA kernel's own rule): the mask comes from the OUTPUT y, so no
 * pre-activation is needed.  g_z = g_y * gain * (clamp < 0 || |y| < clamp) * (act == lrelu && y <= 0 ? alpha : 1).
 *   y, g_y [N][C][HW]; act 0 linear / 1 lrelu.
 * Outputs: g_out [N][C][HW] = g_z * dscale[n][c] (dscale NULL: 1; may alias g_y); g_bias_nc [N][C] = sum over HW of g_z (or NULL);
 *   g_noise [N][HW] = sum over C of g_z (or NULL). */
int p3d_bias_act_backward_f32(const float* y, const float* g_y, int N, int C, int64_t HW, int act, float alpha, float gain,
                              float clamp, const float* dscale, float* g_out, float* g_bias_nc, float* g_noise, void* stream);

/* Data gradient of a convolution as a strided correlation on the matrix cores:
 *   out[n][co][oy][ox] = sum over ci < Ci, t < taps of g[n][ci][stride*oy + ty - pad][stride*ox + tx - pad] * wk[t][ci][co]
 * (out-of-range positions read 0; t = 3 ty + tx for taps = 9, ty = tx = 0 for taps = 1).  g [N][Ci][Hi][Wi], wk [taps][Ci][Co],
 * out [N][Co][Ho][Wo].  Plain 3x3 layer: stride 1, pad 1, wk = the flipped weights; up-sampling layer (after the FIR adjoint):
 * stride 2, pad 0, wk = the weights as they are; 1x1: taps 1. */
int p3d_conv_dgrad_f32(const float* g, int N, int Ci, int Hi, int Wi, const float* wk, int taps, int Co, int Ho, int Wo, int stride,
                       int pad, float* out, void* stream);

/* Modulation backward: g_s[n][c] = sum over HW of x * g, then g <- g * s[n][c] in place.  x, g [N][C][HW]; s, g_s [N][C]. */
int p3d_mod_backward_f32(const float* x, const float* s, int N, int C, int64_t HW, float* g, float* g_s, void* stream);

/* Workspace of p3d_conv_wgrad_f32 (the split-K partial slabs and the per-sample sums). */
size_t p3d_conv_wgrad_workspace_bytes(int N, int O, int I, int taps, int Hd, int Wd);

/* Weight gradient, split-K over the pixels of each sample, slabs summed in a fixed order:
 *   dw[t][o][i] = sum over n, (py, px) < (Hd, Wd) of g[n][o][sg*py + ag*ty - pg][sg*px + ag*tx - pg]
 *                                                 * x[n][i][sx*py + ax*ty - px0][sx*px + ax*tx - px0] * s[n][i]
 * (out-of-range positions read 0).  g [N][O][Hg][Wg], x [N][I][Hx][Wx], s [N][I] or NULL (1).  Plain 3x3: the domain is the output
 * map, (sg, ag, pg) = (1, 0, 0), (sx, ax, px0) = (1, 1, 1); up-sampling (g = the FIR adjoint's [2H+1]^2 map): the domain is the
 * input map, (2, 1, 0) and (1, 0, 0); 1x1: taps 1.
 * g_d (optional, with wk [taps][O][I] and dscale [N][O]): g_d[n][o] = sum over t, i of wk[t][o][i] * dw_n[t][o][i] / dscale[n][o],
 * dw_n the sample's own part of dw — the gradient of the demodulation coefficients when g carries them as a factor. */
int p3d_conv_wgrad_f32(const float* g, int Hg, int Wg, int sg, int ag, int pg, const float* x, const float* s, int Hx, int Wx, int sx,
                       int ax, int px0, int N, int O, int I, int taps, int Hd, int Wd, float* dw, const float* wk, const float* dscale,
                       float* g_d, void* workspace, size_t workspace_bytes, void* stream);

/* Backward of a ToRGB layer whose channel sums came out of conv1's launch and were finished by p3d_torgb_combine_f32 — the
 * super-resolution blocks.  The pre-clamp value v is rebuilt from the same shares in the same order as the forward (tile 0, + tile 1,
 * ..., + bias[r]), so the clamp mask is the forward's own, bit for bit:
 *   g_y[n][r][y][x]    = g_img[n][r][y][x] * (clamp < 0 || |v| < clamp)
 *   g_bias[r]          = sum over n, pixels of g_y (or NULL: not computed)
 *   g_skip[n][r][u][v] = sum over fy, fx < 4 of skip_fir[fy][fx] * g_img[n][r][2u + 2 - fy][2v + 2 - fx] (out of range: 0) — the adjoint
 *                        of the forward's up-sampled skip image, skip_fir the forward's 4x4 filter (flipped, gain 4); NULL: not computed.
 * partial [tiles][N][R][H][W], bias [R] or NULL, g_img / g_y [N][R][H][W], g_skip [N][R][H/2][W/2] (H, W even). */
int p3d_torgb_combine_backward_f32(const float* partial, int tiles, int N, int R, int H, int W, const float* bias, float clamp,
                                   const float* g_img, float* g_y, float* g_bias, const float* skip_fir, float* g_skip, void* stream);

#ifdef __cplusplus
}
#endif
#endif
