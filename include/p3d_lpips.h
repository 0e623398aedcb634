/* p3d_lpips.h — C ABI of LPIPS, the AlexNet perceptual distance (MI355X / gfx950): the layers of lpips.LPIPS(net='alex', version 0.1,
 * lpips=True, spatial=False) as the reference's trainer builds it (_util/pytorch_v1.py:159-168, training_loop_v0.py:168), forward and
 * the gradient with respect to the first image.  The host composes them (panic3d_amd/lpips.py, ops.lpips_distance).
 *
 * Conventions of panic3d_hip.h: raw DEVICE pointers, the stream last, 0 / negative P3D_E_* / positive hipError_t, no allocation,
 * every argument checked before any launch.  Arithmetic: binary32 throughout; the convolutions' products on v_mfma_f32_16x16x4_f32
 * (exact f32 products, a k-ordered f32 fma chain).  Every sum is taken in the fixed order written below, there are no float atomics:
 * every result is bitwise reproducible run to run for the same sizes.
 *
 * The distance of x0 (may carry a gradient) and x1 (the target), both [N][3][H][W], H, W >= 31:
 *   s(x)[c] = (x[c] - shift[c]) / scale[c]          shift = (-.030, -.088, -.188), scale = (.458, .448, .450); a true division;
 *                                                    zero padding applies to s(x), not to x
 *   z_l = corr(in_l, W_l) + b_l,  a_l = max(z_l, 0)  l = 1..5, (k, stride, pad) = (11,4,2), (5,1,2), (3,1,1), (3,1,1), (3,1,1),
 *                                                    widths (64, 192, 384, 256, 256)
 *   in_1 = s(x), in_2 = pool(a_1), in_3 = pool(a_2), in_4 = a_3, in_5 = a_4;  pool: 3 x 3 maximum, stride 2, no padding, floor mode
 *   r = sqrt(sum_c a^2),  n = a / (r + 1e-10),  d_l[n][p] = sum_c lin_l[c] (n0 - n1)^2,  v_l[n] = mean_p d_l,  out[n] = sum_l v_l
 * (the sums over l in the order 1..5).  Both images of a pair go through one launch of every trunk layer (batch 2N: they share the
 * weights).
 */
#ifndef P3D_LPIPS_H
#define P3D_LPIPS_H
#include "panic3d_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define P3D_LPIPS_MAX_K 11        /* largest kernel size of a convolution */
#define P3D_LPIPS_MAX_STRIDE 4    /* largest stride */
#define P3D_LPIPS_BWD_MAX_CI 4    /* a strided layer's backward (the stem) keeps one accumulator per input channel in registers */
#define P3D_LPIPS_EPS 1e-10f      /* the head's epsilon */

/* Convolution + bias + ReLU in one launch, optionally with the scaling layer applied as the input is read:
 *   in[n][ci][y][x]     = scale ? (x[n][ci][y][x] - shift[ci]) / scale[ci] : x[n][ci][y][x]      (outside the image: 0)
 *   z[n][co][oy][ox]    = sum over K = (t, ci), t = k ty + tx < k^2 outer, ci < Ci inner, in that order, of
 *                         in[n][ci][stride oy + ty - pad][stride ox + tx - pad] * wk[t][ci][co]
 *   out[n][co][oy][ox]  = max(z + bias[co], 0)
 * An implicit GEMM: 64 output channels x 64 output pixels per workgroup, K taken in chunks of 64 consecutive (t, ci) pairs (so a
 * 3-channel stem fills its chunks with pairs, not with padding) and inside a chunk in k order on v_mfma_f32_16x16x4_f32: one
 * k-ordered fma chain per value, whatever the chunk size.
 * x [N][Ci][Hi][Wi]; wk [k^2][Ci][Co] (the layer's weight as weight.permute(2, 3, 1, 0)); bias [Co]; shift, scale [Ci], both or
 * neither; out [N][Co][Ho][Wo] with Ho = (Hi + 2 pad - k) / stride + 1 >= 1 (likewise Wo), else P3D_E_RANGE.  1 <= k <= 11,
 * 1 <= stride <= 4, 0 <= pad < k. */
int p3d_lpips_conv_relu_f32(const float* x, int N, int Ci, int Hi, int Wi, const float* wk, int k, int Co, int Ho, int Wo, int stride,
                            int pad, const float* bias, const float* shift, const float* scale, float* out, void* stream);

/* Data gradient of that layer.  With the cotangent of the pre-activation
 *   gz[n][co][oy][ox] = a[n][co][oy][ox] > 0 ? g_in[...] + g_head[...] : 0     (a pointer that is NULL contributes 0; not both)
 * (a: the layer's stored OUTPUT; g_in: what the following layer or pool sent back; g_head: the head's cotangent of this layer;
 * a NULL: the cotangent is taken as it is, gz = g_in + g_head — what p3d_lpips_head_backward_f32 leaves with relu_mask is masked already),
 *   gx[n][ci][y][x] = (sum over t, co of gz[n][co][(y + pad - ty) / stride][(x + pad - tx) / stride] * wk[t][ci][co]) (/ scale[ci])
 * over the taps whose quotient is exact and inside the output.
 *   stride == 1: the same implicit GEMM as the forward, a correlation of gz with the flipped, transposed weights and pad' = k - 1 - pad:
 *                wkb [k^2][Co][Ci], wkb[t][co][ci] = wk[k^2 - 1 - t][ci][co]; K = (t, co) in the forward's order and chunks.
 *   stride  > 1: (the stem) wkb = wk itself, [k^2][Ci][Co], Ci <= P3D_LPIPS_BWD_MAX_CI.  A gather on the vector unit: one workgroup
 *                per 256 input pixels of ONE phase ((y + pad) mod stride, (x + pad) mod stride), which visits only that phase's
 *                ceil or floor (k / stride) taps per axis — never a zero-interleaved cotangent; the phase's weights are staged in LDS
 *                64 output channels at a time.  Order: channel blocks of 64 ascending, inside a block ty ascending, tx ascending, co
 *                ascending.  scale (NULL or [Ci]): the scaling layer's division, last.
 * Rows and columns of x that no window reads get exactly 0.  g_in, g_head, a [N][Co][Ho][Wo]; gx [N][Ci][Hi][Wi]; the sizes are tied
 * as in the forward. */
int p3d_lpips_conv_relu_backward_f32(const float* g_in, const float* g_head, const float* a, int N, int Co, int Ho, int Wo,
                                     const float* wkb, int k, int Ci, int Hi, int Wi, int stride, int pad, const float* scale,
                                     float* gx, void* stream);

/* 3 x 3 stride-2 maximum, no padding, floor mode: x [planes][H][W] -> y [planes][Ho][Wo], Ho = (H - 3) / 2 + 1; H, W >= 3. */
int p3d_lpips_pool_f32(const float* x, int64_t planes, int H, int W, float* y, void* stream);

/* Its backward, as a gather: gx[y][x] = sum over the (at most 2 x 2) windows (oy, ox) that hold (y, x), oy ascending then ox
 * ascending, of g[oy][ox] where (y, x) is the FIRST maximum of that window in row-major scan order (recomputed from x: no index
 * tensor), else 0.  x, gx [planes][H][W]; g [planes][Ho][Wo].  Rows and columns outside every window (even H or W) get 0. */
int p3d_lpips_pool_backward_f32(const float* x, const float* g, int64_t planes, int H, int W, float* gx, void* stream);

/* Bytes of workspace the head's forward needs for N samples of HW pixels (the per-pixel distances d). */
size_t p3d_lpips_head_workspace_bytes(int N, int64_t HW);

/* The head of one layer.  a0, a1 [N][C][HW] (features of x0 and of x1), lin [C]:
 *   r0[p] = sqrt(sum_c a0^2), r1 likewise;  d[n][p] = sum_c lin[c] (a0 / (r0 + eps) - a1 / (r1 + eps))^2;  v[n] = (sum_p d) / HW
 * Sums over c: four partial sums, quarter q over the channels c = q, q + 4, ... ascending, then ((q0 + q1) + q2) + q3.  Sum over p:
 * 256 lane-strided partial sums (p = lane, lane + 256, ... ascending), then a fixed binary tree.
 * v [N]: always written.  out (optional, [N]): accumulate == 0: out[n] = v[n]; else out[n] = out[n] + v[n] — the calls of the five
 * layers in the order 1..5 on one stream leave the distance there. */
int p3d_lpips_head_f32(const float* a0, const float* a1, const float* lin, int N, int C, int64_t HW, float* v, float* out,
                       int accumulate, void* workspace, size_t workspace_bytes, void* stream);

/* Its backward with respect to a0.  g [N]: the cotangent of out.  With u_c = 2 lin[c] (n0_c - n1_c) (g[n] / HW):
 *   g_a0[n][c][p] = u_c / (r0 + eps) - a0_c (sum_j u_j a0_j) / (r0 (r0 + eps)^2);   a pixel with r0 == 0 gets 0
 * (torch produces NaN there and the ReLU's backward then selects 0: the same outcome; this form is finite throughout).  The sums
 * over channels in the forward's order.  Optionally the kernel finishes the cotangent of the layer's pre-activation in the same
 * pass, so that the layer's backward reads one tensor, not three: g_add (NULL or [N][C][HW], what the following layer or pool sent
 * back) is added, g_add + g_a0, and with relu_mask != 0 the sum is kept only where a0 > 0 (else 0). */
int p3d_lpips_head_backward_f32(const float* a0, const float* a1, const float* lin, const float* g, int N, int C, int64_t HW,
                                const float* g_add, int relu_mask, float* g_a0, void* stream);

#ifdef __cplusplus
}
#endif
#endif
