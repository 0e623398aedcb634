/* p3d_loss.h — C ABI of the training loss's operators (MI355X / gfx950): the Gaussian blur in front of the discriminator
 * (loss_orthocondA.py:182-187, :222-226), the L1 image term, and the render-resolution terms of one supervised view
 * (:287-308, :351-375, :434-455, :540-561) with their gradients.
 *
 * Conventions of panic3d_hip.h: raw DEVICE pointers, the stream last, 0 / negative P3D_E_* / positive hipError_t, no allocation
 * (a caller-owned workspace, its size from the *_workspace_bytes query), every argument checked before any launch.  Arithmetic:
 * binary32; every sum is taken in a fixed order (no atomics), so every result is bitwise reproducible run to run for the same
 * sizes.
 */
#ifndef P3D_LOSS_H
#define P3D_LOSS_H
#include "panic3d_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define P3D_BLUR_MAX_TAPS 127

/* Separable "same"-size FIR with zero boundary, both passes in one launch (upfirdn2d.filter2d with a 1-D filter,
 * upfirdn2d.py:197-209: the row pass, then the column pass).  With R = (taps - 1) / 2:
 *   mid[y][x] = sum over t = 0 .. taps-1, ascending, of f[t] * X[y][x + t - R]
 *   out[y][x] = sum over t = 0 .. taps-1, ascending, of f[t] * mid[y + t - R][x]
 * X and mid read 0 outside [0,H) x [0,W); each sum is one fma chain from 0.  A correlation with f as given (pass the flipped filter
 * for a convolution; the adjoint of the operator is the operator with the flipped filter).  x, y [NC][H][W], f [taps];
 * taps odd, 1 <= taps <= P3D_BLUR_MAX_TAPS, else P3D_E_RANGE.  H and W may be smaller than R.  y must not alias x. */
int p3d_blur_f32(const float* x, int64_t NC, int H, int W, const float* f, int taps, float* y, void* stream);

/* sum[0] = sum over i < n of |a[i] - b[i]|: per-workgroup partials (each lane a strided chain, then a fixed tree) into the workspace,
 * then a fixed tree over the partials.  g_a (optional, [n]) = scale * sign(a[i] - b[i]) with sign(0) = 0 (torch's abs backward). */
size_t p3d_l1_workspace_bytes(int64_t n);
int p3d_l1_f32(const float* a, const float* b, int64_t n, float scale, float* sum, float* g_a, void* workspace, size_t workspace_bytes,
               void* stream);

#define P3D_DEPTH_Z 0    /* d = (xyz[2] - g[2])^2            (front and back views) */
#define P3D_DEPTH_X 1    /* d = (xyz[0] - g[0])^2            (left and right views) */
#define P3D_DEPTH_NORM 2 /* d = sqrt(sum_c (xyz[c] - g[c])^2) (random view, reconstruction) */

/* The render-resolution terms of one supervised view and their gradients in one launch.
 *   a, g   = the bilinear resizes of gt_alpha, gt_xyz from S to r (F.interpolate(mode='bilinear', align_corners=False), no
 *            antialias): src = (i + 0.5) * S / r - 0.5 clamped at 0, i0 = floor(src), i1 = min(i0 + 1, S - 1), l = src - i0,
 *            value = (1-ly) * ((1-lx) * v00 + lx * v01) + ly * ((1-lx) * v10 + lx * v11)
 *   box    = the zero-padded 5 x 5 sum of a (rows, then columns, ascending);  m = (|box / 25 - 0.5| * 2 > 0.5)
 *   mz     = m and (w > 0.5) and (a > 0.5)
 *   sums[0] = sum of (w - a)^2 * m * q          sums[1] = sum of d * mz * q       (d by depth_mode, above)
 *   g_weights = s_alpha * 2 (w - a) * m * q
 *   g_xyz[c]  = s_depth * dd/dxyz[c] * mz * q   (2 (xyz[c] - g[c]) on the one channel of the squared modes, 0 on the others;
 *                                                (xyz[c] - g[c]) / d in mode NORM)
 * The sums are over all N r^2 texels (the caller divides by N r^2, the reference's .mean()); the masks carry no gradient.  In mode
 * NORM a texel at distance exactly 0 gets gradient 0: the reference's autograd gives 0 * inf = NaN there (sqrt's backward at 0
 * times pow's backward 0), which this operator does not reproduce.
 * weights [N][1][r][r], xyz [N][3][r][r], gt_alpha [N][1][S][S], gt_xyz [N][3][S][S], q (optional texel weight) [N][1][r][r],
 * sums [2], g_weights [N][1][r][r] and g_xyz [N][3][r][r] (both optional: NULL under no_grad).  1 <= r <= S <= 16384, else
 * P3D_E_RANGE; depth_mode one of P3D_DEPTH_*, else P3D_E_RANGE. */
size_t p3d_view_terms_workspace_bytes(int N, int r);
int p3d_view_terms_f32(const float* weights, const float* xyz, const float* gt_alpha, const float* gt_xyz, const float* q, int N, int r,
                       int S, int depth_mode, float s_alpha, float s_depth, float* sums, float* g_weights, float* g_xyz,
                       void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
