/* p3d_rmline_grad.h — C ABI of the illustration-to-render module's TRAINING operators (MI355X / gfx950): what one optimiser step of the
 * reference's rmlineganA model (rmlineganA.py:57-298) needs beyond the forward layer of p3d_rmline.h — batch statistics, the fold of a
 * train-mode batch norm into the next convolution, the data gradient, the weight / bias gradient, the batch norm's backward coefficients
 * and the head (lerp, L1, their backward).  The host composes them (rmline_train.py, ops.rmline_*).
 *
 * Conventions of p3d_rmline.h: raw DEVICE pointers, the stream last, 0 / negative P3D_E_* / positive hipError_t, no allocation (the
 * caller passes every workspace), every argument checked before any launch, activations channel-last [N][H][W][C].  Arithmetic:
 * binary32 throughout (the reference trains under Lightning's precision=16; that is NOT reproduced); convolution products on
 * v_mfma_f32_16x16x4_f32.  Every sum runs in the fixed order written below, nothing is accumulated with atomics, nothing synchronises
 * with the host: every result is bitwise reproducible run to run.
 */
#ifndef P3D_RMLINE_GRAD_H
#define P3D_RMLINE_GRAD_H
#include "p3d_rmline.h"

#ifdef __cplusplus
extern "C" {
#endif

#define P3D_RMLINE_BN_MAX_GROUPS 256  /* the most workgroups of the statistics' first launch */
#define P3D_RMLINE_BN_ROWS 256        /* a workgroup takes at least this many rows */
#define P3D_RMLINE_WG_MAX_SLICES 512  /* the most slices of a weight gradient */

/* ---- batch statistics -----------------------------------------------------------------------------------------------------------------
 * Per-channel mean and BIASED variance of x [K][C] (a channel-last activation, K = N H W rows), 1 <= C <= 64, by a CENTRED algorithm,
 * TWO launches.  G = min(P3D_RMLINE_BN_MAX_GROUPS, ceil(K / P3D_RMLINE_BN_ROWS)) workgroups take the rows [g K / G, (g + 1) K / G); in
 * a workgroup, part q of 4 takes the rows r0 + q, r0 + q + 4, ...: hi = their ascending sum divided by their count n; a second pass
 * takes res = the ascending sum of (x - hi) and of its square; lo = res / n, M2 = that sum - res lo.  The mean is carried as hi + lo
 * so that no merge sees a mean rounded to binary32.  Parts merge in q order, then the workgroups' moments in g order, by
 *   n = na + nb, d = (hib - hia) + (lob - loa), mean = meana + d nb / n (two-sum into hi, lo), M2 = M2a + M2b + d d na nb / n   (Chan et al.)
 * mean [C] = hi + lo, var [C] = M2 / K.  With running_mean (then running_var and counter too; all or none):
 *   running <- (1 - momentum) running + momentum batch, the variance UNBIASED (M2 / (K - 1)); *counter (int64) += 1.
 * ws: P3D_RMLINE_BN_MAX_GROUPS * 4 * 64 floats at least (ws_floats says how many).  K = 1: P3D_E_RANGE (torch raises there). */
int p3d_rmline_bn_stats_f32(const float* x, int64_t K, int C, float momentum, float* mean, float* var, float* running_mean,
                            float* running_var, int64_t* counter, float* ws, int64_t ws_floats, void* stream);

/* ---- the fold -------------------------------------------------------------------------------------------------------------------------
 * A layer's operands from its parameters, ONE launch.  w [Co][Ci][3][3] (torch's layout), bias [Co]:
 *   gamma == NULL:  wk[t][ci][co] = w[co][ci][t], bias_f = bias                                              (a re-layout only)
 *   else, with the batch norm IN FRONT of this convolution (gamma, beta, mean, var [Ci], its eps):
 *     r = 1 / sqrtf(var + eps), s = gamma r, sh = beta - mean s;  wk[t][ci][co] = w s[ci];
 *     bias_f[co] = bias[co] + (the sum over (t outer, ci inner) ascending of w[co][ci][t] sh[ci], compensated: Dot2 in binary32 — an error
 *     of the folded bias would shift every pixel of the layer alike)
 * exact for this network because the batch norm follows the activation and nothing pads with zeros.  wk [9][Ci][Co], bias_f [Co]. */
int p3d_rmline_bn_fold_f32(const float* w, const float* bias, const float* gamma, const float* beta, const float* mean, const float* var,
                           float eps, int Ci, int Co, float* wk, float* bias_f, void* stream);

/* ---- the data gradient ----------------------------------------------------------------------------------------------------------------
 * The full correlation of g [N][Hg][Wg][Co] with a layer's own wk [9][Ci][Co]: Ho = Hg + 2, Wo = Wg + 2 and
 *   dx[n][y][x][ci] = sum over taps t' = 8 - t ascending of (sum over co ascending of g[n][y - ty][x - tx][co] wk[t][ci][co])
 * each tap's sum ONE fma chain from 0 on the matrix cores, the nine tap sums added in order from 0; g outside its map is zero in the load (never a padded copy); the weights are transposed and
 * tap-flipped while they are staged.  The tile loop is the forward's (csrc/p3d_rmline_tile.hpp).  The store:
 *   a == NULL:  out = dx
 *   else:       out = fma(c1[ci], a[n][y][x][ci], dx + c0[ci]) (a > 0 ? 1 : slope)     a [N][Ho][Wo][Ci]; c0, c1 [Ci] or both NULL (= 0)
 * the batch norm's two statistic terms and LeakyReLU's derivative (the sign of a is its pre-activation's for slope > 0; a = 0 takes
 * the slope, as torch does).  slope <= 0 or not finite with a: P3D_E_ARG.
 * out [N][Ho][Wo][Ci], or with P3D_RMLINE_OUT_PLANAR [N][Ci][Ho][Wo].  1 <= Ci, Co <= 64; g (Co % 4 == 0), a and a channel-last out
 * (Ci % 4 == 0) 16-byte aligned: P3D_E_ARG otherwise. */
int p3d_rmline_conv_dgrad_f32(const float* g, int N, int Hg, int Wg, int Co, const float* wk, int Ci, const float* a, const float* c0,
                              const float* c1, float slope, int flags, float* out, void* stream);

/* ---- the weight / bias gradient -------------------------------------------------------------------------------------------------------
 * The plan (a pure host function, csrc/p3d_rmline_grad_plan.hpp): the N patches are split into `slices` runs of consecutive patches,
 * slice s = [floor(s N / slices), floor((s + 1) N / slices)), one workgroup each.  force_slices 0 chooses min(N,
 * P3D_RMLINE_WG_MAX_SLICES); 1 <= force_slices <= min(N, P3D_RMLINE_WG_MAX_SLICES) is taken as given, anything else P3D_E_RANGE.
 * out4 (HOST, may be NULL) = {slices, accumulator sets per wave (1 or 4), LDS bytes, workspace floats}.  Returns slices or P3D_E_*. */
int p3d_rmline_wgrad_plan(int N, int Ci, int Co, int force_slices, int64_t* out4);

/* dwk[t][ci][co] = sum over (n, oy, ox) of in[n][oy + ty][ox + tx][ci] dz[n][oy][ox][co],  dbias[co] = sum of dz[n][oy][ox][co]
 * TWO launches.  in: as p3d_rmline_conv_f32 takes it (x channel-last, or with P3D_RMLINE_IN_STACK the stack of image / mask / hull
 * built in the load, P3D_RMLINE_IN_NO_MASK as there); dz [N][Hin - 2][Win - 2][Co].  Two levels, so that no chain is longer than a
 * tile row: the 32 pixels of a row of an 8 x 32-pixel tile are ONE fma chain from 0 on the matrix cores (ascending); a slice's partial
 * adds those row sums from 0 in the order patches ascending, a patch's tiles row-major, a tile's rows ascending; the second launch
 * adds the slices' partials in slice order from 0.  dbias, whose terms cancel, is COMPENSATED instead: lane part q of 4 adds the rows
 * q, q + 4, ... of every dz tile (pixels ascending) with a two-sum into a (sum, correction) pair, the parts' pairs merge in q order,
 * the slices' pairs in slice order, and sum + correction is rounded once at the end.  P3D_RMLINE_OUT_OIHW stores dw as
 * [Co][Ci][3][3] (torch's layout) instead of [9][Ci][Co].  ws: out4[3] floats of the plan, slices (9 Ci Co + 2 Co). */
#define P3D_RMLINE_OUT_OIHW 16
int p3d_rmline_conv_wgrad_f32(const float* x, const float* image, const float* mask, const float* hull, int N, int Hin, int Win, int pad,
                              int Ci, const float* dz, int Co, int flags, int force_slices, float* dw, float* dbias, float* ws,
                              int64_t ws_floats, void* stream);

/* ---- the batch norm's backward coefficients -------------------------------------------------------------------------------------------
 * ONE launch, per channel ci of the batch norm in front of a folded layer.  dwk_f [9][Ci][Co], db_f [Co]: the gradients of the FOLDED
 * operands; w [Co][Ci][3][3] the raw weight; gamma, beta, mean, var [Ci], eps; K the count of the statistics.  r, s, sh as in the fold:
 *   ds = sum over (t outer, co inner) of dwk_f w;   dt = sum over (t outer, co inner) of db_f[co] w     (both compensated: Dot2 in binary32,
 *   because ds - mean dt cancels)
 *   dgamma = (ds - mean dt) r;  dbeta = dt;  dw[co][ci][t] = dwk_f[t][ci][co] s[ci] + db_f[co] sh[ci]   (the folded weight AND the folded
 *   bias hold w; torch's layout; NULL: not wanted, like dgamma / dbeta)
 *   c1' = ((ds gamma - dt mean gamma) (-0.5 r^3)) / K;   c0 = -(s dt) / K - 2 mean c1';   c1 = 2 c1'
 * c0, c1 [Ci] are what the data gradient's store adds: the batch norm's backward costs no pass over the activations. */
int p3d_rmline_bn_coef_f32(const float* dwk_f, const float* db_f, const float* w, const float* gamma, const float* beta, const float* mean,
                           const float* var, float eps, int64_t K, int Ci, int Co, float* dgamma, float* dbeta, float* dw, float* c0, float* c1, void* stream);

/* ---- the head -------------------------------------------------------------------------------------------------------------------------
 * Forward, ONE launch, one workgroup per patch.  t, image [N][3][H][W], mask [N][1][H][W]:
 *   img = torch.lerp(image, t, mask)  (both branches, as P3D_RMLINE_OUT_LERP);  loss_l1[n] = (sum of |img - image|) / (3 H W)
 * the sum: lane l of 256 adds its elements l, l + 256, ... ascending from 0, then a binary tree over the lanes (stride 128, 64, ..., 1).
 * crop > 0: the centre window also goes to crop_img [N][3][Hc][Wc] (Hc = H - 2 crop) and hull's to crop_hull [N][1][Hc][Wc] (hull and
 * crop_hull may both be NULL) — the discriminator's input (F.pad by a negative amount). */
int p3d_rmline_head_f32(const float* t, const float* image, const float* mask, const float* hull, int N, int H, int W, int crop,
                        float* img, float* loss_l1, float* crop_img, float* crop_hull, void* stream);

/* Backward, ONE launch.  out [N][H][W][3] (channel-last: the last layer's pre-activation gradient is a weight gradient's dz) =
 *   f m (g_l1[n] sign(img - image) / (3 H W) + d[n][c][y - crop][x - crop] inside the centre window, 0 outside)
 *   f = fma(-t, t, 1) with t given, else 1;  m = mask, or 1 without;  sign(0) = 0 as torch's abs has it;  g_l1 [N] (NULL: no L1 term; then img
 *   and image are not read)
 * d is read with ELEMENT strides ds4 (HOST) = {n, c, y, x}, so that a gradient autograd hands over in any layout needs no copy; d NULL:
 * no such term.  mask = 0 gives exactly 0. */
int p3d_rmline_head_grad_f32(const float* t, const float* img, const float* image, const float* mask, const float* g_l1, const float* d,
                             const int64_t* ds4, int N, int H, int W, int crop, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
