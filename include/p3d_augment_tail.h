/* p3d_augment_tail.h — C ABI of the augmentation pipe's tail (MI355X / gfx950): ADA's image-space filter, additive noise and cutout
 * (training/augment.py:382-437 of the reference) as one operator of the image, and its adjoint.
 *
 * Conventions of panic3d_hip.h: raw DEVICE pointers, the stream last, 0 / negative P3D_E_* / positive hipError_t, no allocation and
 * no workspace, every argument checked before any launch.  Arithmetic: binary32, every sum a fixed-order fma chain from 0 (no
 * atomics): results are bitwise reproducible.
 *
 * The operator, for x [N][C][H][W]; every stage is optional (its pointers NULL), and with all three absent the call is a copy:
 *   1. filter (taps [N][K], K odd, 1 <= K <= P3D_TAIL_MAX_TAPS, R = K / 2, h_n = taps[n]): a separable correlation on the image
 *      reflected without edge repeat, refl(q) = -q for q < 0, 2 (W - 1) - q for q >= W:
 *        rows first:    t[i][j] = sum over k = 0 .. K - 1 ascending of h_n[k] x[i][refl(j + k - R)]
 *        then columns:  f[i][j] = sum over k = 0 .. K - 1 ascending of h_n[k] t[refl(i + k - R)][j]
 *      each sum an fma chain from 0 in that order.  R < min(H, W), else P3D_E_RANGE: a reflect index is not checked again.
 *   2. noise (z [N][C][H][W], sigma [N], both or neither): v = fma(sigma_n, z, f).
 *   3. cutout (rect [N][4] int32 = x0, x1, y0, y1): y = 0 where x0 <= j < x1 and y0 <= i < y1, else v.  A select, not a product:
 *      the reference multiplies by a 0 / 1 mask, so a non-finite v under the rectangle is NaN there and 0 here.  The rectangle
 *      may be empty or reach beyond the image; the kernel only compares.
 * The longest rounding chain of an output is 2 K + 1 (K = 1 without a filter).
 *
 * The adjoint, gx = Fr^T Fc^T (mask . g), has no noise term (z and sigma do not enter it).  Each 1-D adjoint is the transposed
 * correlation onto the padded axis, P[q] = sum over k ascending with 0 <= q - k + R < n of h_n[k] m[q - k + R] for -R <= q < n + R,
 * followed by the reflect fold as a sum over a source pixel's images in the order itself, left, right:
 *   a[i] = P[i]  (+ P[-i] when 1 <= i <= R)  (+ P[2 (n - 1) - i] when n - 1 - R <= i <= n - 2)
 * columns first (n = H), then rows (n = W).  At n = R + 1 every interior pixel has both images.  The longest rounding chain of an
 * output is 2 (K + 2).  One launch: the masked cotangent with its R-wide halo and the column pass's result stay in LDS.
 */
#ifndef P3D_AUGMENT_TAIL_H
#define P3D_AUGMENT_TAIL_H
#include "panic3d_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define P3D_TAIL_MAX_TAPS 63
#define P3D_TAIL_TILE_W 64     /* tile width: one wave of lanes along x */
#define P3D_TAIL_MAX_SIDE 32768
#define P3D_TAIL_LDS_BYTES 81920 /* what one workgroup may take: two fit a CU's 160 KiB */

/* out [4] = { the forward's tile height for K taps, its dynamic LDS bytes, the adjoint's tile height, its dynamic LDS bytes }: the
 * tallest of 64, 32, 16 rows whose footprint stays within P3D_TAIL_LDS_BYTES.  K = 0: no filter (no LDS, out = 0). */
int p3d_augment_tail_plan(int K, int* out, int out_len);

/* taps NULL <=> K == 0.  y must not be x. */
int p3d_augment_tail_f32(const float* x, const float* taps, int K, const float* z, const float* sigma, const int* rect, int N, int C,
                         int H, int W, float* y, void* stream);

int p3d_augment_tail_adjoint_f32(const float* g, const float* taps, int K, const int* rect, int N, int C, int H, int W, float* gx,
                                 void* stream);

#ifdef __cplusplus
}
#endif
#endif
