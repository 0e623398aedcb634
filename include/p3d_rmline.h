/* p3d_rmline.h — C ABI of the illustration-to-render module (MI355X / gfx950): the Difference-of-Gaussians line mask of the reference's
 * RMLineWrapper (rmline_wrapper.py:15-50, sketchers_v2.py:64-83) and the layers of its generator (rmlineganA.py:57-143), a stack of
 * UNPADDED 3 x 3 convolutions in eval mode with the batch norms folded into the next convolution.  Inference only: there is no backward.
 * The host composes them (panic3d_amd/rmline.py, ops.rmline_*).
 *
 * Conventions of panic3d_hip.h: raw DEVICE pointers (unless said otherwise), the stream last, 0 / negative P3D_E_* / positive
 * hipError_t, no allocation, every argument checked before any launch.  Arithmetic: binary32 throughout; the convolutions' products on
 * v_mfma_f32_16x16x4_f32 (exact f32 products, a k-ordered f32 fma chain).  Every sum is taken in the fixed order written below and
 * nothing is accumulated with atomics: every result is bitwise reproducible run to run, and under either plan.
 */
#ifndef P3D_RMLINE_H
#define P3D_RMLINE_H
#include "panic3d_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define P3D_RMLINE_MAX_TAPS 33   /* the most taps of either Gaussian (k1 <= 33: sigma k kernel_factor < 17); more: P3D_E_RANGE */
#define P3D_RMLINE_MAX_DILATE 8  /* the largest structuring element d x d */
#define P3D_RMLINE_MAX_C 64      /* a layer's Ci and Co */

/* The parameters of the line detector (HOST memory).  Doubles, so that the tap counts come out as Python's do:
 *   k0 = max(2 int(sigma kernel_factor) + 1, 3), k1 = max(2 int(sigma k kernel_factor) + 1, 3)        (sketchers_v2.py:72-73)
 * Weights of a blur with `taps` taps and deviation s: exp(-x^2 / (2 s^2)) for x = -(taps/2) .. taps/2 in double, divided by their sum
 * (ascending), rounded once to binary32. */
typedef struct p3d_rmline_dog {
    double t, sigma, k, epsilon, kernel_factor;   /* the wrapper's: 1, 0.5, 1.6, 0.01, 4 (5 and 7 taps) */
    int32_t d;                                    /* the dilation's d x d element, 1 <= d <= 8 (the wrapper's: 2); 1 = none */
    int32_t reserved;                             /* 0 */
} p3d_rmline_dog;

/* The tap counts of those parameters: out2 (HOST) = {k0, k1}.  P3D_E_ARG for a NULL pointer or non-finite / non-positive sigma, k,
 * kernel_factor; P3D_E_RANGE for k1 or k0 > P3D_RMLINE_MAX_TAPS, k1 < k0 (k < 1: the halo is the second blur's), d outside 1..8,
 * reserved != 0. */
int p3d_rmline_dog_taps(const p3d_rmline_dog* dog, int* out2);

/* The line mask, ONE launch: composite, grey, both blurs, threshold, dilation and hull clearing per 8 x 32 tile with a halo of
 * k1/2 + d - 1 in LDS; no intermediate image reaches memory.
 *   img [N][C][H][W], C in {1, 3, 4}.   C = 4: c_j = (img_j a) + (1 - a), a = img_3 (white background), else c_j = img_j.
 *   grey  = c_0 for C = 1, else (0.299 c_0 + 0.587 c_1) + 0.114 c_2                       (kornia.color.rgb_to_grayscale)
 *   g_b   = vertical blur of the horizontal blur of grey with weights w_b, b in {0, 1}; coordinates clamped to the image (replicate
 *           border); each blur one fma chain from 0 over its taps ascending: acc = fma(w[i], v[x + i - taps/2], acc)
 *   resp  = min(max((0.5 + t (g_1 - g_0)) - epsilon, 0), 1)                               (batch_dog with clip=True)
 *   line  = resp > 0.5;  dil[y][x] = any line[y - d/2 .. y + d - 1 - d/2][x - d/2 .. x + d - 1 - d/2] inside the image
 *           (kornia 0.6.5's dilation by ones(d, d): origin d / 2, geodesic border)
 *   mask  = dil and not (hull != 0), as 0.f / 1.f
 * hull NULL or [N][1][H][W]; mask [N][1][H][W]; image NULL or [N][3][H][W]: receives c (C >= 3 only; else P3D_E_ARG when given);
 * response NULL or [N][1][H][W]: receives resp (for tests).  H, W <= 32768. */
int p3d_rmline_mask_f32(const float* img, int N, int C, int H, int W, const float* hull, const p3d_rmline_dog* dog, float* mask,
                        float* image, float* response, void* stream);

/* Activations of a layer's store. */
#define P3D_RMLINE_ACT_NONE 0
#define P3D_RMLINE_ACT_LEAKY 1   /* v > 0 ? v : v * slope */
#define P3D_RMLINE_ACT_TANH 2    /* tanhf */

/* The plan of a layer: the pixel tile of a workgroup (256 lanes, four waves, each a strip of the tile's rows x 32 columns).  A pure host
 * function (csrc/p3d_rmline_plan.hpp).  The tile's input patch and the workgroup's weights live in LDS together:
 *   bytes(rows) = 4 (Ci4 + 2) ((rows + 2) 34 + 9 CoT),   Ci4 = 4 ceil(Ci / 4), CoT = min(32, 16 ceil(Co / 16))
 * plan 0 chooses P3D_RMLINE_TILE_8 when bytes(8) <= 160 KiB, else P3D_RMLINE_TILE_4; a forced plan that does not fit is P3D_E_RANGE.
 * Either plan gives the same bits: a value's sum does not depend on the tile.  out3 (HOST, may be NULL) = {rows, CoT, LDS bytes}.
 * Returns the plan chosen (1 or 2) or P3D_E_*. */
#define P3D_RMLINE_TILE_8 1
#define P3D_RMLINE_TILE_4 2
int p3d_rmline_conv_plan(int Ci, int Co, int force_plan, int* out3);

#define P3D_RMLINE_IN_STACK 1    /* flags of a layer: the input is built from image / mask / hull (below) */
#define P3D_RMLINE_OUT_PLANAR 2  /* the output is [N][Co][Ho][Wo], not channel-last */
#define P3D_RMLINE_OUT_LERP 4    /* with OUT_PLANAR: out = lerp(image, act(z), mask) */
#define P3D_RMLINE_IN_NO_MASK 8  /* with IN_STACK: the image is NOT multiplied by 1 - mask although a mask is given (for OUT_LERP) */
#define P3D_RMLINE_SUM_PER_TAP 32 /* z's sum as nine chains, one per tap over ci from 0, added in tap order: no chain longer than Ci (training; other bits) */

/* One UNPADDED 3 x 3 convolution of an input of Hin x Win pixels: Ho = Hin - 2, Wo = Win - 2 (Hin, Win >= 3) and
 *   z[n][oy][ox][co] = (sum over K = (tap t = 3 ty + tx outer, ci inner) ascending of in[n][oy + ty][ox + tx][ci] wk[t][ci][co]) + bias[co]
 * the sum ONE fma chain from 0 on the matrix cores (zero operands pad Ci to a multiple of 4: they leave the chain's value as it is),
 * the bias added once after it, then the activation.
 *   wk [9][Ci][Co] (the weight as weight.permute(2, 3, 1, 0)); bias [Co]; 1 <= Ci, Co <= P3D_RMLINE_MAX_C.
 * Input, without P3D_RMLINE_IN_STACK: x [N][Hin][Win][Ci] channel-last; pad must be 0; hull is ignored.
 * With it: the reference's `stackin` (rmlineganA.py:117-130) is built in the load and never stored.  With H = Hin - 2 pad >= 1 and
 * W = Win - 2 pad >= 1, pad >= 0: image [N][3][H][W], mask NULL or [N][1][H][W], hull NULL or [N][1][H][W]; Ci = 3 + (hull != NULL);
 *   in[n][y][x][c] = image[n][c][cy][cx] * (1 - mask[n][0][cy][cx])  (c < 3; without mask: image itself),  in[..][3] = hull[n][0][cy][cx]
 *   with cy = clamp(y - pad, 0, H - 1), cx = clamp(x - pad, 0, W - 1)       (replicate padding as a coordinate clamp);  x is ignored.
 * Output, without P3D_RMLINE_OUT_PLANAR: out [N][Ho][Wo][Co] = act(z).  With it: out [N][Co][Ho][Wo] = act(z); with OUT_LERP also
 * (needs OUT_PLANAR, Co = 3, image [N][3][Ho][Wo] and mask [N][1][Ho][Wo]; together with IN_STACK hence pad = 1):
 *   out = w < 0.5 ? a + w (b - a) : b - (b - a) (1 - w),   a = image, b = act(z), w = mask     (torch.lerp; w = 0 gives a's bits)
 * act: P3D_RMLINE_ACT_*; slope: LeakyReLU's.  N Hin Win max(Ci, Co) < 2^31, N <= 65535.
 * Alignment: a channel-last tensor whose channel count is a multiple of 4 moves in 16-byte vectors, so x (Ci % 4 == 0) and a
 * channel-last out (Co % 4 == 0) must be 16-byte aligned: P3D_E_ARG otherwise. */
int p3d_rmline_conv_f32(const float* x, const float* image, const float* mask, const float* hull, int N, int Hin, int Win, int pad, int Ci,
                        const float* wk, const float* bias, int Co, int act, float slope, int flags, int force_plan, float* out,
                        void* stream);

/* One layer of the generator's table (HOST memory). */
typedef struct p3d_rmline_layer {
    int32_t Ci, Co;          /* the first layer's Ci is 3, or 4: then it reads hull, which must be given */
    int32_t act;             /* P3D_RMLINE_ACT_* */
    int32_t plan;            /* force_plan (0 = choose) */
    float slope;             /* LeakyReLU's */
    int32_t reserved;        /* 0 */
    int64_t w_off, b_off;    /* offsets in floats into the weight blob: wk [9][Ci][Co] and bias [Co] */
} p3d_rmline_layer;

/* sizeof and field offsets in declaration order: which = 0 p3d_rmline_dog, 1 p3d_rmline_layer.  Returns the number of values written. */
int p3d_rmline_struct_layout(int which, size_t* out, int cap);

#define P3D_RMLINE_FWD_MASK_INPUT 1   /* flags of the walk: the first layer multiplies the image by 1 - mask (gen_mask_input) */
#define P3D_RMLINE_FWD_LERP 2         /* the last layer stores lerp(image, out, mask) (the wrapper); needs pad == n_layers */

/* The whole module in ONE call: [the mask kernel,] then every layer of `layers` (HOST, n_layers records) on one stream: n_layers (+ 1)
 * launches.  The first layer loads with P3D_RMLINE_IN_STACK, the last stores with P3D_RMLINE_OUT_PLANAR (one layer: both).
 *   dog != NULL: img [N][C][H][W], C in {1, 3, 4} goes through p3d_rmline_mask_f32, which WRITES mask [N][1][H][W] and, for C = 4, image
 *                [N][3][H][W] (C = 3: the layers read img itself and image may be NULL; C = 1: P3D_E_RANGE, the generator wants colour).
 *   dog == NULL: C must be 3, img is the image and mask is an INPUT (NULL allowed without MASK_INPUT and LERP).
 *   hull NULL or [N][1][H][W]: cleared from the mask (dog) and the fourth input channel of the first layer.
 *   pad >= 0: the replicate padding of the first layer's input; the output is [N][Co_last][Ho][Wo], Ho = H + 2 pad - 2 n_layers >= 1.
 *   act0, act1: two channel-last activation buffers of act_floats floats each, used alternately (unused for n_layers = 1): each must
 *               hold the largest intermediate, N (H + 2 pad - 2) (W + 2 pad - 2) max Co.  Both 16-byte aligned (P3D_E_ARG otherwise).
 * launches (HOST, may be NULL) receives the number of kernels started.  Checked before any launch: every record as
 * p3d_rmline_conv_f32 checks it, Ci of a layer against Co of the one before, offsets against weight_floats, the buffers' size. */
int p3d_rmline_forward_f32(const float* img, int N, int C, int H, int W, const float* hull, const p3d_rmline_dog* dog,
                           const p3d_rmline_layer* layers, int n_layers, const float* weights, int64_t weight_floats, int pad, int flags,
                           float* image, float* mask, float* act0, float* act1, int64_t act_floats, float* out, int* launches,
                           void* stream);

#ifdef __cplusplus
}
#endif
#endif
