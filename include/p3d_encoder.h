/* p3d_encoder.h — C ABI of the conditioning encoder (MI355X / gfx950): the layers of a torchvision ResNet v1.5 bottleneck network in
 * eval mode with its batch norms folded into the convolutions, the image front end of the reference's ResnetFeatureExtractor
 * (katebackbone.py:103-121) and the PCA projection of ResnetFeatureExtractorPCA (katepca.py:17-30) as one more 1 x 1 convolution.
 * Inference only: there is no backward.  The host composes them (panic3d_amd/encoder.py, ops.encoder_forward).
 *
 * Conventions of panic3d_hip.h: raw DEVICE pointers (unless said otherwise), the stream last, 0 / negative P3D_E_* / positive
 * hipError_t, no allocation, every argument checked before any launch.  Arithmetic: binary32 throughout; the convolutions' products on
 * v_mfma_f32_16x16x4_f32 (exact f32 products, a k-ordered f32 fma chain; no f16 operand mode, so no domain restriction).  Every sum is
 * taken in the fixed order written below and nothing is accumulated with atomics: every result is bitwise reproducible run to run for
 * the same sizes and the same plan.
 */
#ifndef P3D_ENCODER_H
#define P3D_ENCODER_H
#include "panic3d_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define P3D_ENC_KC 64          /* K is taken in chunks of 64 consecutive (tap, input channel) pairs; split-K cuts between chunks */
#define P3D_ENC_CUS 256        /* the workgroup count the plan aims for: one per compute unit */
#define P3D_ENC_TILE_64 1      /* plan tile: 64 output channels x 64 output pixels per workgroup */
#define P3D_ENC_TILE_32 2      /* plan tile: 32 output channels x 64 output pixels per workgroup */
#define P3D_ENC_MAX_SPLIT 255  /* a plan code is (tile << 8) | split */

#define P3D_ENC_RELU 1         /* flags of a convolution */

/* The plan of one convolution: a pure host function (csrc/p3d_encoder_plan.hpp), no GPU needed.
 *   P      = N Ho Wo output pixels, all samples flattened into one pixel axis (so that a batch of two 8 x 8 maps is 128 pixels, not
 *            two ragged tiles), K = k^2 Ci, chunks = ceil(K / 64)
 *   T(t)   = ceil(Co / t) ceil(P / 64) workgroups of tile t without a split
 * The rule, in this order:
 *   1. T(64) >= 256:                     tile 64, split 1;
 *   2. T(32) >= 256:                     tile 32, split 1   (a smaller tile before a split: no workspace traffic, one launch);
 *   3. T(64) chunks >= 256 (a split can reach 256):   tile 64, want = ceil(256 / T(64)) splits;
 *   4. otherwise                         tile 32, want = min(chunks, ceil(256 / T(32)));
 *   with a split: cps = max(1, floor(chunks / want)) chunks per split, split = ceil(chunks / cps) >= want (at most 255: cps grows
 *   until it is).
 * Hence T(tile) split >= 256 for every layer with T(32) chunks >= 256; a layer below that (its arithmetic has fewer than 256
 * tile-chunks of work) gets tile 32 and one chunk per split.
 * force_plan: 0 = choose; else (tile << 8) | want with tile in {1, 2} and 1 <= want <= 255, want clipped to chunks and turned into
 * (cps, split) as above.  out4 (HOST pointer, may be NULL) receives {tile (P3D_ENC_TILE_*), split, cps, workgroups of the
 * convolution launch}.  Returns the plan code (tile << 8) | split, or P3D_E_ARG / P3D_E_RANGE for sizes the convolution refuses. */
int p3d_enc_conv_plan(int N, int Ci, int Co, int Ho, int Wo, int k, int stride, int force_plan, int* out4);

/* Bytes of workspace the convolution needs under that plan: split > 1 ? split N Co Ho Wo sizeof(float) : 0 (0 also for refused sizes). */
size_t p3d_enc_conv_workspace_bytes(int N, int Ci, int Co, int Ho, int Wo, int k, int stride, int force_plan);

/* Convolution with folded batch norm: out = [relu]( corr(x, wk) + bias [+ res] ), NCHW binary32.
 *   z[n][co][oy][ox]   = sum over K = (t, ci), t = k ty + tx < k^2 outer, ci < Ci inner, of
 *                        x[n][ci][stride oy + ty - pad][stride ox + tx - pad] * wk[t][ci][co]          (outside the image: 0)
 *   out[n][co][oy][ox] = z + bias[co] (+ res[n][co][oy][ox]), then max(., 0) with P3D_ENC_RELU
 * x [N][Ci][H][W]; wk [k^2][Ci][Co] (the folded weight as weight.permute(2, 3, 1, 0)); bias [Co]; res NULL or [N][Co][Ho][Wo];
 * k in {1, 3, 7}, stride in {1, 2}, pad = (k - 1) / 2, Ho = (H + 2 pad - k) / stride + 1 (likewise Wo).  Any N, Ci, Co, H, W >= 1:
 * ragged edges are predicated, nothing is padded by the caller.
 * Order of the sum: split s takes the K indices [64 cps s, min(K, 64 cps (s + 1))) ascending as ONE fma chain that starts from 0
 * (v_mfma_f32_16x16x4_f32: acc = fma(x, w, acc) in k order).  split == 1: the chain's result is z.  split > 1: partial s goes to
 * workspace[s][n][co][oy][ox]; a second launch forms z = ((p_0 + p_1) + p_2) + ... ascending.  The bias, the residual and the ReLU
 * are applied once, after the reduction: (z + bias) + res, then the maximum.
 * workspace_bytes < p3d_enc_conv_workspace_bytes(...): P3D_E_WORKSPACE.  out must not alias x or res' storage partially (out == res
 * exactly is allowed: each value is read and written by the same lane). */
int p3d_enc_conv_f32(const float* x, int N, int Ci, int H, int W, const float* wk, int k, int stride, int Co, const float* bias,
                     const float* res, int flags, float* out, int force_plan, void* workspace, size_t workspace_bytes, void* stream);

/* 3 x 3 stride-2 maximum with padding 1 (torchvision's stem pool): x [planes][H][W] -> y [planes][Ho][Wo], Ho = (H - 1) / 2 + 1.
 * Padding cells never win: they count as -infinity, not as 0 (the window always holds at least one real cell). */
int p3d_enc_maxpool_f32(const float* x, int64_t planes, int H, int W, float* y, void* stream);

/* The front end, one launch.  img [N][C >= 3][H][W] in [0, 1], of which the first three channels are read; out [2N][3][h][w]:
 *   rows 0..N-1:   r = bilinear(img[n][c], y, x), align_corners = False, no antialiasing; out = (r - mean[c]) / std[c]
 *   rows N..2N-1:  the same of the horizontally mirrored image, img[n][c][y][W - 1 - x]    (katepca.py:22-25)
 * Bilinear: source coordinate sx = max(0, (x + 1/2) W / w - 1/2) as the exact rational (2x + 1) W - w over 2w; x0 = floor(sx),
 * x1 = min(x0 + 1, W - 1), l1 = frac(sx) and l0 = 1 - frac(sx), each rounded once from exact integers; likewise y.
 *   r = fma(ly1, fma(lx1, v11, lx0 v10), ly0 fma(lx1, v01, lx0 v00))            v_ab = img[..][y_a][x_b]
 * mean, std [3] DEVICE pointers.  (h, w) is the caller's: torchvision's Resize(int) makes the shorter side `size` and the longer one
 * int(size * long / short).  H, W, h, w < 2^22. */
int p3d_enc_prepare_f32(const float* img, int N, int C, int H, int W, const float* mean, const float* std3, int h, int w, float* out,
                        void* stream);

/* One layer of the whole network's table (HOST memory). */
#define P3D_ENC_KIND_CONV 0
#define P3D_ENC_KIND_MAXPOOL 1
#define P3D_ENC_KIND_PREPARE 2
typedef struct p3d_enc_layer {
    int32_t kind;            /* P3D_ENC_KIND_* */
    int32_t N, Ci, H, W;     /* the input: conv [N][Ci][H][W]; maxpool planes = N Ci; prepare img [N][Ci][H][W] */
    int32_t Co, Ho, Wo;      /* the output: conv [N][Co][Ho][Wo]; maxpool [N][Ci][Ho][Wo], Co = Ci; prepare [2N][3][Ho][Wo], Co = 3 */
    int32_t k, stride;       /* conv only (else 0) */
    int32_t in, out, res;    /* buffer indices into the arena; res = -1: none (conv only) */
    int32_t flags;           /* conv: P3D_ENC_RELU */
    int32_t plan;            /* conv: force_plan (0 = choose) */
    int32_t reserved;        /* 0 */
    int64_t w_off, b_off;    /* offsets in floats into the weight blob: conv wk and bias; prepare mean[3] and std[3] */
} p3d_enc_layer;

/* sizeof(p3d_enc_layer) and its field offsets in declaration order, for a binding that restates the struct (ctypes).  Returns the
 * number of values written, P3D_E_ARG / P3D_E_RANGE. */
int p3d_enc_struct_layout(size_t* out, int cap);

/* The whole network: walks `layers` (HOST, n_layers records) in order on one stream — one call, one launch per layer plus one per
 * split-K reduction; no graph capture.  Buffer b of the activation arena is arena[buf_off[b] .. buf_off[b] + buf_len[b]) in floats
 * (buf_off, buf_len: HOST arrays of n_bufs); weights: one DEVICE blob of weight_floats floats.
 * Checked before any launch, for every record: the kind; the sizes as the layer's own entry point checks them (and Co, Ho, Wo against
 * what the input sizes give); in / out / res in [0, n_bufs) (res may be -1), in != out; each buffer long enough for the tensor put
 * into it and inside the arena; w_off / b_off ranges inside the blob; the largest workspace any convolution needs against
 * workspace_bytes (P3D_E_WORKSPACE).  P3D_E_ARG for NULL pointers and counts <= 0, P3D_E_RANGE for everything else. */
int p3d_encoder_forward_f32(const p3d_enc_layer* layers, int n_layers, const float* weights, int64_t weight_floats, float* arena,
                            int64_t arena_floats, const int64_t* buf_off, const int64_t* buf_len, int n_bufs, void* workspace,
                            size_t workspace_bytes, void* stream);

/* Bytes of workspace p3d_encoder_forward_f32 needs for that table: the maximum over its convolutions (0 for a table it would refuse). */
size_t p3d_encoder_workspace_bytes(const p3d_enc_layer* layers, int n_layers);

#ifdef __cplusplus
}
#endif
#endif
