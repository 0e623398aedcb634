/* p3d_clip.h — C ABI of the 2-D evaluation metrics that were missing (MI355X / gfx950): CLIP's ViT-B/32 image tower (clip/model.py's
 * VisionTransformer: patch embedding, class token, positional embedding, ln_pre, pre-norm residual blocks of multi-head attention and a
 * QuickGELU MLP, ln_post, projection), clip's image front end (_transform: PIL's 8-bit bicubic resize, centre crop, normalisation), the
 * cosine of measure.py:42, and the three reductions of PSNR.  Inference only: there is no backward.  The host composes them
 * (panic3d_amd/clip.py, ops.clip_forward).
 *
 * Conventions of panic3d_hip.h: raw DEVICE pointers (unless said otherwise), the stream last, 0 / negative P3D_E_* / positive
 * hipError_t, no allocation, every argument checked before any launch.  Arithmetic: binary32 throughout (the reference runs clip in
 * float16 on CUDA, because clip.load converts the weights; this is NOT reproduced); the GEMM's products on v_mfma_f32_16x16x4_f32 (exact
 * f32 products, a k-ordered f32 fma chain).  Every sum is taken in the fixed order written below and nothing is accumulated with
 * atomics: every result is bitwise reproducible run to run for the same sizes and the same plan.
 *
 * Activations are token-major: [M][D] with M = N T rows, T = 1 + (image / patch)^2 tokens per image.  Weights are stored once, at load
 * time, in the order the consuming kernel reads them: [K][Nout] (a torch Linear's weight transposed).
 *
 * "The wave tree" below: lane l of a 64-lane wave adds its elements l, l + 64, l + 128, ... ascending into one accumulator that starts
 * from 0; then six butterfly steps v = v + v(lane ^ o) for o = 32, 16, 8, 4, 2, 1 (addition commutes, so every lane ends with the same
 * bits).
 */
#ifndef P3D_CLIP_H
#define P3D_CLIP_H
#include "panic3d_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define P3D_CLIP_KC 64          /* K is taken in chunks of 64; split-K cuts between chunks */
#define P3D_CLIP_CUS 256        /* the workgroup count the plan aims for: one per compute unit */
#define P3D_CLIP_TILE_64 1      /* plan tile: 64 rows x 64 output columns per workgroup */
#define P3D_CLIP_TILE_32 2      /* plan tile: 32 rows x 64 output columns per workgroup */
#define P3D_CLIP_MAX_SPLIT 255  /* a plan code is (tile << 8) | split */
#define P3D_CLIP_XCDS 8         /* workgroups that share a weight slab are dealt to the same XCD (see p3d_clip_gemm_f32) */

#define P3D_CLIP_GELU 1         /* flags of the GEMM: QuickGELU */
#define P3D_CLIP_PATCH 2        /* flags of the GEMM: A is an NCHW image read as flattened patches */

#define P3D_CLIP_HEAD_DIM 64    /* the attention's head dimension, the only one */
#define P3D_CLIP_MAX_T 64       /* the attention's largest token count */
#define P3D_CLIP_MAX_SIDE 16384 /* the front end's largest source side */
#define P3D_CLIP_MAX_S 4096     /* the front end's largest output side */

/* ---- 1. the front end ------------------------------------------------------------------------------------------------------------
 * clip's _transform(S) of the tensor measure.py hands it: quantise, Resize(S, BICUBIC), CenterCrop(S), ToTensor, Normalize.
 *   quantise   q = floor(min(max(x, 0), 1) * 255) in binary32 (to_pil_image of x.clamp(0, 1): byte(x * 255)); NaN counts as 0
 *   resize     the shorter side becomes S, the longer one int(S long / short); PIL's 8-bit resample, integer arithmetic: a horizontal
 *              pass, then a vertical pass over its uint8 result.  One axis, in -> out, coefficient table built on the HOST in double:
 *                scale = in / out, fs = max(scale, 1), support = 2 fs, ksize = 2 ceil(support) + 1
 *                center = (xx + 0.5) scale, xmin = max(int(center - support + 0.5), 0), xmax = min(int(center + support + 0.5), in)
 *                w[x] = cubic((x + xmin - center + 0.5) / fs), x < xmax - xmin, divided by their sum (added ascending)
 *                cubic (a = -0.5): ((a + 2)|t| - (a + 3)) t^2 + 1 for |t| < 1, (((|t| - 5)|t| + 8)|t| - 4) a for |t| < 2, else 0
 *                k[x] = int(w 2^22 + 0.5) for w >= 0, int(w 2^22 - 0.5) for w < 0 (int truncates)
 *              each output value: clip8((2^21 + sum k[x] pixel[xmin + x]) >> 22), an arithmetic shift
 *   crop       offset int(round((size - S) / 2.0)) on each axis, round half to even (Python's round)
 *   normalise  (v / 255 - mean[c]) / std[c], two IEEE divisions, mean (0.48145466, 0.4578275, 0.40821073), std (0.26862954,
 *              0.26130258, 0.27577711) rounded to binary32
 * Built as TWO launches through a uint8 workspace [N][3][row_hi - row_lo][S]: only the source rows the kept output rows read and only
 * the kept columns are computed by the horizontal pass.
 *
 * p3d_clip_resize_plan (host only): out8 (HOST) = {h, w (the resized size), offy, offx (the crop), ksy, ksx (the tables' ksize),
 * row_lo, row_hi (the source rows the vertical pass reads)}.  H, W in [1, 16384], S in [1, 4096].
 * p3d_clip_resize_table (host only): the table of outputs first .. first + count - 1 of one axis into tab (HOST, count (2 + ksize)
 * int32): per output {xmin, n = xmax - xmin, k[0 .. ksize)} with k[x >= n] = 0.  ksize must be the plan's. */
int p3d_clip_resize_plan(int H, int W, int S, int* out8);
int p3d_clip_resize_table(int in, int out, int first, int count, int ksize, int32_t* tab);
size_t p3d_clip_prepare_workspace_bytes(int N, int H, int W, int S);
/* img [N][C >= 3][H][W] (channels beyond the third are ignored); tabx / taby: DEVICE copies of the tables of the S kept columns / rows
 * (p3d_clip_resize_table(W, w, offx, S, ksx) and (H, h, offy, S, ksy)); out [N][3][S][S].  The kernels clamp every table entry to the
 * image, so a wrong table gives wrong pixels, never an access outside img or the workspace. */
int p3d_clip_prepare_f32(const float* img, int N, int C, int H, int W, int S, const int32_t* tabx, const int32_t* taby, float* out,
                         void* workspace, size_t workspace_bytes, void* stream);

/* ---- 2. the GEMM -----------------------------------------------------------------------------------------------------------------
 * The plan: a pure host function (csrc/p3d_clip_plan.hpp).  chunks = ceil(K / 64), T(t) = ceil(M / t) ceil(Nout / 64) workgroups of
 * tile t without a split.  The rule, in this order (p3d_enc_conv_plan's):
 *   1. T(64) >= 256: tile 64, split 1;   2. T(32) >= 256: tile 32, split 1 (a smaller tile before a split);
 *   3. T(64) chunks >= 256: tile 64, want = ceil(256 / T(64)) splits;   4. otherwise tile 32, want = min(chunks, ceil(256 / T(32)));
 *   with a split: cps = max(1, floor(chunks / want)) chunks per split, split = ceil(chunks / cps) (at most 255: cps grows until it is).
 * Hence T(tile) split >= 256 wherever T(32) chunks >= 256.  force_plan: 0 = choose; else (tile << 8) | want, tile in {1, 2},
 * 1 <= want <= 255, want clipped to chunks.  out4 (HOST, may be NULL): {tile, split, cps, working workgroups}.  Returns the plan code
 * (tile << 8) | split, or P3D_E_ARG / P3D_E_RANGE.  M K, M Nout and K Nout must stay below 2^31. */
int p3d_clip_gemm_plan(int M, int K, int Nout, int force_plan, int* out4);
size_t p3d_clip_gemm_workspace_bytes(int M, int K, int Nout, int force_plan); /* split > 1 ? split M Nout sizeof(float) : 0 */
/* out[M][Nout] = epi(A[M][K] W[K][Nout]).
 *   z[m][n] = sum over k of A[m][k] W[k][n]: split s takes k in [64 cps s, min(K, 64 cps (s + 1))) ascending as ONE fma chain that
 *   starts from 0.  split == 1: the chain's result is z.  split > 1: partial s goes to workspace[s][m][n]; a second launch forms
 *   z = ((p_0 + p_1) + p_2) + ... ascending.  The epilogue is applied once, after the reduction, in this order:
 *     v = z + bias[n]                                   (bias may be NULL: v = z)
 *     v = v * (1 / (1 + exp(-1.702f * v)))              with P3D_CLIP_GELU (QuickGELU; exp is the library's expf, the division IEEE)
 *     v = res[m][n] + v                                 (res may be NULL; out == res exactly is allowed: each value is read and written
 *                                                        by the same lane)
 * P3D_CLIP_PATCH: A is an image [N][3][S][S], row (n, py, px) of the GEMM is its patch (py, px) flattened in (c, y, x) order:
 * A[m][k] = img[n][c][py patch + y][px patch + x]; M = N (S / patch)^2 and K = 3 patch^2 are checked (conv1 with stride = patch, no
 * bias).  Without the flag N, S and patch must be 0.  Any M, K, Nout >= 1: ragged edges are predicated.
 * Launch order: the workgroups of one (column tile, split) pair — they read the same 64-column slab of W — have consecutive places in
 * one XCD's queue (linear id L: XCD L % 8, place L / 8), so that a slab is fetched from memory once and re-read from that XCD's L2. */
int p3d_clip_gemm_f32(const float* a, int M, int K, const float* w, int Nout, const float* bias, const float* res, int flags, int N,
                      int S, int patch, float* out, int force_plan, void* workspace, size_t workspace_bytes, void* stream);

/* ---- 3. LayerNorm ----------------------------------------------------------------------------------------------------------------
 * Per row of x (row r at x + r ldx, ldx >= D: ldx = T D normalises the class token of each image without a gather), one wave per row:
 *   mean = (the wave tree's sum of x) / D;  var = (the wave tree's sum of (x - mean)^2) / D   (two passes, biased; the square is a
 *   product, added with a separate addition);  r = 1 / sqrt(var + eps) (correctly rounded sqrt, IEEE division);
 *   y[r][d] = ((x - mean) * r) * gamma[d] + beta[d]                                       (y [M][D] dense; no fused multiply-add) */
int p3d_clip_layernorm_f32(const float* x, int M, int D, int64_t ldx, const float* gamma, const float* beta, float eps, float* y,
                           void* stream);
/* The embedding step: row (n, t) of y [N T][D] is the LayerNorm above (ln_pre) of tok + pos[t], tok = cls for t = 0 and row
 * (n, t - 1) of patches [N (T - 1)][D] otherwise.  T >= 1 (T = 1: patches is not read and may be NULL). */
int p3d_clip_embed_f32(const float* patches, const float* cls, const float* pos, int N, int T, int D, const float* gamma,
                       const float* beta, float eps, float* y, void* stream);

/* ---- 4. attention ----------------------------------------------------------------------------------------------------------------
 * qkv [N T][3 D], columns q | k | v, head h takes columns 64 h .. 64 h + 63 of each; out [N T][D].  Per image, head and query row i:
 *   s_j = 0.125f * (fma chain over c ascending from 0 of q_ic k_jc);  m = max_j s_j;  p_j = expf(s_j - m);
 *   l = sum_j p_j, j ascending from 0;  o_c = (fma chain over j ascending from 0 of p_j v_jc) / l          (IEEE division)
 * D = 64 heads and 1 <= T <= 64, anything else P3D_E_RANGE.  One workgroup takes one (image, head) and a block of query rows, with those
 * rows of Q and that head's whole K and V in LDS; the plan wants want = min(ceil(T / 4), ceil(256 / (N heads))) blocks and cuts the rows into blocks of
 * rows = max(1, floor(T / want)), qblocks = ceil(T / rows) >= want: at least 256 workgroups wherever N heads ceil(T / 4) >= 256.
 * The cut does not change any sum.  out4 (HOST): {workgroups, qblocks, rows per block, LDS bytes the kernel reserves (sized for
 * T = 64: 50 432; T = 50 uses 38.6 KB of it)}. */
int p3d_clip_attention_plan(int N, int T, int heads, int* out4);
int p3d_clip_attention_f32(const float* qkv, int N, int T, int heads, int D, float* out, void* stream);

/* ---- 5. the cosine ---------------------------------------------------------------------------------------------------------------
 * measure.py:42 per pair: sim[i] = dot / (sqrt(aa) * sqrt(bb)) with dot, aa, bb the wave tree's sums (each term one fma into the
 * lane's accumulator) of a_i b_i, a_i a_i, b_i b_i over row i of a and of b, both [pairs][D].  Row i against row i, not all against all. */
int p3d_clip_cosine_f32(const float* a, const float* b, int pairs, int D, float* sim, void* stream);

/* ---- 6. the walk -----------------------------------------------------------------------------------------------------------------*/
#define P3D_CLIP_KIND_PREPARE 0
#define P3D_CLIP_KIND_GEMM 1
#define P3D_CLIP_KIND_LAYERNORM 2
#define P3D_CLIP_KIND_EMBED 3
#define P3D_CLIP_KIND_ATTENTION 4
typedef struct p3d_clip_step {
    int32_t kind;            /* P3D_CLIP_KIND_* */
    int32_t M, K, Nout;      /* GEMM: its sizes.  LAYERNORM: M rows, K = Nout = D.  EMBED: M = N T, K = Nout = D.  ATTENTION: M = N T,
                                K = 3 D, Nout = D.  PREPARE: M = N, K = C, Nout = 3 */
    int32_t N, T, heads;     /* ATTENTION: N, T, heads.  EMBED: N, T.  GEMM with P3D_CLIP_PATCH: N.  PREPARE: N.  Else 0 */
    int32_t S, patch;        /* GEMM with P3D_CLIP_PATCH: the image side and the patch side.  PREPARE: S.  Else 0 */
    int32_t H, W;            /* PREPARE: the source size.  Else 0 */
    int32_t ld;              /* LAYERNORM: the input's row stride in floats.  Else 0 */
    int32_t in, out, res;    /* buffer indices into the arena; res = -1: none (GEMM only) */
    int32_t flags;           /* GEMM: P3D_CLIP_GELU | P3D_CLIP_PATCH */
    int32_t plan;            /* GEMM: force_plan (0 = choose) */
    float eps;               /* LAYERNORM, EMBED */
    int32_t reserved[2];     /* 0 */
    int64_t w_off, b_off;    /* offsets in floats into the weight blob.  GEMM: W and bias (b_off = -1: none).  LAYERNORM, EMBED: gamma and
                                beta.  PREPARE: tabx and taby, int32 values stored in the blob's 4-byte cells */
    int64_t w2_off, b2_off;  /* EMBED: cls [D] and pos [T][D].  Else 0 */
} p3d_clip_step;

/* sizeof(p3d_clip_step) and its field offsets in declaration order (reserved once), for a binding that restates the struct. */
int p3d_clip_struct_layout(size_t* out, int cap);

/* The whole network: walks `steps` (HOST, n_steps records) in order on one stream — one call, one launch per step plus one per split-K
 * reduction and two for PREPARE; no graph capture; the bits of the step-by-step entry points.  Buffer b of the activation arena is
 * arena[buf_off[b] .. buf_off[b] + buf_len[b]) in floats (HOST arrays); weights: one DEVICE blob.
 * Checked before any launch, for every record: the kind; the sizes as the step's own entry point checks them, and the fields that
 * restate them; in / out / res in [0, n_bufs), in != out (res == out is the residual stream's normal form), res != in; each buffer
 * long enough for the tensor put into it or read from it and inside the arena; the offset ranges inside the blob; reserved == 0; the
 * largest workspace any step needs against workspace_bytes (P3D_E_WORKSPACE). */
int p3d_clip_forward_f32(const p3d_clip_step* steps, int n_steps, const float* weights, int64_t weight_floats, float* arena,
                         int64_t arena_floats, const int64_t* buf_off, const int64_t* buf_len, int n_bufs, void* workspace,
                         size_t workspace_bytes, void* stream);
size_t p3d_clip_workspace_bytes(const p3d_clip_step* steps, int n_steps); /* the maximum over the steps (0 for a refused table) */

/* ---- 7. PSNR ---------------------------------------------------------------------------------------------------------------------
 * The three reductions of 10 log10(range^2 / mse) over `count` values, one pass: out3 (DEVICE) = {sum (pred - target)^2, min target,
 * max target}.  B = min(1024, ceil(count / 4096)) workgroups of 256 lanes; lane t of workgroup b takes the elements 256 b + t,
 * + 256 B, + 512 B, ... ascending (d = pred - target, acc = fma(d, d, acc) from 0); a workgroup's value is the wave tree's butterfly
 * of each wave, then ((w0 + w1) + w2) + w3; a second launch of one workgroup reduces the B partials the same way (lane t takes
 * partials t, t + 256, ...).  min and max likewise (exact in any order).  The logarithm is the caller's, in float64. */
size_t p3d_psnr_workspace_bytes(int64_t count); /* 3 B sizeof(float) */
int p3d_psnr_f32(const float* pred, const float* target, int64_t count, float* out3, void* workspace, size_t workspace_bytes,
                 void* stream);

#ifdef __cplusplus
}
#endif
#endif
