/* p3d_render_grad.h — C ABI of the backward passes of libpanic3d_hip.so (MI355X / gfx950).
 *
 * Gradients of the fused renderer (p3d_render_f32 / p3d_render_limits_f32 / p3d_render_rng_f32: ImportanceRenderer.forward,
 * renderer.py:162-264) and of the point decode (p3d_triplane_decode_f32: run_model, renderer.py:266-280) with respect to the
 * triplanes and the four pre-scaled OSGDecoder tensors (training/triplane.py:516-544).  Gradients to rays, ray limits and depths are
 * not computed: the reference draws its depths (stratified jitter, sample_importance under torch.no_grad, renderer.py:332).
 *
 * Conventions of panic3d_hip.h: raw DEVICE pointers, the stream last, 0 / negative P3D_E_* / positive hipError_t, no allocation,
 * caller-owned workspace (size from the matching *_workspace_bytes query, 256-byte aligned), every argument checked before any launch.
 *
 * Arithmetic: every sample is re-decoded on the exact contract of include/p3d_numerics.h (whatever mode the forward ran in), so the
 * densities, mask decisions and weights the backward sees are the exact forward's bits.  The gradients themselves are binary32
 * (fp32 tolerance against the reference's autograd).  Decoder gradients are reduced in a fixed order (per-workgroup partial slabs
 * + one reduce launch): bitwise reproducible run to run for the same sizes.  Plane gradients are accumulated with float atomics:
 * equal run to run up to the order of the additions.
 */
#ifndef P3D_RENDER_GRAD_H
#define P3D_RENDER_GRAD_H
#include "panic3d_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Workspace of p3d_render_backward_f32 for N images of R rays and Sc + Sf merged samples per ray. */
size_t p3d_render_backward_workspace_bytes(int N, int64_t R, int Sc, int Sf);

/* Backward of ImportanceRenderer.forward at the forward's merged, sorted depths.
 *   planes_nhwc [N][3][H][W][32] (or [1][...] with P3D_FLAG_SHARED_PLANES), rays_o / rays_d [N][R][3], w0 [64][32], b0 [64],
 *   w1 [33][64], b1 [33] (pre-scaled): the forward's inputs; opts: the forward's options (Sc, Sf, masks, force_sigmoid, white_back,
 *   coord_scale, plane_mode, P3D_FLAG_PER_VIEW_CLAMP, P3D_FLAG_SHARED_PLANES are read; every other flag is ignored).
 *   depths_sorted [N*R][Sc+Sf]: the forward's p3d_dumps.depths_sorted (Sf == 0: the coarse depths).
 *   g_feat [N][R][32], g_depth [N][R], g_wsum [N][R], g_xyz [N][R][3]: cotangents of the four outputs; any may be NULL (zero).
 * Outputs:
 *   d_planes_nhwc: ACCUMULATED into (the caller zeroes it), same shape as planes_nhwc; NULL: the plane gradient is not wanted
 *                  (no scatter: decoder gradients only);
 *   d_w0 [64][32], d_b0 [64], d_w1 [33][64], d_b1 [33]: OVERWRITTEN with the gradients of the pre-scaled tensors. */
int p3d_render_backward_f32(const float* planes_nhwc, int N, int H, int W, const float* rays_o, const float* rays_d, int64_t R,
                            const float* depths_sorted, const float* w0, const float* b0, const float* w1, const float* b1,
                            const p3d_opts* opts, const float* g_feat, const float* g_depth, const float* g_wsum,
                            const float* g_xyz, float* d_planes_nhwc, float* d_w0, float* d_b0, float* d_w1, float* d_b1,
                            void* workspace, size_t workspace_bytes, void* stream);

/* Workspace of p3d_triplane_decode_backward_f32 for N batches of M points. */
size_t p3d_triplane_decode_backward_workspace_bytes(int N, int64_t M);

/* Backward of run_model / p3d_triplane_decode_f32: coords [N][M][3], g_sigma [N][M] and g_rgb [N][M][32] (either may be NULL).
 * Masks of opts.flags (crop / cull / binarize) zero the density gradient of the points they overwrite, as in the forward.
 * Outputs as for p3d_render_backward_f32. */
int p3d_triplane_decode_backward_f32(const float* planes_nhwc, int N, int H, int W, const float* coords, int64_t M,
                                     const float* w0, const float* b0, const float* w1, const float* b1, const p3d_opts* opts,
                                     const float* g_sigma, const float* g_rgb, float* d_planes_nhwc, float* d_w0, float* d_b0,
                                     float* d_w1, float* d_b1, void* workspace, size_t workspace_bytes, void* stream);

/* Statistics of the last p3d_render_backward_f32 / p3d_triplane_decode_backward_f32 call on a workspace (host-readable after the
 * stream is synchronised): u64 at byte 0 of the workspace = samples that ran the MLP backward and the plane scatter. */
#define P3D_GRAD_STATS_BYTES 256

#ifdef __cplusplus
}
#endif
#endif
