/* p3d_paste_grad.h — C ABI of the backward pass of the front-view paste (p3d_paste_front_f32; MI355X / gfx950).
 *
 * The forward (training/triplane.py:607-691) returns image = torch.lerp(image_in, paste, mask) and paste =
 * sample_orthofront(illustration, interpolate(image_xyz, S)); the masks are computed under no_grad in the reference and are
 * constants here: the backward reads the forward's own mask.
 *
 * Conventions of panic3d_hip.h: raw DEVICE pointers, the stream last, 0 / negative P3D_E_* / positive hipError_t, no allocation,
 * caller-owned workspace (size from the *_workspace_bytes query, 256-byte aligned), every argument checked before any launch.
 *
 * Arithmetic (binary32; the up-sampling taps and the sampling taps are recomputed with the forward's own expressions, so they are
 * the forward's bits):
 *   g_image = g_out * (1 - mask)                       (torch.lerp's derivative with respect to its start, in both of its branches)
 *   g_paste = g_out * mask + g_paste_direct            (either term may be absent)
 * and, with grad_sample (otherwise the paste is a constant, as in the reference, and only g_image is produced):
 *   per output pixel, g_ix / g_iy = sum over the 3 channels of g_paste * d(bilinear sample) / d(ix, iy) from the forward's four taps
 *     (an out-of-range tap counts 0), ZERO where the forward clamped the coordinate to the border (unclamped ix <= 0 or >= S - 1:
 *     F.grid_sample's rule for padding_mode='border'), times d ix / d up_y = d iy / d up_x = -S / box_warp: the illustration is
 *     sampled transposed, so grid x comes from xyz channel 1 and grid y from channel 0; normalize_images scales the taps by 2;
 *   g_xyz[N][3][r][r] = the adjoint of the r -> S bilinear resize as a GATHER: each texel sums, rows then columns in ascending
 *     order, the pixels whose up-sampling taps touch it.  Channel 2 is written as zero.  No atomics: g_xyz and g_image are bitwise
 *     reproducible run to run;
 *   g_front[N or 1][3][S][S] (only when asked for) = the four-tap scatter of g_paste * tap weight (x 2 under normalize_images),
 *     accumulated with global_atomic_add_f32 (no return value): equal run to run up to the order of the additions.  A shared
 *     illustration (front_shared: one for the N views) receives the sum over the views.  The function zeroes g_front itself.
 */
#ifndef P3D_PASTE_GRAD_H
#define P3D_PASTE_GRAD_H
#include "panic3d_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct p3d_paste_grad_args {
    const float* g_out;    /* [N][3][S][S] cotangent of the pasted image, or NULL (zero) */
    const float* g_paste;  /* [N][3][S][S] cotangent of the returned paste, or NULL (zero); g_out and g_paste not both NULL */
    const float* mask;     /* [N][1][S][S] the forward's out_mask */
    const float* xyz;      /* [N][3][r][r] the forward's xyz (needed for g_xyz / g_front) */
    const float* front;    /* [N or 1][3][S][S] the forward's illustration (needed for g_xyz / g_front) */
    float* g_image;        /* [N][3][S][S] or NULL: not computed */
    float* g_xyz;          /* [N][3][r][r] or NULL: not computed; needs grad_sample and the workspace */
    float* g_front;        /* [N or 1][3][S][S] or NULL: not computed; needs grad_sample */
    void* workspace;       /* the per-pixel gradients of the up-sampled x and y ([N][2][S][S] floats); only for g_xyz */
    size_t workspace_bytes;
    int32_t N, r, S, front_shared, normalize_images, grad_sample;
    float box_warp;
} p3d_paste_grad_args;

/* Bytes of workspace p3d_paste_front_backward_f32 needs to produce g_xyz (0 for non-positive sizes). */
size_t p3d_paste_front_backward_workspace_bytes(int N, int S);

/* P3D_E_ARG: args / mask NULL, both cotangents NULL, no output asked for, non-positive N / r / S, g_xyz or g_front without
 * grad_sample, xyz or front missing where needed, workspace NULL or unaligned; P3D_E_RANGE: r > 4096 or S > 8192 (the forward's
 * limits); P3D_E_WORKSPACE: workspace too small. */
int p3d_paste_front_backward_f32(const p3d_paste_grad_args* args, void* stream);

#ifdef __cplusplus
}
#endif
#endif
