/* p3d_optim.h — C ABI of the optimiser step (MI355X / gfx950): multi-tensor Adam with the gradient clean-up of the training
 * loop (training_loop_v0.py:364-375) and the G_ema update (:387-392), any number of tensors in ONE launch.
 *
 * Conventions of panic3d_hip.h: raw DEVICE pointers, the stream last, 0 / negative P3D_E_* / positive hipError_t, no allocation,
 * every argument checked before any launch.  The three tables an update reads live in DEVICE memory and are the caller's: the
 * library cannot look into them, so a table that names memory the caller does not own is the caller's fault, as a wrong pointer is.
 *
 * Arithmetic, per element, binary32, every operation rounded once (no contraction; sqrt and / correctly rounded):
 *   g  = grad * grad_scale                                         (grad_scale = 1 / num_gpus; scaling comes BEFORE cleaning)
 *   g  = isnan(g) ? nan_v : g == +inf ? posinf_v : g == -inf ? neginf_v : g       (only with `sanitize`; finite values pass unchanged)
 *   m1 = b1 * m0 + c1 * g            b1 = (float)beta1, c1 = (float)(1.0 - beta1), the subtraction in double
 *   v1 = b2 * v0 + (c2 * g) * g      b2 = (float)beta2, c2 = (float)(1.0 - beta2)
 *   p1 = p0 - step_size * (m1 / (sqrt(v1) / bc2_sqrt + eps))
 *   e1 = w == 0 ? p1 : w == 1 ? e0 : w < 0.5 ? p1 + w * (e0 - p1) : e0 - (e0 - p1) * (1 - w)       (torch's lerp(p1, e0, w), on the NEW p)
 * With beta1 == 0 the kernel does not read m: m1 = g, the same bits (0 * m0 + 1 * g) for every finite m0.  m is written in every
 * Adam mode.  The caller computes step_size = lr / (1 - beta1^step) and bc2_sqrt = sqrt(1 - beta2^step) per tensor in double from
 * that tensor's own step count (torch.optim.Adam's non-capturable form) and rounds them to binary32.
 * The two ends of the EMA weight are selects, so w = 0 copies p1 and w = 1 keeps e0 bit for bit, signed zeros and infinities too.
 *
 * Every element is read and written by exactly one lane and nothing is summed across elements: results are bitwise reproducible,
 * and do not depend on which of the two access widths a tensor takes.
 */
#ifndef P3D_OPTIM_H
#define P3D_OPTIM_H
#include "panic3d_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define P3D_OPTIM_CHUNK 4096 /* elements of one workgroup: 256 lanes x 4 x 16 bytes per stream */

#define P3D_OPTIM_ADAM 1     /* p, m, v <- Adam(grad) */
#define P3D_OPTIM_ADAM_EMA 2 /* the same, then ema <- lerp(p1, ema, w) */
#define P3D_OPTIM_EMA 3      /* ema <- lerp(p, ema, w) alone: grad, m, v, step_size and bc2_sqrt are not read */

/* The static part of the tensor table: one entry per tensor, uploaded once per optimiser. */
typedef struct p3d_optim_tensor {
    float* p;          /* [numel] the parameter (read-only in mode EMA) */
    float* m;          /* [numel] exp_avg;     unused (may be NULL) in mode EMA */
    float* v;          /* [numel] exp_avg_sq;  unused (may be NULL) in mode EMA */
    float* ema;        /* [numel] the EMA copy; unused (may be NULL) in mode ADAM */
    int64_t numel;
    int32_t aligned16; /* every pointer above that the mode uses is 16-byte aligned (p3d_optim_aligned16) */
    int32_t reserved;  /* 0 */
} p3d_optim_tensor;

/* The dynamic part: one entry per tensor, uploaded per step. */
typedef struct p3d_optim_step {
    const float* grad;      /* [numel], or NULL: Adam SKIPS the tensor in this step — p, m, v stay untouched; its ema still follows p (ADAM_EMA) */
    float step_size;        /* lr / (1 - beta1^step) */
    float bc2_sqrt;         /* sqrt(1 - beta2^step) */
    float ema_w;            /* the weight of the OLD ema value, in [0, 1]; 0 copies (a buffer) */
    int32_t grad_aligned16; /* grad is 16-byte aligned (a segment of a flat gradient vector usually is not) */
} p3d_optim_step;

/* One workgroup's share: elements [offset, offset + count) of tensor `tensor`; offset is a multiple of P3D_OPTIM_CHUNK and
 * 1 <= count <= P3D_OPTIM_CHUNK.  A chunk never crosses a tensor. */
typedef struct p3d_optim_chunk {
    int64_t offset;
    int32_t tensor;
    int32_t count;
} p3d_optim_chunk;

typedef struct p3d_optim_args {
    const p3d_optim_tensor* tensors; /* DEVICE [n_tensors] */
    const p3d_optim_step* steps;     /* DEVICE [n_tensors] */
    const p3d_optim_chunk* chunks;   /* DEVICE [n_chunks], as p3d_optim_plan wrote them */
    int64_t n_chunks;
    int32_t n_tensors;
    int32_t mode;     /* P3D_OPTIM_* */
    int32_t sanitize; /* 0 / 1 */
    float grad_scale, nan_v, posinf_v, neginf_v;
    float eps;
    double beta1, beta2; /* in [0, 1) */
} p3d_optim_args;

/* The chunk plan, on the host: a pure function of the numels.  Writes the chunks of tensor 0, then tensor 1, ... in ascending
 * offset; a tensor with numel 0 gets none.  chunks == NULL (capacity ignored) only counts.  Returns the number of chunks, or
 * P3D_E_ARG (numels NULL, n_tensors <= 0, a negative numel), P3D_E_RANGE (more than 2^31 - 1 chunks) or P3D_E_WORKSPACE (capacity
 * too small). */
int64_t p3d_optim_plan(const int64_t* numels, int n_tensors, p3d_optim_chunk* chunks, int64_t capacity);

/* 1 when every non-NULL pointer of ptrs[0 .. n) is 16-byte aligned, else 0 (0 for ptrs == NULL or n <= 0). */
int p3d_optim_aligned16(const void* const* ptrs, int n);

/* One launch of n_chunks workgroups.  P3D_E_ARG: args or one of its tables NULL, n_tensors <= 0, n_chunks <= 0; P3D_E_RANGE: an
 * unknown mode, n_chunks > 2^31 - 1, beta1 or beta2 outside [0, 1), eps < 0 or any of these not a number. */
int p3d_optim_step_f32(const p3d_optim_args* args, void* stream);

/* sizeof and field offsets of the structs above, for a binding that restates them (ctypes ...): which = P3D_OPTIM_STRUCT_*;
 * out[0] = sizeof, out[1 + i] = offsetof field i in declaration order; returns the number of entries or P3D_E_ARG / P3D_E_RANGE
 * (out NULL / cap too small, unknown `which`), as p3d_struct_layout does for the structs of panic3d_hip.h. */
#define P3D_OPTIM_STRUCT_TENSOR 0
#define P3D_OPTIM_STRUCT_STEP 1
#define P3D_OPTIM_STRUCT_CHUNK 2
#define P3D_OPTIM_STRUCT_ARGS 3
int p3d_optim_struct_layout(int which, size_t* out, int cap);

#ifdef __cplusplus
}
#endif
#endif
