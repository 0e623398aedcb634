// p3d_optim.hip — the optimiser step (include/p3d_optim.h): multi-tensor Adam with the gradient clean-up and the
// G_ema update, any number of tensors in one launch.
//
//   k_adam_ema<ADAM, EMA, READ_M>   one 256-lane workgroup per chunk of the plan (p3d_optim_plan.hpp): at most P3D_OPTIM_CHUNK
//                  elements of ONE tensor.  The chunk, the tensor's table entry and its per-step entry are uniform across the
//                  workgroup.  Of a tensor without a gradient in this step p, m and v are not touched (its EMA copy still follows p).
//                  A full chunk of a tensor whose pointers are all 16-byte aligned takes the 16-byte path: per lane four float4
//                  of every stream, every load issued before the first use (up to 5 streams x 4 x 16 B = 320 B per lane in
//                  flight).  Anything else — the last, partial chunk of a tensor, a segment of a flat gradient vector — takes
//                  the 4-byte path: batches of four lane-strided elements, the loads of a batch issued before its first use.
//                  Both paths run the same per-element function, so a value does not depend on the path it took.
// Memory-bound: ADAM reads g, v, p and writes m, v, p (READ_M adds m), ADAM_EMA adds a read and a write of e.  Plain vector
// loads and stores only; no LDS, no atomics.
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "../../include/p3d_optim.h"
#include "p3d_optim_plan.hpp"

#define OP_WG 256
#define OP_VEC (P3D_OPTIM_CHUNK / (OP_WG * 4))  // float4 per lane and stream in a full chunk
static_assert(OP_VEC * OP_WG * 4 == P3D_OPTIM_CHUNK, "a full chunk is a whole number of float4 per lane");

// A pointer read from a table in memory is a generic one to the compiler, and a generic access is a flat_load / flat_store that
// also counts against the LDS counter.  Every pointer of the tables is global memory: say so.
typedef float op_f4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) float op_gf;
typedef __attribute__((address_space(1))) op_f4 op_gf4;

struct OptimScalars {
    float grad_scale, nan_v, posinf_v, neginf_v;
    float b1, c1, b2, c2, eps;
    int sanitize;
};

struct OptimElem {
    float p, m, v, e;
};

// The per-element arithmetic of include/p3d_optim.h, one rounding per operation (-ffp-contract=off).
template <bool ADAM, bool EMA, bool READ_M>
static __device__ __forceinline__ OptimElem optim_elem(float g, OptimElem s, const OptimScalars& k, float step_size, float bc2_sqrt, float w) {
    OptimElem o = s;
    if (ADAM) {
        g = g * k.grad_scale;
        if (k.sanitize) g = (g != g) ? k.nan_v : (g == INFINITY) ? k.posinf_v : (g == -INFINITY) ? k.neginf_v : g;
        o.m = READ_M ? k.b1 * s.m + k.c1 * g : g;
        o.v = k.b2 * s.v + (k.c2 * g) * g;
        const float denom = __fsqrt_rn(o.v) / bc2_sqrt + k.eps;
        o.p = s.p - step_size * (o.m / denom);
    }
    if (EMA) {
        const float d = s.e - o.p;
        const float lo = o.p + w * d, hi = s.e - d * (1.0f - w);
        o.e = (w == 0.0f) ? o.p : (w == 1.0f) ? s.e : (w < 0.5f) ? lo : hi;
    }
    return o;
}

// One chunk in one mode.  `ch`, `st` and `tn` are uniform across the workgroup.
template <bool ADAM, bool EMA, bool READ_M>
static __device__ __forceinline__ void optim_chunk(const p3d_optim_chunk& ch, const p3d_optim_step& st, const p3d_optim_tensor& tn,
                                                   const OptimScalars& k) {
    const op_gf* __restrict__ g = ADAM ? (const op_gf*)st.grad + ch.offset : nullptr;
    op_gf* __restrict__ p = (op_gf*)tn.p + ch.offset;
    op_gf* __restrict__ m = ADAM ? (op_gf*)tn.m + ch.offset : nullptr;
    op_gf* __restrict__ v = ADAM ? (op_gf*)tn.v + ch.offset : nullptr;
    op_gf* __restrict__ e = EMA ? (op_gf*)tn.ema + ch.offset : nullptr;
    const int tid = threadIdx.x;

    if (ch.count == P3D_OPTIM_CHUNK && tn.aligned16 && (!ADAM || st.grad_aligned16)) {
        op_f4 G[OP_VEC], P[OP_VEC], M[OP_VEC], V[OP_VEC], E[OP_VEC];
#pragma unroll
        for (int j = 0; j < OP_VEC; ++j) {
            const int i = j * OP_WG + tid;  // a wave-instruction covers 64 consecutive float4: 1 KiB
            if (ADAM) G[j] = ((const op_gf4*)g)[i];
            if (ADAM && READ_M) M[j] = ((const op_gf4*)m)[i];
            if (ADAM) V[j] = ((const op_gf4*)v)[i];
            P[j] = ((const op_gf4*)p)[i];
            if (EMA) E[j] = ((const op_gf4*)e)[i];
        }
#pragma unroll
        for (int j = 0; j < OP_VEC; ++j) {
            const int i = j * OP_WG + tid;
            op_f4 p1, m1, v1, e1;
#define OP_LANE(c)                                                                                                                      \
    {                                                                                                                                   \
        const OptimElem s = {P[j].c, (ADAM && READ_M) ? M[j].c : 0.f, ADAM ? V[j].c : 0.f, EMA ? E[j].c : 0.f};                              \
        const OptimElem o = optim_elem<ADAM, EMA, READ_M>(ADAM ? G[j].c : 0.f, s, k, st.step_size, st.bc2_sqrt, st.ema_w);                \
        p1.c = o.p, m1.c = o.m, v1.c = o.v, e1.c = o.e;                                                                                \
    }
            OP_LANE(x) OP_LANE(y) OP_LANE(z) OP_LANE(w)
#undef OP_LANE
            if (ADAM) {
                ((op_gf4*)m)[i] = m1;
                ((op_gf4*)v)[i] = v1;
                ((op_gf4*)p)[i] = p1;
            }
            if (EMA) ((op_gf4*)e)[i] = e1;
        }
        return;
    }

    // the 4-byte path: batches of 4 x 256 elements, lane-strided; i < count guards every access
    for (int base = 0; base < ch.count; base += 4 * OP_WG) {
        float G[4], P[4], M[4], V[4], E[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = base + j * OP_WG + tid;
            const bool in = i < ch.count;
            G[j] = (ADAM && in) ? g[i] : 0.f;
            M[j] = (ADAM && READ_M && in) ? m[i] : 0.f;
            V[j] = (ADAM && in) ? v[i] : 0.f;
            P[j] = in ? p[i] : 0.f;
            E[j] = (EMA && in) ? e[i] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = base + j * OP_WG + tid;
            if (i >= ch.count) continue;
            const OptimElem s = {P[j], M[j], V[j], E[j]};
            const OptimElem o = optim_elem<ADAM, EMA, READ_M>(G[j], s, k, st.step_size, st.bc2_sqrt, st.ema_w);
            if (ADAM) {
                m[i] = o.m;
                v[i] = o.v;
                p[i] = o.p;
            }
            if (EMA) e[i] = o.e;
        }
    }
}

// A tensor without a gradient in this step is skipped by Adam (torch.optim.Adam skips grad is None): p, m, v stay untouched.  Its
// EMA copy still follows p in mode ADAM_EMA, so that the fused launch equals an Adam launch followed by an EMA launch.
template <bool ADAM, bool EMA, bool READ_M>
__global__ __launch_bounds__(OP_WG) void k_adam_ema(const p3d_optim_tensor* __restrict__ tensors, const p3d_optim_step* __restrict__ steps,
                                                    const p3d_optim_chunk* __restrict__ chunks, OptimScalars k) {
    const p3d_optim_chunk ch = chunks[blockIdx.x];
    const p3d_optim_step st = steps[ch.tensor];
    if (ADAM && !st.grad) {
        if (EMA) optim_chunk<false, true, false>(ch, st, tensors[ch.tensor], k);
        return;
    }
    optim_chunk<ADAM, EMA, READ_M>(ch, st, tensors[ch.tensor], k);
}

extern "C" int64_t p3d_optim_plan(const int64_t* numels, int n_tensors, p3d_optim_chunk* chunks, int64_t capacity) {
    return optim_plan(numels, n_tensors, chunks, capacity);
}

extern "C" int p3d_optim_aligned16(const void* const* ptrs, int n) { return optim_aligned16(ptrs, n); }

extern "C" int p3d_optim_step_f32(const p3d_optim_args* a, void* stream) {
    if (!a || !a->tensors || !a->steps || !a->chunks) return P3D_E_ARG;
    if (a->n_tensors <= 0 || a->n_chunks <= 0) return P3D_E_ARG;
    if (a->mode != P3D_OPTIM_ADAM && a->mode != P3D_OPTIM_ADAM_EMA && a->mode != P3D_OPTIM_EMA) return P3D_E_RANGE;
    if (a->n_chunks > OPTIM_MAX_CHUNKS) return P3D_E_RANGE;
    if (!(a->beta1 >= 0.0 && a->beta1 < 1.0) || !(a->beta2 >= 0.0 && a->beta2 < 1.0) || !(a->eps >= 0.f)) return P3D_E_RANGE;  // (NaN fails every comparison)
    OptimScalars k;
    k.grad_scale = a->grad_scale, k.nan_v = a->nan_v, k.posinf_v = a->posinf_v, k.neginf_v = a->neginf_v;
    k.b1 = (float)a->beta1, k.c1 = (float)(1.0 - a->beta1), k.b2 = (float)a->beta2, k.c2 = (float)(1.0 - a->beta2), k.eps = a->eps;
    k.sanitize = a->sanitize != 0;
    const dim3 grid((unsigned)a->n_chunks), block(OP_WG);
    hipStream_t s = (hipStream_t)stream;
#define OP_LAUNCH(ADAM, EMA, READ_M) hipLaunchKernelGGL((k_adam_ema<ADAM, EMA, READ_M>), grid, block, 0, s, a->tensors, a->steps, a->chunks, k)
    const bool read_m = k.b1 != 0.f;
    if (a->mode == P3D_OPTIM_EMA) OP_LAUNCH(false, true, false);
    else if (a->mode == P3D_OPTIM_ADAM_EMA) {
        if (read_m) OP_LAUNCH(true, true, true);
        else OP_LAUNCH(true, true, false);
    } else {
        if (read_m) OP_LAUNCH(true, false, true);
        else OP_LAUNCH(true, false, false);
    }
#undef OP_LAUNCH
    return (int)hipGetLastError();
}

extern "C" int p3d_optim_struct_layout(int which, size_t* out, int cap) {
    if (!out || cap <= 0) return P3D_E_ARG;
    int n = 0;
#define OP_PUT(v) do { if (n >= cap) return P3D_E_RANGE; out[n++] = (size_t)(v); } while (0)
#define OP_OFF(T, f) OP_PUT(offsetof(T, f))
    switch (which) {
    case P3D_OPTIM_STRUCT_TENSOR:
        OP_PUT(sizeof(p3d_optim_tensor));
        OP_OFF(p3d_optim_tensor, p); OP_OFF(p3d_optim_tensor, m); OP_OFF(p3d_optim_tensor, v); OP_OFF(p3d_optim_tensor, ema);
        OP_OFF(p3d_optim_tensor, numel); OP_OFF(p3d_optim_tensor, aligned16); OP_OFF(p3d_optim_tensor, reserved);
        break;
    case P3D_OPTIM_STRUCT_STEP:
        OP_PUT(sizeof(p3d_optim_step));
        OP_OFF(p3d_optim_step, grad); OP_OFF(p3d_optim_step, step_size); OP_OFF(p3d_optim_step, bc2_sqrt); OP_OFF(p3d_optim_step, ema_w);
        OP_OFF(p3d_optim_step, grad_aligned16);
        break;
    case P3D_OPTIM_STRUCT_CHUNK:
        OP_PUT(sizeof(p3d_optim_chunk));
        OP_OFF(p3d_optim_chunk, offset); OP_OFF(p3d_optim_chunk, tensor); OP_OFF(p3d_optim_chunk, count);
        break;
    case P3D_OPTIM_STRUCT_ARGS:
        OP_PUT(sizeof(p3d_optim_args));
        OP_OFF(p3d_optim_args, tensors); OP_OFF(p3d_optim_args, steps); OP_OFF(p3d_optim_args, chunks); OP_OFF(p3d_optim_args, n_chunks);
        OP_OFF(p3d_optim_args, n_tensors); OP_OFF(p3d_optim_args, mode); OP_OFF(p3d_optim_args, sanitize); OP_OFF(p3d_optim_args, grad_scale);
        OP_OFF(p3d_optim_args, nan_v); OP_OFF(p3d_optim_args, posinf_v); OP_OFF(p3d_optim_args, neginf_v); OP_OFF(p3d_optim_args, eps);
        OP_OFF(p3d_optim_args, beta1); OP_OFF(p3d_optim_args, beta2);
        break;
    default:
        return P3D_E_RANGE;
    }
#undef OP_OFF
#undef OP_PUT
    return n;
}
