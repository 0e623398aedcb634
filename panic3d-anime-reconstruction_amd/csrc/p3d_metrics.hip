// p3d_metrics.hip — the squared distance from points to a triangle mesh (include/p3d_metrics.h), brute force.
//   k_pm_prepare  one lane per face: gathers the vertices into a 64-byte record, so the pair loop never chases an index; one wave per
//                 face tile: the tile's bounding box and its longest squared edge
//   k_pm_pairs    lanes are queries (two per lane, kept in registers with their running minimum); a workgroup is ONE wave, stages a
//                 tile of records in LDS and every lane reads the same record (a broadcast).  Grid = query blocks x face slices;
//                 each (query, slice) minimum goes to the workspace
//                 With culling the loop runs twice: first over the SAMPLE records (the first face of every tile, 1/64 of the work), whose
//                 per-query minimum (k_pm_reduce into a [Q] array) seeds the culling bound of the second run — without it every slice
//                 would have to find a near face of its own before it could skip anything
//   k_pm_reduce   one lane per query: the minimum over the slices in slice order, the closest point for the winner only (the seeding
//                 run: the minimum alone)
// No atomics: a minimum with the lowest index on ties is the same for every tiling, so the outputs are bitwise independent of the
// slice count and of the culling.  Every fma of the contract is written out (the unit is compiled with -ffp-contract=off).
#include <hip/hip_runtime.h>

#include "../../include/p3d_metrics.h"
#include "p3d_metrics_plan.hpp"

#define PM_WAVE 64
#define PM_QPL (P3D_PM_QUERY_BLOCK / PM_WAVE)  // queries per lane
#define PM_PREP_WG 256
#define PM_INF __builtin_inff()

struct pm_v3 {
    float x, y, z;
};
static __device__ __forceinline__ pm_v3 pm_sub(pm_v3 u, pm_v3 v) { return {u.x - v.x, u.y - v.y, u.z - v.z}; }
static __device__ __forceinline__ float pm_dot(pm_v3 u, pm_v3 v) { return __builtin_fmaf(u.z, v.z, __builtin_fmaf(u.y, v.y, u.x * v.x)); }
static __device__ __forceinline__ pm_v3 pm_cross(pm_v3 u, pm_v3 v) {
    return {__builtin_fmaf(u.y, v.z, -(u.z * v.y)), __builtin_fmaf(u.z, v.x, -(u.x * v.z)), __builtin_fmaf(u.x, v.y, -(u.y * v.x))};
}

// the record of one face: what of the contract does not depend on the query
struct pm_rec {
    pm_v3 a, b, c, n;
    float nn, d_ab, d_bc, d_ca;
};
static __device__ __forceinline__ pm_rec pm_unpack(float4 r0, float4 r1, float4 r2, float4 r3) {
    return {{r0.x, r0.y, r0.z}, {r0.w, r1.x, r1.y}, {r1.z, r1.w, r2.x}, {r2.y, r2.z, r2.w}, r3.x, r3.y, r3.z, r3.w};
}

// seg(p; a, b) with ab, ap and den = dot(ab, ab) given; *t_out: the clamped parameter
static __device__ __forceinline__ float pm_seg(pm_v3 ab, pm_v3 ap, float den, float* t_out) {
    const float num = pm_dot(ab, ap);
    const float t = den > 0.f ? __builtin_fminf(__builtin_fmaxf(num / den, 0.f), 1.f) : 0.f;
    const pm_v3 r = {__builtin_fmaf(-t, ab.x, ap.x), __builtin_fmaf(-t, ab.y, ap.y), __builtin_fmaf(-t, ab.z, ap.z)};
    *t_out = t;
    return pm_dot(r, r);
}

// the four terms of d2(p, T); term[3] = +inf when the face term does not apply; h_out = dot(n, ap)
static __device__ __forceinline__ void pm_terms(pm_v3 p, const pm_rec& T, float term[4], float t[3], float* h_out) {
    const pm_v3 ab = pm_sub(T.b, T.a), bc = pm_sub(T.c, T.b), ca = pm_sub(T.a, T.c);
    const pm_v3 ap = pm_sub(p, T.a), bp = pm_sub(p, T.b), cp = pm_sub(p, T.c);
    term[0] = pm_seg(ab, ap, T.d_ab, &t[0]);
    term[1] = pm_seg(bc, bp, T.d_bc, &t[1]);
    term[2] = pm_seg(ca, cp, T.d_ca, &t[2]);
    float f = PM_INF, h = 0.f;
    if (T.nn > 0.f && pm_dot(pm_cross(ab, ap), T.n) > 0.f && pm_dot(pm_cross(bc, bp), T.n) > 0.f && pm_dot(pm_cross(ca, cp), T.n) > 0.f) {
        h = pm_dot(T.n, ap);
        f = (h * h) / T.nn;
    }
    term[3] = f;
    *h_out = h;
}

static __device__ __forceinline__ float pm_d2(pm_v3 p, const pm_rec& T) {
    float term[4], t[3], h;
    pm_terms(p, T, term, t, &h);
    return __builtin_fminf(__builtin_fminf(__builtin_fminf(term[0], term[1]), term[2]), term[3]);
}

static __device__ __forceinline__ float pm_wave_min(float v) {
    for (int m = PM_WAVE / 2; m >= 1; m >>= 1) v = __builtin_fminf(v, __shfl_xor(v, m, PM_WAVE));
    return v;
}
static __device__ __forceinline__ float pm_wave_max(float v) {
    for (int m = PM_WAVE / 2; m >= 1; m >>= 1) v = __builtin_fmaxf(v, __shfl_xor(v, m, PM_WAVE));
    return v;
}

// ---- prepare ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PM_PREP_WG) void k_pm_prepare(const float* __restrict__ verts, int64_t V, const int32_t* __restrict__ faces,
                                                           int64_t F, float4* __restrict__ rec, float* __restrict__ boxes,
                                                           float4* __restrict__ samples) {
    const int64_t f = (int64_t)blockIdx.x * PM_PREP_WG + threadIdx.x;  // a wave = the faces of one tile (P3D_PM_FACE_TILE == PM_WAVE)
    pm_v3 lo = {PM_INF, PM_INF, PM_INF}, hi = {-PM_INF, -PM_INF, -PM_INF};
    float edge = 0.f;
    if (f < F) {
        pm_v3 v[3];
        for (int k = 0; k < 3; ++k) {
            int64_t i = faces[3 * f + k];
            i = i < 0 ? 0 : (i >= V ? V - 1 : i);  // (the caller checks the indices; this keeps a bad one inside verts)
            v[k] = {verts[3 * i], verts[3 * i + 1], verts[3 * i + 2]};
        }
        const pm_v3 ab = pm_sub(v[1], v[0]), ac = pm_sub(v[2], v[0]), bc = pm_sub(v[2], v[1]), ca = pm_sub(v[0], v[2]);
        const pm_v3 n = pm_cross(ab, ac);
        const float nn = pm_dot(n, n), d_ab = pm_dot(ab, ab), d_bc = pm_dot(bc, bc), d_ca = pm_dot(ca, ca);
        const float4 r[4] = {make_float4(v[0].x, v[0].y, v[0].z, v[1].x), make_float4(v[1].y, v[1].z, v[2].x, v[2].y),
                             make_float4(v[2].z, n.x, n.y, n.z), make_float4(nn, d_ab, d_bc, d_ca)};
        for (int k = 0; k < 4; ++k) rec[4 * f + k] = r[k];
        if (f % P3D_PM_FACE_TILE == 0)  // the tile's first face again, packed: the mesh of the seeding run
            for (int k = 0; k < 4; ++k) samples[4 * (f / P3D_PM_FACE_TILE) + k] = r[k];
        lo = {__builtin_fminf(__builtin_fminf(v[0].x, v[1].x), v[2].x), __builtin_fminf(__builtin_fminf(v[0].y, v[1].y), v[2].y),
              __builtin_fminf(__builtin_fminf(v[0].z, v[1].z), v[2].z)};
        hi = {__builtin_fmaxf(__builtin_fmaxf(v[0].x, v[1].x), v[2].x), __builtin_fmaxf(__builtin_fmaxf(v[0].y, v[1].y), v[2].y),
              __builtin_fmaxf(__builtin_fmaxf(v[0].z, v[1].z), v[2].z)};
        edge = __builtin_fmaxf(__builtin_fmaxf(d_ab, d_bc), d_ca);
    }
    lo = {pm_wave_min(lo.x), pm_wave_min(lo.y), pm_wave_min(lo.z)};
    hi = {pm_wave_max(hi.x), pm_wave_max(hi.y), pm_wave_max(hi.z)};
    edge = pm_wave_max(edge);
    const int64_t tile = f / P3D_PM_FACE_TILE;
    if ((threadIdx.x & (PM_WAVE - 1)) == 0 && tile * P3D_PM_FACE_TILE < F) {
        float* b = boxes + PM_BOX_FLOATS * tile;
        b[0] = lo.x, b[1] = lo.y, b[2] = lo.z, b[3] = hi.x, b[4] = hi.y, b[5] = hi.z, b[6] = edge, b[7] = 0.f;
    }
}

// ---- the pair loop ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PM_WAVE) void k_pm_pairs(const float* __restrict__ points, int64_t Q, const float4* __restrict__ rec,
                                                      const float* __restrict__ boxes, int64_t F, int64_t ntiles, int64_t tiles_per_slice,
                                                      const float* __restrict__ seed, float margin,
                                                      float* __restrict__ pd2, int32_t* __restrict__ pface) {
    // boxes == NULL: no culling.  seed [Q] (with boxes): each query's smallest d2 to SOME faces of this mesh, an upper bound
    // of each query's result that every slice may cull with from its first tile on.  pface == NULL: only the distances are wanted.
    const bool cull = boxes != nullptr;
    __shared__ float4 stage[4 * P3D_PM_FACE_TILE];
    const int lane = threadIdx.x;
    const int64_t q0 = (int64_t)blockIdx.x * P3D_PM_QUERY_BLOCK + lane;
    const int64_t slice = blockIdx.y;
    const int64_t t_begin = slice * tiles_per_slice;
    const int64_t t_end = t_begin + tiles_per_slice < ntiles ? t_begin + tiles_per_slice : ntiles;

    pm_v3 p[PM_QPL];
    float best[PM_QPL], bound[PM_QPL];
    int32_t bface[PM_QPL];
#pragma unroll
    for (int k = 0; k < PM_QPL; ++k) {
        int64_t q = q0 + (int64_t)k * PM_WAVE;
        q = q < Q ? q : Q - 1;  // a lane past the end repeats the last query (never stored): no special case in the loop or in the box
        p[k] = {points[3 * q], points[3 * q + 1], points[3 * q + 2]};
        best[k] = PM_INF;
        bound[k] = cull && seed ? seed[q] : PM_INF;
        bface[k] = (int32_t)(t_begin * P3D_PM_FACE_TILE);
    }

    for (int64_t tile = t_begin; tile < t_end; ++tile) {
        if (cull) {  // skipped when NO query of the wave can find its minimum, or a tie with it, in this tile
            const float* b = boxes + PM_BOX_FLOATS * tile;
            const float slack = margin + b[6];
            int wanted = 0;
#pragma unroll
            for (int k = 0; k < PM_QPL; ++k) {
                const float gx = __builtin_fmaxf(0.f, __builtin_fmaxf(b[0] - p[k].x, p[k].x - b[3]));
                const float gy = __builtin_fmaxf(0.f, __builtin_fmaxf(b[1] - p[k].y, p[k].y - b[4]));
                const float gz = __builtin_fmaxf(0.f, __builtin_fmaxf(b[2] - p[k].z, p[k].z - b[5]));
                const float gap2 = gx * gx + gy * gy + gz * gz;  // from the query to the tile's box
                wanted |= !(gap2 > __builtin_fminf(best[k], bound[k]) + slack);  // (a bound of +inf: wanted)
            }
            if (!__any(wanted)) continue;  // wave-uniform: the workgroup is one wave
        }
        const int64_t base = 4 * P3D_PM_FACE_TILE * tile;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t i = base + lane + k * PM_WAVE;
            if (i < 4 * F) stage[lane + k * PM_WAVE] = rec[i];
        }
        __syncthreads();
        const int64_t f0 = tile * P3D_PM_FACE_TILE;
        const int nf = (int)(F - f0 < P3D_PM_FACE_TILE ? F - f0 : P3D_PM_FACE_TILE);
        for (int j = 0; j < nf; ++j) {
            const pm_rec T = pm_unpack(stage[4 * j], stage[4 * j + 1], stage[4 * j + 2], stage[4 * j + 3]);
#pragma unroll
            for (int k = 0; k < PM_QPL; ++k) {
                const float d = pm_d2(p[k], T);
                if (d < best[k]) {  // strict: faces come in ascending order, the lowest index keeps a tie
                    best[k] = d;
                    bface[k] = (int32_t)(f0 + j);
                }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < PM_QPL; ++k) {
        const int64_t q = q0 + (int64_t)k * PM_WAVE;
        if (q < Q) {
            pd2[slice * Q + q] = best[k];
            if (pface) pface[slice * Q + q] = bface[k];
        }
    }
}

// ---- the minimum over the slices, and the closest point ------------------------------------------------------------------------------
__global__ __launch_bounds__(PM_PREP_WG) void k_pm_reduce(const float* __restrict__ points, int64_t Q, const float4* __restrict__ rec,
                                                          const float* __restrict__ pd2, const int32_t* __restrict__ pface, int64_t slices,
                                                          float* __restrict__ dist2, int32_t* __restrict__ face, float* __restrict__ closest) {
    const int64_t q = (int64_t)blockIdx.x * PM_PREP_WG + threadIdx.x;
    if (q >= Q) return;
    float best = pd2[q];
    int64_t bs = 0;
    for (int64_t s = 1; s < slices; ++s) {
        const float d = pd2[s * Q + q];
        if (d < best) {  // slices hold ascending faces: strict keeps the lowest index
            best = d;
            bs = s;
        }
    }
    dist2[q] = best;
    if (!pface) return;  // (the seeding run: only the distance)
    const int32_t bf = pface[bs * Q + q];
    if (face) face[q] = bf;
    if (closest) {
        const pm_v3 p = {points[3 * q], points[3 * q + 1], points[3 * q + 2]};
        const pm_rec T = pm_unpack(rec[4 * (int64_t)bf], rec[4 * (int64_t)bf + 1], rec[4 * (int64_t)bf + 2], rec[4 * (int64_t)bf + 3]);
        float term[4], t[3], h;
        pm_terms(p, T, term, t, &h);
        const float d = __builtin_fminf(__builtin_fminf(__builtin_fminf(term[0], term[1]), term[2]), term[3]);
        pm_v3 c;
        if (term[0] == d || term[1] == d || term[2] == d) {
            const int e = term[0] == d ? 0 : (term[1] == d ? 1 : 2);
            const pm_v3 o = e == 0 ? T.a : (e == 1 ? T.b : T.c), to = e == 0 ? T.b : (e == 1 ? T.c : T.a);
            const pm_v3 dir = pm_sub(to, o);
            c = {__builtin_fmaf(t[e], dir.x, o.x), __builtin_fmaf(t[e], dir.y, o.y), __builtin_fmaf(t[e], dir.z, o.z)};
        } else {
            const float w = h / T.nn;
            c = {__builtin_fmaf(-w, T.n.x, p.x), __builtin_fmaf(-w, T.n.y, p.y), __builtin_fmaf(-w, T.n.z, p.z)};
        }
        closest[3 * q] = c.x, closest[3 * q + 1] = c.y, closest[3 * q + 2] = c.z;
    }
}

// ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
extern "C" int p3d_point_mesh_plan(int64_t Q, int64_t F, int flags, int64_t* out, int cap) {
    if (!out || cap < 6) return P3D_E_ARG;
    pm_plan p;
    const int rc = pm_make_plan(Q, F, flags, &p);
    if (rc) return rc;
    out[0] = p.qblocks, out[1] = p.ntiles, out[2] = p.slices, out[3] = p.tiles_per_slice, out[4] = P3D_PM_QUERY_BLOCK, out[5] = P3D_PM_FACE_TILE;
    return 0;
}

extern "C" size_t p3d_point_mesh_workspace_bytes(int64_t Q, int64_t F) { return pm_ws_bytes(Q, F); }

extern "C" int p3d_point_mesh_dist2_f32(const float* points, int64_t Q, const float* verts, int64_t V, const int32_t* faces, int64_t F,
                                        int flags, float cull_margin, float* dist2, int32_t* face, float* closest, void* workspace,
                                        size_t workspace_bytes, void* stream) {
    static_assert(P3D_PM_FACE_TILE == PM_WAVE && PM_PREP_WG % PM_WAVE == 0 && PM_QPL * PM_WAVE == P3D_PM_QUERY_BLOCK, "one wave per face tile");
    if (!points || !verts || !faces || !dist2 || !workspace || ((uintptr_t)workspace & 15)) return P3D_E_ARG;  // (float4 records)
    if (!(cull_margin >= 0.f) || cull_margin == PM_INF) return P3D_E_ARG;
    if (V < 1 || V > 0x7fffffffLL) return P3D_E_RANGE;
    pm_plan p;
    const int rc = pm_make_plan(Q, F, flags, &p);
    if (rc) return rc;
    if (workspace_bytes < pm_ws_bytes(Q, F)) return P3D_E_WORKSPACE;
    if (Q == 0) return 0;
    char* ws = (char*)workspace;
    float4* rec = (float4*)ws;
    float* boxes = (float*)(ws + pm_ws_boxes(F));
    float4* samples = (float4*)(ws + pm_ws_samples(F));
    float* seed = (float*)(ws + pm_ws_seed(F));
    float* pd2 = (float*)(ws + pm_ws_pd2(Q, F));
    int32_t* pface = (int32_t*)(ws + pm_ws_pface(Q, F));
    const hipStream_t st = (hipStream_t)stream;
    const unsigned prep = (unsigned)((p.ntiles * P3D_PM_FACE_TILE + PM_PREP_WG - 1) / PM_PREP_WG);
    hipLaunchKernelGGL(k_pm_prepare, dim3(prep), dim3(PM_PREP_WG), 0, st, verts, V, faces, F, rec, boxes, samples);
    const bool cull = !(flags & P3D_PM_NO_CULL);
    pm_plan sp;  // the seeding run: the sample records as a mesh of ntiles faces, the plan's own slice count
    if (cull) {
        const int src = pm_make_plan(Q, p.ntiles, 0, &sp);
        if (src) return src;
        hipLaunchKernelGGL(k_pm_pairs, dim3((unsigned)sp.qblocks, (unsigned)sp.slices), dim3(PM_WAVE), 0, st, points, Q, (const float4*)samples,
                           (const float*)nullptr, p.ntiles, sp.ntiles, sp.tiles_per_slice, (const float*)nullptr, 0.f, pd2,
                           (int32_t*)nullptr);  // (its partials borrow the main run's array, which is written after they are reduced)
        hipLaunchKernelGGL(k_pm_reduce, dim3((unsigned)((Q + PM_PREP_WG - 1) / PM_PREP_WG)), dim3(PM_PREP_WG), 0, st, points, Q, (const float4*)samples,
                           (const float*)pd2, (const int32_t*)nullptr, sp.slices, seed, (int32_t*)nullptr, (float*)nullptr);
    }
    hipLaunchKernelGGL(k_pm_pairs, dim3((unsigned)p.qblocks, (unsigned)p.slices), dim3(PM_WAVE), 0, st, points, Q, (const float4*)rec,
                       cull ? (const float*)boxes : (const float*)nullptr, F, p.ntiles, p.tiles_per_slice, cull ? (const float*)seed : (const float*)nullptr,
                       cull_margin, pd2, pface);
    hipLaunchKernelGGL(k_pm_reduce, dim3((unsigned)((Q + PM_PREP_WG - 1) / PM_PREP_WG)), dim3(PM_PREP_WG), 0, st, points, Q, (const float4*)rec,
                       (const float*)pd2, (const int32_t*)pface, p.slices, dist2, face, closest);
    return (int)hipGetLastError();
}
