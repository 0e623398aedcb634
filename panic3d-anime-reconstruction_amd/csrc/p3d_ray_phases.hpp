// p3d_ray_phases.hpp — the per-ray phases of ImportanceRenderer.forward, each defined ONCE (device only, force-inlined, the
// operation sequence of the arithmetic contract, include/p3d_numerics.h, kept literally).  k_render, k_render_slots, the stand-alone
// stage kernels (p3d_kernels.hip) and the backward's forward sweep (p3d_render_grad.hip) call these; the schedules around them
// (who decodes what, when) stay in the kernels.  In the order a ray goes through them: tile -> ray, wave set-up (P3dRayCtx),
// stratified depths (P3dSpacing), crop test, marcher interval (MarchState), weights -> pdf -> cdf, inverse-CDF draws (what the two
// lane halves share out: p3d_importance.hpp), guards + compositing (P3dAccum), per-ray outputs, depth range.
// RenderParams, the launch parameters the host side of p3d_kernels.hip fills, is declared here because the tile functions, the
// set-up and the outputs read it (p3d_render_grad.hip, which includes this header for the marcher interval, does not use it).
#pragma once
#include "p3d_decode.hpp"
#include "p3d_importance.hpp"
#include "p3d_render_plan.hpp"

struct RenderParams {
    const float* planes;  // [N][3][H][W][32]
    const float *rays_o, *rays_d;  // [N][R][3]
    const float* jitter;  // [N][R][Sc]
    const float* u;       // [N*R][Sf]
    const float *w0, *b0, *w1, *b1;
    float *out_feat, *out_depth, *out_wsum, *out_xyz;
    uint32_t* gminmax;  // [0..1] order-mapped min / max of all depths, [2..3] decode-step count, [4 + 2n ..] per-view min / max
    int per_view_clamp;  // P3D_FLAG_PER_VIEW_CLAMP: the N views are N calls of the reference -> one clamp range each
    p3d_dumps dumps;
    long long R;
    long long tiles_per_img, ntiles;
    int tile_w;       // >0: 8x4 screen tiles over a tile_w-wide image
    int tiles_x;      // tile_w / 8
    int H, W;
    int Sc, Sf;
    float ray_start, ray_end, depth_delta;
    const float *ray_start_arr, *ray_end_arr;  // per-ray limits [N][R] ('auto', renderer.py:165-171) or null
    int disparity;                             // P3D_FLAG_DISPARITY
    int white_back;
    int lds_rows;     // rows (of 32 floats) of per-wave LDS
    int rng;          // p3d_render_rng_f32: the two draws come from the counter-based generator of include/p3d_numerics.h
    uint32_t seed_lo, seed_hi;
    int wide_rows;    // k_render: P3D_WIDE_JITTER | P3D_WIDE_U, the rows it may load as 16-byte pieces (p3d_render_wide_rows)
    int serial_merge;  // P3D_FLAG_SERIAL_MERGE: k_render's merge pre-pass walks the merged list also where it would search by rank
    P3dTileOrder order;  // k_render: the XCD tile order (p3d_render_plan.hpp)
    P3dDecodeCfg cfg;
};

// The 32-ray tile of wave `wave` of this block in k_render, after the XCD-aware block swizzle: hardware places block b on XCD
// b % 8; give each XCD a contiguous range of tiles so that the plane texels its rays touch stay in that XCD's L2.
// Each XCD gets runs of consecutive blocks: contiguous enough for L2 reuse, fine enough that the XCDs finish together although
// the early-outs make the work per tile uneven.  The orders themselves: p3d_tile_of_block / p3d_tile_screen (p3d_render_plan.hpp),
// which the host evaluates too.
P3D_DEV long long p3d_render_wave_tile(const RenderParams& p, int wave) {
    return p3d_tile_of_block(p.order, gridDim.x, blockIdx.x, blockDim.x >> 6, wave, p.tiles_x, p.tiles_per_img);
}

struct P3dTileRay { long long n, r; };  // view, ray of the view (may lie past the last ray: the caller clamps)

// lane j's ray of k_render's tile
P3D_DEV P3dTileRay p3d_render_tile_ray(const RenderParams& p, long long tile, int j) {
    P3dTileRay o;
    if (p.tile_w > 0) {
        const P3dTileXY t = p3d_tile_screen(p.order, tile, p.tiles_x, p.tiles_per_img);
        o.n = t.n;
        // 8x4 pixel tile in Morton-like lane order: every lane quad is a 2x2 pixel block, so the quad's four gathers of a
        // tap fall into 1-2 cache lines (the L1 coalesces within a quad; rocprof: TCP accesses/instr 48 -> see DESIGN.md)
        const int lx = (j & 1) | ((j >> 1) & 6), ly = ((j >> 1) & 1) | ((j >> 3) & 2);
        o.r = (t.ty * 4 + ly) * p.tile_w + t.tx * 8 + lx;
    } else {
        o.n = tile / p.tiles_per_img;
        o.r = (tile - o.n * p.tiles_per_img) * 32 + j;
    }
    return o;
}

// ray jr of k_render_slots' tile: 4 x (RPW / 4) pixels, Morton lane order (a lane quad = a 2x2 pixel block: the quad-cooperative gathers)
template <int RPW>
P3D_DEV P3dTileRay p3d_slots_tile_ray(const RenderParams& p, long long tile, int jr) {
    P3dTileRay o;
    o.n = tile / p.tiles_per_img;
    const long long tl = tile - o.n * p.tiles_per_img;
    if (p.tile_w > 0) {
        long long ty = tl / p.tiles_x, tx = tl - ty * p.tiles_x;
        const int lx = (jr & 1) | ((jr >> 1) & 2), ly = ((jr >> 1) & 1) | ((jr >> 2) & 2);
        o.r = (ty * (RPW / 4) + ly) * p.tile_w + tx * 4 + lx;
    } else {
        o.r = tl * RPW + jr;
    }
    return o;
}

// The counter-based generator of p3d_render_rng_f32 (include/p3d_numerics.h "device draws"): stream 0 = the jitter of
// sample_stratified (renderer.py:324), stream 1 = the u of sample_pdf (:371); a pure function of (seed, stream, ray, index).
P3D_DEV uint32_t p3d_fmix32(uint32_t h) {
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}
P3D_DEV float p3d_draw(uint32_t seed_lo, uint32_t seed_hi, uint32_t stream, size_t ray, int idx) {
    uint32_t h = p3d_fmix32(seed_lo ^ ((uint32_t)ray * 0x9E3779B1u));
    h = p3d_fmix32(h ^ seed_hi ^ ((uint32_t)((unsigned long long)ray >> 32) * 0x7FEB352Du) ^ (((uint32_t)idx * 2u + stream) * 0x846CA68Bu));
    return (float)(h >> 8) * 0x1p-24f;  // 24 random bits in [0, 1): exact in binary32
}

// crop by POSITION (triplane_crop, renderer.py:138-149): such a sample's sigma is -1000 whatever the network says.
// (flag and limit by REFERENCE, as the kernels' lambdas captured them: by value, k_render_slots<4, 96, tolerance> spilled 110 VGPRs
// instead of 30)
P3D_DEV bool p3d_crop_xz(const bool& f_crop, const float& crop_limit, float px, float pz) {
    return f_crop && (__builtin_fabsf(px) > crop_limit || __builtin_fabsf(pz) > crop_limit);
}

typedef decltype(__builtin_amdgcn_make_buffer_rsrc((void*)nullptr, (short)0, 0, 0)) p3d_rsrc_t;

// What a lane knows of its ray before the first phase; n is wave-uniform (a tile never straddles two views).
struct P3dRayCtx {
    bool active;   // r < R; an inactive lane works on the view's last ray and stores nothing
    size_t ray;    // n * R + min(r, R - 1)
    unsigned nlo;  // the view, wave-uniform (an SGPR)
    P3dPlaneGeom g;
    p3d_rsrc_t rs;  // the view's three planes (P3D_FLAG_SHARED_PLANES: image 0's)
    P3dDecodeCfg cfg;
    bool f_crop;
    float ox, oy, oz, dx, dy, dz;
    int rng;
    uint32_t seed_lo, seed_hi;
    const float *jit, *uu;  // the ray's rows of the jitter / u tensors (not dereferenced with the in-kernel generator)
    P3D_DEV float jitter(int i) const { return rng ? p3d_draw(seed_lo, seed_hi, 0u, ray, i) : jit[i]; }
    P3D_DEV float u(int i) const { return rng ? p3d_draw(seed_lo, seed_hi, 1u, ray, i) : uu[i]; }
    P3D_DEV bool cropped(float px, float pz) const { return p3d_crop_xz(f_crop, cfg.crop_limit, px, pz); }
    P3D_DEV bool cropped_at(float t) const { return cropped(ox + t * dx, oz + t * dz); }
};

P3D_DEV P3dRayCtx p3d_ray_setup(const RenderParams& p, P3dTileRay tr, int Sc, int Sf) {
    P3dRayCtx c;
    c.active = tr.r < p.R;
    const long long rc = c.active ? tr.r : p.R - 1;
    c.ray = (size_t)tr.n * p.R + rc;
    c.g.halfW = 0.5f * (float)p.W; c.g.halfH = 0.5f * (float)p.H; c.g.fW = (float)p.W; c.g.fH = (float)p.H; c.g.W = p.W;
    c.g.plane_bytes = (uint32_t)p.H * (uint32_t)p.W * 128u;
    c.nlo = __builtin_amdgcn_readfirstlane((unsigned)tr.n);
    const float* pbase = p.planes + ((p.cfg.flags & P3D_FLAG_SHARED_PLANES) ? (size_t)0 : (size_t)c.nlo * 3 * (c.g.plane_bytes / 4));
    c.rs = __builtin_amdgcn_make_buffer_rsrc((void*)pbase, 0, 3 * c.g.plane_bytes, 0x00020000);
    c.cfg = p.cfg;
    c.f_crop = (c.cfg.flags & P3D_FLAG_CROP) != 0;
    c.ox = p.rays_o[c.ray * 3]; c.oy = p.rays_o[c.ray * 3 + 1]; c.oz = p.rays_o[c.ray * 3 + 2];
    c.dx = p.rays_d[c.ray * 3]; c.dy = p.rays_d[c.ray * 3 + 1]; c.dz = p.rays_d[c.ray * 3 + 2];
    c.rng = p.rng; c.seed_lo = p.seed_lo; c.seed_hi = p.seed_hi;
    c.jit = p.jitter + c.ray * Sc;
    c.uu = p.u + c.ray * Sf;
    return c;
}

// ---- sample_stratified: renderer.py:309-326 ------------------------------------------------------------------------------------
struct P3dSpacing {
    float ray_start, ray_end, depth_delta, step;  // fixed limits (disparity: ray_start / ray_end hold the reciprocals)
    bool limits;                                  // per-ray limits (ray_start = ray_end = 'auto'): math_utils.linspace + per-ray depth_delta (:317-319)
    float rs, span, rdelta;
    bool disparity;                               // uniform in 1 / depth (:309-316)
};
P3D_DEV P3dSpacing p3d_spacing_fixed(float ray_start, float ray_end, float depth_delta, int Sc) {
    return {ray_start, ray_end, depth_delta, (ray_end - ray_start) / (float)(Sc - 1), false, 0.0f, 0.0f, 0.0f, false};
}
// filled once per ray
P3D_DEV P3dSpacing p3d_spacing_of(const RenderParams& p, size_t ray, int Sc) {
    P3dSpacing s = p3d_spacing_fixed(p.ray_start, p.ray_end, p.depth_delta, Sc);
    s.limits = p.ray_start_arr != nullptr;
    s.rs = s.limits ? p.ray_start_arr[ray] : 0.0f;
    s.span = s.limits ? p.ray_end_arr[ray] - s.rs : 0.0f;
    s.rdelta = s.span / (float)(Sc - 1);
    s.disparity = p.disparity != 0;
    return s;
}
// coarse sample i of the fixed spacing from its jitter value jv (:320-326): linspace from both ends, as torch computes it
P3D_DEV float p3d_stratified_fixed(int i, int Sc, float jv, const P3dSpacing& s) {
    const float lin = (i < Sc / 2) ? p3d_fma(s.step, (float)i, s.ray_start) : p3d_fma(-s.step, (float)(Sc - 1 - i), s.ray_end);
    return lin + jv * s.depth_delta;
}
// ... of whichever spacing the launch asked for
P3D_DEV float p3d_stratified_depth(int i, int Sc, float jv, const P3dSpacing& s) {
    float t = p3d_stratified_fixed(i, Sc, jv, s);
    if (s.limits) {  // wave-uniform
        const float prod = ((float)i / (float)(Sc - 1)) * s.span;
        t = (s.rs + prod) + jv * s.rdelta;
    } else if (s.disparity) {
        const float s01 = 1.0f / (float)(Sc - 1);
        const float l01 = (i < Sc / 2) ? p3d_fma(s01, (float)i, 0.0f) : p3d_fma(-s01, (float)(Sc - 1 - i), 1.0f);
        const float dd = l01 + jv * s.depth_delta;
        const float ta_ = s.ray_start * (1.0f - dd), tb_ = s.ray_end * dd;
        t = 1.0f / (ta_ + tb_);
    }
    return t;
}

// ---- MipRayMarcher2: ray_marcher.py:25-57 --------------------------------------------------------------------------------------
// per-ray running state
struct MarchState {
    double Td;
    float W, D;
    float prev_t, prev_sigma;
};
P3D_DEV MarchState p3d_march_start(float t0 = 0.0f, float sigma0 = 0.0f) { return {1.0, 0.0f, 0.0f, t0, sigma0}; }
struct P3dInterval { float w, tm, alpha, T; };  // weight, mid depth, opacity, transmittance in front of it
// interval (prev, cur); advances the transmittance (binary64), not prev_t / prev_sigma.  ray_marcher.py:26-42
P3D_DEV P3dInterval p3d_march_interval(MarchState& st, float t, float sigma) {
    P3dInterval iv;
    float dl = t - st.prev_t;
    float sm = (st.prev_sigma + sigma) * 0.5f;
    iv.tm = (st.prev_t + t) * 0.5f;
    float rho = p3d_softplus(sm - 1.0f);
    float dd = rho * dl;
    iv.alpha = 1.0f - p3d_exp(-dd);
    iv.T = (float)st.Td;
    iv.w = iv.alpha * iv.T;
    st.Td = st.Td * (double)((1.0f - iv.alpha) + 1e-10f);
    return iv;
}
// weights.sum and the depth numerator: ray_marcher.py:43-46
P3D_DEV void p3d_march_accumulate(MarchState& st, const P3dInterval& iv) {
    st.W = st.W + iv.w;
    st.D = p3d_fma(iv.w, iv.tm, st.D);
}

// ---- sample_importance: weights -> smoothed pdf -> cdf, renderer.py:328-370 ----------------------------------------------------
// v[jj] = ws[jj+1] + 1e-5, ws[q] = (max(w[q-1],w[q]) + max(w[q],w[q+1])) * 0.5 + 0.01, from the three weights around bin jj
P3D_DEV float p3d_pdf_bin(float wa, float wb, float wc) {
    float m1 = __builtin_fmaxf(wa, wb), m2 = __builtin_fmaxf(wb, wc);
    return ((m1 + m2) * 0.5f + 0.01f) + 1e-5f;
}
// cdf entry behind bin value v: the pdf is v / (float)sum, accumulated in binary64
P3D_DEV float p3d_cdf_step(double& acc, float v, float fsum) {
    float pdf = v / fsum;
    acc += (double)pdf;
    return (float)acc;
}
// In place on column j of an LDS array of row stride RS: rows [0, Sc - 1) hold the coarse weights, afterwards rows [0, Ns] the
// cdf (row 0 = 0).  The order of the two binary64 sums is the contract.
template <int RS>
P3D_DEV void p3d_pdf_to_cdf(float* A, int Ns, int j) {
    double sum = 0.0;
    float wa = A[0 * RS + j], wb = A[1 * RS + j];
    for (int jj = 0; jj < Ns; ++jj) {
        float wc = A[(jj + 2) * RS + j];
        float v = p3d_pdf_bin(wa, wb, wc);
        sum += (double)v;
        A[(jj + 1) * RS + j] = v;
        wa = wb; wb = wc;
    }
    float fsum = (float)sum;
    double acc = 0.0;
    A[j] = 0.0f;  // cdf[0]
    for (int jj = 0; jj < Ns; ++jj) A[(jj + 1) * RS + j] = p3d_cdf_step(acc, A[(jj + 1) * RS + j], fsum);  // cdf[jj+1]
}

// ---- sample_pdf: renderer.py:371-386 ---------------------------------------------------------------------------------------------
// B independent inverse-CDF draws.  cdf rows [0, Ns] of the LDS column j (RS floats per row); the coarse
// depths, rows [0, Sc), behind a functor tc(index): an LDS column, or in k_render's TCG instantiations recomputed from the jitter
// tensor.  The B LDS reads of every search step are in flight together (one draw is a chain of 8 dependent LDS round trips; 48 of
// them back to back were ~9 % of k_render).
template <int B, int RS, typename TCF>
P3D_DEV void p3d_inverse_cdf(const float* cdfA, TCF tc, int Ns, int j, const float (&ui)[B], float (&out)[B], int (&k_out)[B]) {
    // k = #{q in 0..Ns : cdf[q] <= u}  (searchsorted right=True): branchless binary search on the non-decreasing cdf
    const int n = Ns + 1;
    int pos[B];
#pragma unroll
    for (int q = 0; q < B; ++q) pos[q] = 0;
#pragma unroll
    for (int step = 128; step >= 1; step >>= 1) {
        if (step <= n) {  // wave-uniform
            float c[B];
#pragma unroll
            for (int q = 0; q < B; ++q) c[q] = cdfA[((pos[q] + step <= n) ? pos[q] + step - 1 : 0) * RS + j];
#pragma unroll
            for (int q = 0; q < B; ++q) pos[q] = ((pos[q] + step <= n) && (c[q] <= ui[q])) ? pos[q] + step : pos[q];
        }
    }
    float cb[B], ca[B], t0[B], t1[B], t2[B], t3[B];
#pragma unroll
    for (int q = 0; q < B; ++q) {
        const int k = pos[q], below = k - 1 > 0 ? k - 1 : 0, above = k < Ns ? k : Ns;
        k_out[q] = k;
        cb[q] = cdfA[below * RS + j]; ca[q] = cdfA[above * RS + j];
        t0[q] = tc(below); t1[q] = tc(below + 1);
        t2[q] = tc(above); t3[q] = tc(above + 1);
    }
#pragma unroll
    for (int q = 0; q < B; ++q) {
        float den = ca[q] - cb[q];
        if (den < 1e-5f) den = 1.0f;
        const float bb = 0.5f * (t0[q] + t1[q]), ba = 0.5f * (t2[q] + t3[q]);
        out[q] = bb + ((ui[q] - cb[q]) / den) * (ba - bb);
        // the result exists HERE: without this the optimiser sinks the lerp (and keeps its six LDS operands alive) down to the
        // first use — the sorting network behind the last batch: 6 x Sf live values, 82-169 spilled VGPRs in the NF = 48 / 96 kernels
        asm volatile("" : "+v"(out[q]));
    }
}

#define P3D_DRAW_BATCH 8  // draws in flight

// insertion sort of rows [0, n) of a per-wave LDS column (generic / rare path)
template <int RS = 32>  // RS: floats per LDS row (the rays of a wave: 32 in k_render, 32 / SLOTS in k_render_slots)
P3D_DEV void p3d_lds_insertion_sort(float* A, int n, int j) {
    for (int i = 1; i < n; ++i) {
        float key = A[i * RS + j];
        int q = i - 1;
        while (q >= 0) {
            float v = A[q * RS + j];
            if (!(v > key)) break;
            A[(q + 1) * RS + j] = v;
            --q;
        }
        A[(q + 1) * RS + j] = key;
    }
}

// ---- final pass: guards, compositing, outputs ----------------------------------------------------------------------------------
// Exactness guard of the early-outs: an interval endpoint that went without a decode has no colour; if the interval's exact weight
// w is non-zero after all (sigma of the neighbour >= ~794) it is decoded now.  Wave-level: every lane must reach this call.
template <bool FAST>
P3D_DEV void p3d_guard_colours(const float* lds, const P3dRayCtx& cx, bool marching, float w, bool& prev_skipped, f32x16& prev_rgb,
                               float ppx, float ppy, float ppz, bool& skipped, f32x16& rgb, float px, float py, float pz) {
    if (__builtin_amdgcn_ballot_w64(marching && prev_skipped && w != 0.0f) != 0) {
        float s2;
        f32x16 c2;
        if constexpr (FAST) p3d_decode_wave_fast<true, true>(lds, cx.rs, cx.g, cx.cfg, ppx, ppy, ppz, s2, c2);
        else p3d_decode_wave<true>(lds, cx.rs, cx.g, cx.cfg, ppx, ppy, ppz, s2, c2);
        if (prev_skipped) prev_rgb = c2;
        prev_skipped = false;
    }
    if (__builtin_amdgcn_ballot_w64(marching && skipped && w != 0.0f) != 0) {
        float s2;
        if constexpr (FAST) p3d_decode_wave_fast<true, true>(lds, cx.rs, cx.g, cx.cfg, px, py, pz, s2, rgb);
        else p3d_decode_wave<true>(lds, cx.rs, cx.g, cx.cfg, px, py, pz, s2, rgb);
        skipped = false;
    }
}

// the composited [rgb | xyz] of a lane: 16 of the 32 feature channels (its channel half) and the position
struct P3dAccum {
    f32x16 C = 0.0f;
    float Cx = 0.0f, Cy = 0.0f, Cz = 0.0f;
};
// one channel of one interval: weight x mid value of its two endpoints (ray_marcher.py:30, :44)
P3D_DEV float p3d_composite_channel(float w, float a, float b, float acc) { return p3d_fma(w, (a + b) * 0.5f, acc); }
// one interval into the lane's accumulators; WO (weights only): W and D alone
template <bool WO>
P3D_DEV void p3d_composite_interval(P3dAccum& a, MarchState& st, const P3dInterval& iv, const f32x16& prev_rgb, const f32x16& rgb,
                                    float ppx, float ppy, float ppz, float px, float py, float pz) {
    if constexpr (!WO) {
#pragma unroll
        for (int c = 0; c < 16; ++c) a.C[c] = p3d_composite_channel(iv.w, prev_rgb[c], rgb[c], a.C[c]);
        a.Cx = p3d_composite_channel(iv.w, ppx, px, a.Cx);
        a.Cy = p3d_composite_channel(iv.w, ppy, py, a.Cy);
        a.Cz = p3d_composite_channel(iv.w, ppz, pz, a.Cz);
    }
    p3d_march_accumulate(st, iv);
}

// depth of a ray: nan_to_num(D / W, nan=inf), ray_marcher.py:49 (the clamp to the global range: k_render_finish)
P3D_DEV float p3d_ray_depth(const MarchState& st) {
    float d = st.D / st.W;
    if (d != d) d = __builtin_inff();
    return d;
}
// white_back and the [-1,1] rescale of one composited channel: ray_marcher.py:52-55
P3D_DEV float p3d_white_back_rescale(float v, int white_back, float Wt) {
    if (white_back) v = (v + 1.0f) - Wt;
    return v * 2.0f - 1.0f;
}
// The stores of a ray by its `writer` lanes: 16 feature channels per channel half h as 16-byte stores (register r holds channel
// rowof(r) + 4h, p3d_decode.hpp), half 0 the three scalar outputs.  WO: depth and wsum only.
template <bool WO, bool DUMP>
P3D_DEV void p3d_ray_outputs(const RenderParams& p, size_t ray, int h, bool writer, P3dAccum a, const MarchState& st) {
    const float Wt = st.W;
    const float d = p3d_ray_depth(st);
#pragma unroll
    for (int c = 0; c < 16; ++c) a.C[c] = p3d_white_back_rescale(a.C[c], p.white_back, Wt);
    a.Cx = p3d_white_back_rescale(a.Cx, p.white_back, Wt);
    a.Cy = p3d_white_back_rescale(a.Cy, p.white_back, Wt);
    a.Cz = p3d_white_back_rescale(a.Cz, p.white_back, Wt);
    if (writer) {
        if constexpr (!WO) {
            float* dst = p.out_feat + ray * 32 + 4 * h;
#pragma unroll
            for (int q = 0; q < 4; ++q) *(f32x4*)(dst + 8 * q) = (f32x4){a.C[4 * q], a.C[4 * q + 1], a.C[4 * q + 2], a.C[4 * q + 3]};
        }
        if (h == 0) {
            p.out_depth[ray] = d;  // clamped by k_render_finish
            p.out_wsum[ray] = Wt;  // weights.sum(2): renderer.py:264
            if constexpr (!WO) { p.out_xyz[ray * 3] = a.Cx; p.out_xyz[ray * 3 + 1] = a.Cy; p.out_xyz[ray * 3 + 2] = a.Cz; }
            if constexpr (DUMP) if (p.dumps.depth_unclamped) p.dumps.depth_unclamped[ray] = st.D / Wt;
        }
    }
}

// ---- global min / max of all depths of the call (torch.min/max(depths): ray_marcher.py:50) -------------------------------------
// every lane ends with the wave's extrema; a lane that is not `active` contributes nothing
P3D_DEV void p3d_wave_minmax(bool active, float& lo, float& hi) {
    if (!active) { lo = __builtin_inff(); hi = -__builtin_inff(); }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        lo = __builtin_fminf(lo, __shfl_xor(lo, o));
        hi = __builtin_fmaxf(hi, __shfl_xor(hi, o));
    }
}
// lane 0 folds them into the call's range, the view's (a tile never straddles two views) and, COUNT, the launch's decode steps
template <bool COUNT>
P3D_DEV void p3d_depth_range_atomics(const RenderParams& p, unsigned nlo, int lane, float tmin, float tmax, int ndec) {
    if (lane == 0) {
        atomicMin(p.gminmax, p3d_f2ord(tmin));
        atomicMax(p.gminmax + 1, p3d_f2ord(tmax));
        if (p.per_view_clamp) {
            atomicMin(p.gminmax + 4 + 2 * nlo, p3d_f2ord(tmin));
            atomicMax(p.gminmax + 5 + 2 * nlo, p3d_f2ord(tmax));
        }
        if constexpr (COUNT) atomicAdd((unsigned long long*)(p.gminmax + 2), (unsigned long long)ndec);  // wave-level decode steps
    }
}
