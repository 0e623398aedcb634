// p3d_render_grad.hip — backward passes of the fused renderer and of the point decode (include/p3d_render_grad.h).
//
// Render backward, four launches after a small depth-range pass:
//   k_g_range       per-call / per-view min and max of the merged depths (the depth clamp of ray_marcher.py:49-50);
//   k_g_decode      one lane per merged sample: exact-contract re-decode -> the density the forward composited, whether a mask
//                   overwrote it, and s_i = <g_feat, c_i> + <g_xyz, p_i> (the only way a sample's colour enters the weight gradient);
//   k_g_ray         one lane per ray: the forward's weights again (p3d_march_interval, the forward's own), then the alpha recursion
//                   back to front -> per sample the density gradient (zero where masked) and the colour coefficient w_{i-1} + w_i;
//   k_g_mlp         one lane per sample, one wave per workgroup, 64 samples per step: re-decode, MLP backward, the decoder
//                   gradient as a per-workgroup partial slab (fixed order: reproducible), the plane gradient as 256-byte
//                   global_atomic_add_f32 wave instructions (two taps x 32 channels);
//   k_g_reduce      the slabs summed in a fixed order into the four decoder gradients.
// The point backward (run_model) is k_g_mlp + k_g_reduce on the caller's cotangents.
//
// Workspace layout (p3d_render_backward_workspace_bytes): [0, 256) statistics (u64 executed samples), then the depth ranges
// (order-mapped u32 min / max: the call, then one pair per view), then four f32 arrays and one byte array [S][N*R] (sample-major:
// consecutive lanes are consecutive rays), then the slabs.
#include "p3d_decode_grad.hpp"
#include "p3d_ray_phases.hpp"
#include "../../include/p3d_render_grad.h"

#define G_WG 64                      // one wave per workgroup
#define G_SLOTS 67                   // decoder-gradient slots per lane: 64 * 67 = 4288 >= 2048 + 64 + 2112 + 33
#define G_SLAB (G_WG * G_SLOTS)      // floats per workgroup slab
#define G_NPARAM (2048 + 64 + 2112 + 33)
#define G_MAX_BLOCKS 1024            // k_g_mlp grid cap = slab count (4 resident per CU at 481 registers); fixed per size: fixed reduction order
#define G_ROW 65                     // LDS row pitch of 64-wide rows (odd: conflict-free lane-per-row writes)
#define G_ROW33 33
#define G_LDS_FLOATS (64 * G_ROW33 + 64 * G_ROW)

static inline size_t g_align(size_t b) { return (b + 255) & ~(size_t)255; }

static int64_t g_blocks(int64_t samples) {
    const int64_t chunks = (samples + G_WG - 1) / G_WG;
    return chunks < G_MAX_BLOCKS ? (chunks > 0 ? chunks : 1) : G_MAX_BLOCKS;
}

// ---- the shared MLP backward + scatter ---------------------------------------------------------------------------------------
struct GCommon {
    const float* planes;
    float* dplanes;
    int H, W;
    int64_t img_floats;  // 3 * H * W * 32
    const float *w0, *b0, *w1, *b1;
    p3d_opts o;
    float* slab;
    unsigned long long* executed;
    int64_t total;  // samples
};

// What k_g_mlp needs of one sample: where it is, which image, its density gradient and the colour gradient's source.
struct GSample {
    float px, py, pz;
    int img;
    float dsig;       // before masking
    bool live;        // false: the whole gradient is exactly zero (skip)
};

struct GRenderSrc {
    const float *depths, *rays_o, *rays_d, *g_feat;
    const float *dsig, *coef;  // workspace arrays [S][NR]
    int64_t NR, R;
    int S;
    bool shared;
    P3D_DEV GSample get(int64_t g) const {
        GSample s;
        const int64_t i = g / NR, r = g - i * NR;
        s.dsig = dsig[g];
        const float a = coef[g];
        s.live = (s.dsig != 0.0f) || (a != 0.0f);
        const float t = depths[r * S + i];
        s.px = rays_o[3 * r] + t * rays_d[3 * r];  // renderer.py:179 (mul, then add)
        s.py = rays_o[3 * r + 1] + t * rays_d[3 * r + 1];
        s.pz = rays_o[3 * r + 2] + t * rays_d[3 * r + 2];
        s.img = shared ? 0 : (int)(r / R);
        return s;
    }
    P3D_DEV void dcolor(int64_t g, float dc[P3D_C]) const {  // colour gradient: (w_{i-1} + w_i) * g_feat
        const int64_t i = g / NR, r = g - i * NR;
        const float a = coef[g];
#pragma unroll
        for (int k = 0; k < P3D_C; ++k) dc[k] = (a != 0.0f) ? a * g_feat[r * P3D_C + k] : 0.0f;
    }
};

struct GPointSrc {
    const float *coords, *g_sigma, *g_rgb;
    int64_t M;
    bool shared;
    P3D_DEV GSample get(int64_t g) const {
        GSample s;
        s.px = coords[3 * g];
        s.py = coords[3 * g + 1];
        s.pz = coords[3 * g + 2];
        s.img = shared ? 0 : (int)(g / M);
        s.dsig = g_sigma ? g_sigma[g] : 0.0f;
        bool any = s.dsig != 0.0f;
        if (g_rgb && !any)
            for (int k = 0; k < P3D_C; ++k) any = any || (g_rgb[g * P3D_C + k] != 0.0f);
        s.live = any;
        return s;
    }
    P3D_DEV void dcolor(int64_t g, float dc[P3D_C]) const {
#pragma unroll
        for (int k = 0; k < P3D_C; ++k) dc[k] = g_rgb ? g_rgb[g * P3D_C + k] : 0.0f;
    }
};

template <typename SRC>
__global__ __launch_bounds__(G_WG) void k_g_mlp(GCommon c, SRC src) {
    __shared__ float lds[G_LDS_FLOATS];
    float* rowA = lds;                  // [64][33]: dO, then X, then dX
    float* rowB = lds + 64 * G_ROW33;   // [64][65]: h, then dpre, then the tap table
    __shared__ int live_s[G_WG];
    const int lane = threadIdx.x;
    float acc[G_SLOTS];
#pragma unroll
    for (int k = 0; k < G_SLOTS; ++k) acc[k] = 0.0f;
    const bool fsig = (c.o.flags & P3D_FLAG_FORCE_SIGMOID) != 0;
    unsigned long long executed = 0;
    const int64_t chunks = (c.total + G_WG - 1) / G_WG;
    for (int64_t ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
        const int64_t g = ch * G_WG + lane;
        GSample s;
        s.live = false;
        if (g < c.total) s = src.get(g);
        const uint64_t ballot = __ballot(s.live);
        if (ballot == 0) continue;  // uniform: nothing in this step carries gradient
        executed += __builtin_popcountll(ballot);
        live_s[lane] = s.live ? 1 : 0;
        P3dGradTaps tp;
        float X[P3D_C], pre[P3D_HID], h[P3D_HID], dO[P3D_HID / 2 + 1];
        if (s.live) {
            const float* img = c.planes + (int64_t)s.img * c.img_floats;
            p3d_g_taps(c.H, c.W, c.o.coord_scale, c.o.plane_mode, s.px, s.py, s.pz, tp);
            p3d_g_features(img, tp, X);
            p3d_g_hidden(c.w0, c.b0, X, pre, h);
            bool masked;
            p3d_g_masks(p3d_g_out_row(c.w1, c.b1, 0, h), s.px, s.pz, c.o, &masked);
            dO[0] = masked ? 0.0f : s.dsig;  // the reference writes a constant into masked slots: no gradient
            float dc[P3D_C];
            src.dcolor(g, dc);
#pragma unroll
            for (int k = 1; k <= P3D_C; ++k) {
                float d = 0.0f;
                if (dc[k - 1] != 0.0f) {
                    const float sg = p3d_sigmoid(p3d_g_out_row(c.w1, c.b1, k, h));
                    d = dc[k - 1] * (fsig ? 1.0f : 1.002f) * (sg * (1.0f - sg));  // sigmoid (* 1.002 - 0.001) backward
                }
                dO[k] = d;
            }
        } else {
#pragma unroll
            for (int k = 0; k <= P3D_C; ++k) dO[k] = 0.0f;
#pragma unroll
            for (int n = 0; n < P3D_HID; ++n) h[n] = pre[n] = 0.0f;
#pragma unroll
            for (int k = 0; k < P3D_C; ++k) X[k] = 0.0f;
#pragma unroll
            for (int k = 0; k < 12; ++k) {
                tp.off[k] = P3D_G_NOTAP;
                tp.wt[k] = 0.0f;
            }
        }
        // phase 1: d w1 [33][64] += dO (x) h, d b1 += dO   (slots 33..65: row k - 33, column lane; slot 66: b1[lane])
#pragma unroll
        for (int k = 0; k <= P3D_C; ++k) rowA[lane * G_ROW33 + k] = dO[k];
#pragma unroll
        for (int n = 0; n < P3D_HID; ++n) rowB[lane * G_ROW + n] = h[n];
        __syncthreads();
        for (int q = 0; q < G_WG; ++q) {
            if (!live_s[q]) continue;
            const float hv = rowB[q * G_ROW + lane];
#pragma unroll
            for (int k = 0; k <= P3D_C; ++k) acc[33 + k] += rowA[q * G_ROW33 + k] * hv;
            if (lane <= P3D_C) acc[66] += rowA[q * G_ROW33 + lane];
        }
        __syncthreads();
        // dh = w1^T dO, dpre = dh * softplus'(pre)
        float dpre[P3D_HID];
#pragma unroll
        for (int n = 0; n < P3D_HID; ++n) {
            float a = 0.0f;
#pragma unroll
            for (int k = 0; k <= P3D_C; ++k) a += c.w1[k * P3D_HID + n] * dO[k];
            dpre[n] = s.live ? a * p3d_g_softplus_grad(pre[n]) : 0.0f;
        }
        // phase 2: d w0 [64][32] += dpre (x) X, d b0 += dpre   (slots 0..31: row 2k + lane/32, column lane%32; slot 32: b0[lane])
#pragma unroll
        for (int k = 0; k < P3D_C; ++k) rowA[lane * G_ROW33 + k] = X[k];
#pragma unroll
        for (int n = 0; n < P3D_HID; ++n) rowB[lane * G_ROW + n] = dpre[n];
        __syncthreads();
        for (int q = 0; q < G_WG; ++q) {
            if (!live_s[q]) continue;
            const float xv = rowA[q * G_ROW33 + (lane & 31)];
#pragma unroll
            for (int k = 0; k < 32; ++k) acc[k] += rowB[q * G_ROW + 2 * k + (lane >> 5)] * xv;
            acc[32] += rowB[q * G_ROW + lane];
        }
        __syncthreads();
        // dX = w0^T dpre; each plane receives dX / 3 (the mean), spread over its four taps
        float dX[P3D_C];
#pragma unroll
        for (int k = 0; k < P3D_C; ++k) {
            float a = 0.0f;
#pragma unroll
            for (int n = 0; n < P3D_HID; ++n) a += c.w0[n * P3D_C + k] * dpre[n];
            dX[k] = a * P3D_THIRD;
        }
        uint32_t* toff = reinterpret_cast<uint32_t*>(rowB);  // [64][12]
        float* twt = rowB + 64 * 12;                          // [64][12]
        int* timg = reinterpret_cast<int*>(rowB + 64 * 24);   // [64]
#pragma unroll
        for (int k = 0; k < P3D_C; ++k) rowA[lane * G_ROW33 + k] = dX[k];
#pragma unroll
        for (int k = 0; k < 12; ++k) {
            toff[lane * 12 + k] = tp.off[k];
            twt[lane * 12 + k] = tp.wt[k];
        }
        timg[lane] = s.live ? s.img : 0;
        __syncthreads();
        // scatter: one wave instruction = two taps x 32 channels = two 128-byte texel lines
        const int half = lane >> 5, ch32 = lane & 31;
        for (int q = 0; q < G_WG; ++q) {
            if (!live_s[q] || !c.dplanes) continue;
            float* dimg = c.dplanes + (int64_t)timg[q] * c.img_floats;
            const float dv = rowA[q * G_ROW33 + ch32];
#pragma unroll
            for (int pr = 0; pr < 6; ++pr) {
                const int tap = 2 * pr + half;
                const uint32_t off = toff[q * 12 + tap];
                const float v = twt[q * 12 + tap] * dv;
                if (off != P3D_G_NOTAP && v != 0.0f) unsafeAtomicAdd(dimg + off + ch32, v);
            }
        }
        __syncthreads();
    }
    float* slab = c.slab + (int64_t)blockIdx.x * G_SLAB;
#pragma unroll
    for (int k = 0; k < G_SLOTS; ++k) slab[k * G_WG + lane] = acc[k];
    if (lane == 0 && executed) atomicAdd(c.executed, executed);
}

// slot k of lane t <-> parameter index: slots 0..31 -> w0[2k + t/32][t%32]; 32 -> b0[t]; 33..65 -> w1[k-33][t]; 66 -> b1[t] (t < 33)
__device__ __forceinline__ int g_param_of(int k, int t) {
    if (k < 32) return (2 * k + (t >> 5)) * P3D_C + (t & 31);
    if (k == 32) return 2048 + t;
    if (k < 66) return 2112 + (k - 33) * P3D_HID + t;
    return t < 33 ? 4224 + t : -1;
}

// The slabs, summed in a fixed order: 16 strided partial sums per parameter, then the 16 partials in order.
__global__ __launch_bounds__(1024) void k_g_reduce(const float* __restrict__ slab, int nblocks, float* dw0, float* db0, float* dw1,
                                                   float* db1) {
    __shared__ float part[16][64];
    const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
    const int k = blockIdx.x;  // slot
    float a = 0.0f;
    for (int b = grp; b < nblocks; b += 16) a += slab[(int64_t)b * G_SLAB + k * G_WG + lane];
    part[grp][lane] = a;
    __syncthreads();
    if (grp == 0) {
        float s = part[0][lane];
        for (int q = 1; q < 16; ++q) s += part[q][lane];
        const int p = g_param_of(k, lane);
        if (p >= 0) {
            if (p < 2048) dw0[p] = s;
            else if (p < 2112) db0[p - 2048] = s;
            else if (p < 4224) dw1[p - 2112] = s;
            else db1[p - 4224] = s;
        }
    }
}

// ---- render backward: depth ranges, decode, ray recursion ---------------------------------------------------------------------
__global__ void k_g_range_init(uint32_t* mm, int n_pairs, unsigned long long* executed) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_pairs) {
        mm[2 * i] = 0xffffffffu;
        mm[2 * i + 1] = 0u;
    }
    if (i == 0) *executed = 0ull;
}

// Depths are sorted per ray: the ray's range is its first and last sample.  Wave-reduced, then one atomic per wave (and per view
// where a wave spans views only lane by lane).
__global__ void k_g_range(const float* __restrict__ depths, int64_t NR, int64_t R, int S, bool per_view, uint32_t* mm) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t lo = 0xffffffffu, hi = 0u;
    if (r < NR) {
        lo = p3d_f2ord(depths[r * S]);
        hi = p3d_f2ord(depths[r * S + S - 1]);
    }
    uint32_t wlo = lo, whi = hi;
    for (int m = 32; m >= 1; m >>= 1) {
        wlo = min(wlo, (uint32_t)__shfl_xor((int)wlo, m));
        whi = max(whi, (uint32_t)__shfl_xor((int)whi, m));
    }
    if ((threadIdx.x & 63) == 0) {
        atomicMin(mm, wlo);
        atomicMax(mm + 1, whi);
    }
    if (per_view && r < NR) {
        const int64_t v = r / R;
        atomicMin(mm + 2 + 2 * v, lo);
        atomicMax(mm + 3 + 2 * v, hi);
    }
}

struct GRayArgs {
    const float *planes, *rays_o, *rays_d, *depths, *w0, *b0, *w1, *b1, *g_feat, *g_depth, *g_wsum, *g_xyz;
    int H, W;
    int64_t NR, R, img_floats;
    int S;
    p3d_opts o;
    const uint32_t* mm;
    float *SG, *GS, *A, *TT;  // [S][NR]: sigma, s_i -> g_j, alpha_j -> colour coefficient, T_j -> density gradient
    uint8_t* FL;              // [S][NR]: 1 = a mask overwrote the density
};

__global__ __launch_bounds__(256) void k_g_decode(GRayArgs p) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= p.NR * p.S) return;
    const int64_t i = g / p.NR, r = g - i * p.NR;
    const float t = p.depths[r * p.S + i];
    const float px = p.rays_o[3 * r] + t * p.rays_d[3 * r];
    const float py = p.rays_o[3 * r + 1] + t * p.rays_d[3 * r + 1];
    const float pz = p.rays_o[3 * r + 2] + t * p.rays_d[3 * r + 2];
    const int img = (p.o.flags & P3D_FLAG_SHARED_PLANES) ? 0 : (int)(r / p.R);
    P3dGradTaps tp;
    float X[P3D_C], pre[P3D_HID], h[P3D_HID];
    p3d_g_taps(p.H, p.W, p.o.coord_scale, p.o.plane_mode, px, py, pz, tp);
    p3d_g_features(p.planes + (int64_t)img * p.img_floats, tp, X);
    p3d_g_hidden(p.w0, p.b0, X, pre, h);
    bool masked;
    const float sigma = p3d_g_masks(p3d_g_out_row(p.w1, p.b1, 0, h), px, pz, p.o, &masked);
    float s = 0.0f;
    if (p.g_feat) {
        const bool fsig = (p.o.flags & P3D_FLAG_FORCE_SIGMOID) != 0;
        for (int k = 1; k <= P3D_C; ++k) {
            const float gk = p.g_feat[r * P3D_C + k - 1];
            if (gk != 0.0f) s += gk * p3d_g_rgb(p3d_g_out_row(p.w1, p.b1, k, h), fsig);
        }
    }
    if (p.g_xyz) s += (p.g_xyz[3 * r] * px + p.g_xyz[3 * r + 1] * py) + p.g_xyz[3 * r + 2] * pz;
    p.SG[g] = sigma;
    p.GS[g] = s;
    p.FL[g] = masked ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_g_ray(GRayArgs p) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= p.NR) return;
    const int S = p.S;
    const int64_t NR = p.NR;
    const float* t = p.depths + r * S;
    float gsum = 0.0f;
    bool anyc = false;
    if (p.g_feat)
        for (int k = 0; k < P3D_C; ++k) {
            const float v = p.g_feat[r * P3D_C + k];
            gsum += v;
            anyc = anyc || (v != 0.0f);
        }
    if (p.g_xyz) gsum += (p.g_xyz[3 * r] + p.g_xyz[3 * r + 1]) + p.g_xyz[3 * r + 2];
    const float gW = p.g_wsum ? p.g_wsum[r] : 0.0f;
    const float gD = p.g_depth ? p.g_depth[r] : 0.0f;
    const float wb = (p.o.flags & P3D_FLAG_WHITE_BACK) ? 1.0f : 0.0f;
    const float gconst = gW - 2.0f * wb * gsum;  // d/dw_j of  2 (sum w cmid + b (1 - W)) - 1  and of  W, the part common to all j
    // forward sweep: the forward's weights (ray_marcher.py:25-46, numerics as p3d_numerics.h "compositing")
    MarchState st = p3d_march_start(t[0], p.SG[r]);
    float s0 = p.GS[r];
    for (int j = 0; j < S - 1; ++j) {
        const int64_t g1 = (int64_t)(j + 1) * NR + r;
        const float t1 = t[j + 1], sg1 = p.SG[g1], s1 = p.GS[g1];
        const P3dInterval iv = p3d_march_interval(st, t1, sg1);
        p3d_march_accumulate(st, iv);
        const int64_t g0 = (int64_t)j * NR + r;
        p.A[g0] = iv.alpha;
        p.TT[g0] = iv.T;
        p.GS[g0] = (s0 + s1) + gconst;  // 2 <g_feat, cmid_j> + 2 <g_xyz, pmid_j> + g_W - 2 b (sum g_feat + sum g_xyz)
        st.prev_t = t1;
        st.prev_sigma = sg1;
        s0 = s1;
    }
    const float Wsum = st.W, Dsum = st.D;
    // depth = clamp(nan_to_num(D / W, inf), tmin, tmax): its gradient passes only where D / W is finite and inside the range
    const uint32_t* mm = (p.o.flags & P3D_FLAG_PER_VIEW_CLAMP) ? p.mm + 2 + 2 * (r / p.R) : p.mm;
    const float tmin = p3d_ord2f(mm[0]), tmax = p3d_ord2f(mm[1]);
    const float dep = Dsum / Wsum;
    const float kappa = (gD != 0.0f && __builtin_isfinite(dep) && dep >= tmin && dep <= tmax) ? gD : 0.0f;
    // back to front: dL/dalpha_j = T_j (g_j - R_{j+1}),  R_j = alpha_j g_j + (1 - alpha_j + 1e-10) R_{j+1}
    float Racc = 0.0f, dsm_next = 0.0f, w_next = 0.0f;
    float t1 = t[S - 1], sg1 = p.SG[(int64_t)(S - 1) * NR + r];
    for (int j = S - 2; j >= 0; --j) {
        const int64_t g0 = (int64_t)j * NR + r, g1 = g0 + NR;
        const float tj = t[j], sgj = p.SG[g0];
        const float a = p.A[g0], T = p.TT[g0];
        float gj = p.GS[g0];
        const float dl = t1 - tj, sm = (sgj + sg1) * 0.5f;
        if (kappa != 0.0f) gj += kappa * (((tj + t1) * 0.5f - dep) / Wsum);
        const float dalpha = T * (gj - Racc);
        Racc = a * gj + ((1.0f - a) + 1e-10f) * Racc;
        // alpha = 1 - exp(-softplus(sm - 1) dl): d alpha / d sm = dl exp(-rho dl) softplus'(sm - 1)
        const float dsm = dalpha * dl * (1.0f - a) * p3d_g_softplus_grad(sm - 1.0f);
        const float w = a * T;
        p.TT[g1] = p.FL[g1] ? 0.0f : 0.5f * (dsm + dsm_next);  // sample j+1 is complete: both of its intervals are done
        p.A[g1] = anyc ? (w + w_next) : 0.0f;
        dsm_next = dsm;
        w_next = w;
        t1 = tj;
        sg1 = sgj;
    }
    p.TT[r] = p.FL[r] ? 0.0f : 0.5f * dsm_next;
    p.A[r] = anyc ? w_next : 0.0f;
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
struct GLayout {
    size_t mm, sg, gs, a, tt, fl, slab, total;
    int64_t blocks;
};

static GLayout g_render_layout(int N, int64_t R, int S) {
    GLayout L;
    const int64_t NS = (int64_t)N * R * S;
    size_t o = P3D_GRAD_STATS_BYTES;
    L.mm = o;
    o += g_align(sizeof(uint32_t) * 2 * ((size_t)N + 1));
    L.sg = o;
    o += g_align(sizeof(float) * NS);
    L.gs = o;
    o += g_align(sizeof(float) * NS);
    L.a = o;
    o += g_align(sizeof(float) * NS);
    L.tt = o;
    o += g_align(sizeof(float) * NS);
    L.fl = o;
    o += g_align((size_t)NS);
    L.blocks = g_blocks(NS);
    L.slab = o;
    o += g_align(sizeof(float) * G_SLAB * (size_t)L.blocks);
    L.total = o;
    return L;
}

static bool g_sizes_ok(int N, int H, int W) {
    return N > 0 && H > 0 && W > 0 && H <= 4096 && W <= 4096;  // per-image float offsets are 32-bit: 3 * 4096^2 * 32 < 2^32
}

extern "C" size_t p3d_render_backward_workspace_bytes(int N, int64_t R, int Sc, int Sf) {
    if (N <= 0 || R <= 0 || Sc < 2 || Sf < 0) return 0;
    return g_render_layout(N, R, Sc + Sf).total;
}

extern "C" size_t p3d_triplane_decode_backward_workspace_bytes(int N, int64_t M) {
    if (N <= 0 || M <= 0) return 0;
    return P3D_GRAD_STATS_BYTES + g_align(sizeof(float) * G_SLAB * (size_t)g_blocks((int64_t)N * M));
}

static int g_launch_mlp_reduce(const GCommon& c, int64_t blocks, float* d_w0, float* d_b0, float* d_w1, float* d_b1,
                               hipStream_t st, const GRenderSrc* rs, const GPointSrc* ps) {
    if (rs)
        hipLaunchKernelGGL(k_g_mlp<GRenderSrc>, dim3((unsigned)blocks), dim3(G_WG), 0, st, c, *rs);
    else
        hipLaunchKernelGGL(k_g_mlp<GPointSrc>, dim3((unsigned)blocks), dim3(G_WG), 0, st, c, *ps);
    hipLaunchKernelGGL(k_g_reduce, dim3(G_SLOTS), dim3(1024), 0, st, (const float*)c.slab, (int)blocks, d_w0, d_b0, d_w1, d_b1);
    return (int)hipGetLastError();
}

extern "C" int p3d_render_backward_f32(const float* planes_nhwc, int N, int H, int W, const float* rays_o, const float* rays_d,
                                       int64_t R, const float* depths_sorted, const float* w0, const float* b0, const float* w1,
                                       const float* b1, const p3d_opts* opts, const float* g_feat, const float* g_depth,
                                       const float* g_wsum, const float* g_xyz, float* d_planes_nhwc, float* d_w0, float* d_b0,
                                       float* d_w1, float* d_b1, void* workspace, size_t workspace_bytes, void* stream) {
    if (!planes_nhwc || !rays_o || !rays_d || !depths_sorted || !w0 || !b0 || !w1 || !b1 || !opts || !d_w0 || !d_b0 || !d_w1 ||
        !d_b1 || !workspace)
        return P3D_E_ARG;
    if (N <= 0 || R <= 0 || H <= 0 || W <= 0) return P3D_E_ARG;
    const int Sc = opts->Sc, Sf = opts->Sf;
    if (!g_sizes_ok(N, H, W) || Sc < 2 || Sc > P3D_MAX_S || Sf < 0 || Sf > P3D_MAX_S) return P3D_E_RANGE;
    if (((uintptr_t)workspace & 255) != 0) return P3D_E_ARG;
    const int S = Sc + Sf;
    const GLayout L = g_render_layout(N, R, S);
    if (workspace_bytes < L.total) return P3D_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    const int64_t NR = (int64_t)N * R, NS = NR * S;
    const int64_t img_floats = (int64_t)3 * H * W * P3D_C;
    GRayArgs p;
    p.planes = planes_nhwc;
    p.rays_o = rays_o;
    p.rays_d = rays_d;
    p.depths = depths_sorted;
    p.w0 = w0;
    p.b0 = b0;
    p.w1 = w1;
    p.b1 = b1;
    p.g_feat = g_feat;
    p.g_depth = g_depth;
    p.g_wsum = g_wsum;
    p.g_xyz = g_xyz;
    p.H = H;
    p.W = W;
    p.NR = NR;
    p.R = R;
    p.img_floats = img_floats;
    p.S = S;
    p.o = *opts;
    p.mm = (const uint32_t*)(ws + L.mm);
    p.SG = (float*)(ws + L.sg);
    p.GS = (float*)(ws + L.gs);
    p.A = (float*)(ws + L.a);
    p.TT = (float*)(ws + L.tt);
    p.FL = (uint8_t*)(ws + L.fl);
    unsigned long long* executed = (unsigned long long*)ws;
    const int pairs = N + 1;
    hipLaunchKernelGGL(k_g_range_init, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, st, (uint32_t*)(ws + L.mm), pairs, executed);
    hipLaunchKernelGGL(k_g_range, dim3((unsigned)((NR + 255) / 256)), dim3(256), 0, st, depths_sorted, NR, R, S,
                       (opts->flags & P3D_FLAG_PER_VIEW_CLAMP) != 0, (uint32_t*)(ws + L.mm));
    hipLaunchKernelGGL(k_g_decode, dim3((unsigned)((NS + 255) / 256)), dim3(256), 0, st, p);
    hipLaunchKernelGGL(k_g_ray, dim3((unsigned)((NR + 255) / 256)), dim3(256), 0, st, p);
    GCommon c;
    c.planes = planes_nhwc;
    c.dplanes = d_planes_nhwc;
    c.H = H;
    c.W = W;
    c.img_floats = img_floats;
    c.w0 = w0;
    c.b0 = b0;
    c.w1 = w1;
    c.b1 = b1;
    c.o = *opts;
    c.slab = (float*)(ws + L.slab);
    c.executed = executed;
    c.total = NS;
    GRenderSrc rs;
    rs.depths = depths_sorted;
    rs.rays_o = rays_o;
    rs.rays_d = rays_d;
    rs.g_feat = g_feat;
    rs.dsig = p.TT;
    rs.coef = p.A;
    rs.NR = NR;
    rs.R = R;
    rs.S = S;
    rs.shared = (opts->flags & P3D_FLAG_SHARED_PLANES) != 0;
    return g_launch_mlp_reduce(c, L.blocks, d_w0, d_b0, d_w1, d_b1, st, &rs, nullptr);
}

extern "C" int p3d_triplane_decode_backward_f32(const float* planes_nhwc, int N, int H, int W, const float* coords, int64_t M,
                                                const float* w0, const float* b0, const float* w1, const float* b1,
                                                const p3d_opts* opts, const float* g_sigma, const float* g_rgb, float* d_planes_nhwc,
                                                float* d_w0, float* d_b0, float* d_w1, float* d_b1, void* workspace,
                                                size_t workspace_bytes, void* stream) {
    if (!planes_nhwc || !coords || !w0 || !b0 || !w1 || !b1 || !opts || !d_w0 || !d_b0 || !d_w1 || !d_b1 || !workspace)
        return P3D_E_ARG;
    if (N <= 0 || M <= 0 || H <= 0 || W <= 0) return P3D_E_ARG;
    if (!g_sizes_ok(N, H, W)) return P3D_E_RANGE;
    if (((uintptr_t)workspace & 255) != 0) return P3D_E_ARG;
    const int64_t blocks = g_blocks((int64_t)N * M);
    if (workspace_bytes < p3d_triplane_decode_backward_workspace_bytes(N, M)) return P3D_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    unsigned long long* executed = (unsigned long long*)ws;
    hipLaunchKernelGGL(k_g_range_init, dim3(1), dim3(64), 0, st, (uint32_t*)nullptr, 0, executed);
    GCommon c;
    c.planes = planes_nhwc;
    c.dplanes = d_planes_nhwc;
    c.H = H;
    c.W = W;
    c.img_floats = (int64_t)3 * H * W * P3D_C;
    c.w0 = w0;
    c.b0 = b0;
    c.w1 = w1;
    c.b1 = b1;
    c.o = *opts;
    c.slab = (float*)(ws + P3D_GRAD_STATS_BYTES);
    c.executed = executed;
    c.total = (int64_t)N * M;
    GPointSrc ps;
    ps.coords = coords;
    ps.g_sigma = g_sigma;
    ps.g_rgb = g_rgb;
    ps.M = M;
    ps.shared = (opts->flags & P3D_FLAG_SHARED_PLANES) != 0;
    return g_launch_mlp_reduce(c, blocks, d_w0, d_b0, d_w1, d_b1, st, nullptr, &ps);
}
