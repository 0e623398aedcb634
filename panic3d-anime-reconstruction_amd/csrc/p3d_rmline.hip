// p3d_rmline.hip — the illustration-to-render module's kernels (include/p3d_rmline.h).
//
//   k_rm_mask          the line mask in one launch: per 8 x 32 tile the composited grey values of the tile and its halo go to LDS, both
//                      Gaussians run over them horizontally, then vertically, the response is thresholded into LDS and the d x d window
//                      over those bits, less the hull, is the mask.  Nothing in between reaches memory;
//   k_rm_conv<MB, R>   one unpadded 3 x 3 convolution as an implicit GEMM on v_mfma_f32_16x16x4_f32: a workgroup takes 4R rows x 32
//                      columns of output pixels and 16 MB output channels; its input patch ((4R + 2) x 34 pixels, channel-last) and its
//                      weights (all nine taps) are staged in LDS once, then each wave walks K = (tap, ci) for its R rows.  The first
//                      layer's load builds `stackin` from image, mask and hull with the replicate padding as a coordinate clamp; the
//                      last layer's store applies tanh and the lerp against image and mask;
//   p3d_rmline_forward_f32   the mask kernel and every layer from a host table: one C call.
// Every sum runs in a fixed order and nothing is accumulated with atomics.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/p3d_rmline.h"
#include "p3d_rmline_plan.hpp"
#include "p3d_rmline_tile.hpp"

// ---- the line mask ------------------------------------------------------------------------------------------------------------------
#define RM_MT_W 32
#define RM_MT_H 8
#define RM_MAX_R (P3D_RMLINE_MAX_TAPS / 2)    // the widest blur's radius
#define RM_MAX_E (P3D_RMLINE_MAX_DILATE - 1)  // the rows / columns of response a dilated tile needs beyond its own
#define RM_G_ROWS (RM_MT_H + RM_MAX_E + 2 * RM_MAX_R)
#define RM_G_COLS (RM_MT_W + RM_MAX_E + 2 * RM_MAX_R)
#define RM_R_ROWS (RM_MT_H + RM_MAX_E)
#define RM_R_COLS (RM_MT_W + RM_MAX_E)

struct RmMask {
    const float* img;
    const float* hull;
    float* mask;
    float* image;
    float* response;
    int C, H, W, tiles_x;
    int k0, k1, d;
    float t, eps;
    float w0[P3D_RMLINE_MAX_TAPS], w1[P3D_RMLINE_MAX_TAPS];
};

// the composited colour j of pixel p (a pointer to its first channel), plane = H W
__device__ __forceinline__ float rm_colour(const float* p, int64_t plane, int C, int j) {
    const float v = p[j * plane];
    if (C != 4) return v;
    const float a = p[3 * plane];
    return v * a + (1.f - a);
}

__device__ __forceinline__ float rm_grey(const float* p, int64_t plane, int C) {
    if (C == 1) return p[0];
    return (0.299f * rm_colour(p, plane, C, 0) + 0.587f * rm_colour(p, plane, C, 1)) + 0.114f * rm_colour(p, plane, C, 2);
}

__global__ __launch_bounds__(RM_WG) void k_rm_mask(RmMask m) {
    __shared__ float G[RM_G_ROWS * RM_G_COLS];       // grey, tile + halo
    __shared__ float H0[RM_G_ROWS * RM_R_COLS];      // horizontally blurred with w0 / w1
    __shared__ float H1[RM_G_ROWS * RM_R_COLS];
    __shared__ unsigned char B[RM_R_ROWS * RM_R_COLS];  // response > 0.5, inside the image
    const int tid = threadIdx.x, n = blockIdx.y;
    const int x0 = (blockIdx.x % m.tiles_x) * RM_MT_W, y0 = (blockIdx.x / m.tiles_x) * RM_MT_H;
    const int r0 = m.k0 / 2, r1 = m.k1 / 2, e = m.d - 1, o = m.d / 2;
    const int gw = RM_MT_W + e + 2 * r1, gh = RM_MT_H + e + 2 * r1;  // the grey region: starts at (y0 - o - r1, x0 - o - r1)
    const int rw = RM_MT_W + e, rh = RM_MT_H + e;                    // the response region: starts at (y0 - o, x0 - o)
    const int64_t plane = (int64_t)m.H * m.W;
    const float* img = m.img + (int64_t)n * m.C * plane;
    for (int i = tid; i < gh * gw; i += RM_WG) {
        const int gy = i / gw, gx = i % gw;
        const int y = rm_clamp(y0 - o - r1 + gy, m.H - 1), x = rm_clamp(x0 - o - r1 + gx, m.W - 1);
        G[gy * gw + gx] = rm_grey(img + (int64_t)y * m.W + x, plane, m.C);
    }
    __syncthreads();
    for (int i = tid; i < gh * rw; i += RM_WG) {
        const int gy = i / rw, rx = i % rw;
        const float* row = G + gy * gw + rx;  // column rx of the response region is column rx + r1 of the grey region
        float a0 = 0.f, a1 = 0.f;
        for (int j = 0; j < m.k0; ++j) a0 = __builtin_fmaf(m.w0[j], row[r1 - r0 + j], a0);
        for (int j = 0; j < m.k1; ++j) a1 = __builtin_fmaf(m.w1[j], row[j], a1);
        H0[gy * rw + rx] = a0;
        H1[gy * rw + rx] = a1;
    }
    __syncthreads();
    for (int i = tid; i < rh * rw; i += RM_WG) {
        const int ry = i / rw, rx = i % rw;
        float g0 = 0.f, g1 = 0.f;
        for (int j = 0; j < m.k0; ++j) g0 = __builtin_fmaf(m.w0[j], H0[(ry + r1 - r0 + j) * rw + rx], g0);
        for (int j = 0; j < m.k1; ++j) g1 = __builtin_fmaf(m.w1[j], H1[(ry + j) * rw + rx], g1);
        float resp = (0.5f + m.t * (g1 - g0)) - m.eps;
        resp = __builtin_fminf(__builtin_fmaxf(resp, 0.f), 1.f);
        const int y = y0 - o + ry, x = x0 - o + rx;
        const bool in = y >= 0 && y < m.H && x >= 0 && x < m.W;
        B[ry * rw + rx] = in && resp > 0.5f;
        const int ty = ry - o, tx = rx - o;  // this tile's own pixels carry the response out
        if (m.response && in && ty >= 0 && ty < RM_MT_H && tx >= 0 && tx < RM_MT_W) m.response[(int64_t)n * plane + (int64_t)y * m.W + x] = resp;
    }
    __syncthreads();
    const int ty = tid / RM_MT_W, tx = tid % RM_MT_W, y = y0 + ty, x = x0 + tx;
    if (y >= m.H || x >= m.W) return;
    bool any = false;
    for (int j = 0; j < m.d; ++j)
        for (int i = 0; i < m.d; ++i) any = any || B[(ty + j) * rw + tx + i];
    const int64_t at = (int64_t)y * m.W + x;
    if (m.hull && m.hull[(int64_t)n * plane + at] != 0.f) any = false;
    m.mask[(int64_t)n * plane + at] = any ? 1.f : 0.f;
    if (m.image)
        for (int j = 0; j < 3; ++j) m.image[((int64_t)n * 3 + j) * plane + at] = rm_colour(img + at, plane, m.C, j);
}

// taps and weights of one Gaussian, as the header states them
static void rm_gauss(int taps, double s, float* w) {
    double e[P3D_RMLINE_MAX_TAPS], sum = 0.0;
    for (int i = 0; i < taps; ++i) {
        const double x = (double)(i - taps / 2);
        e[i] = exp(-(x * x) / (2.0 * s * s));
        sum += e[i];
    }
    for (int i = 0; i < taps; ++i) w[i] = (float)(e[i] / sum);
}

static int rm_dog_taps(const p3d_rmline_dog* dog, int* k0, int* k1) {
    if (!dog) return P3D_E_ARG;
    const double s = dog->sigma, k = dog->k, kf = dog->kernel_factor;
    if (!(s > 0.0) || !(k > 0.0) || !(kf > 0.0) || !isfinite(s) || !isfinite(k) || !isfinite(kf) || !isfinite(dog->t) || !isfinite(dog->epsilon))
        return P3D_E_ARG;
    if (dog->d < 1 || dog->d > P3D_RMLINE_MAX_DILATE || dog->reserved != 0) return P3D_E_RANGE;
    const double a = s * kf, b = s * k * kf;  // (Python's order: sigma*kernel_factor, sigma*k*kernel_factor)
    if (a >= P3D_RMLINE_MAX_TAPS || b >= P3D_RMLINE_MAX_TAPS) return P3D_E_RANGE;
    *k0 = 2 * (int)a + 1 < 3 ? 3 : 2 * (int)a + 1;
    *k1 = 2 * (int)b + 1 < 3 ? 3 : 2 * (int)b + 1;
    if (*k0 > P3D_RMLINE_MAX_TAPS || *k1 > P3D_RMLINE_MAX_TAPS || *k1 < *k0) return P3D_E_RANGE;  // (the halo is the second blur's)
    return 0;
}

extern "C" int p3d_rmline_dog_taps(const p3d_rmline_dog* dog, int* out2) {
    if (!out2) return P3D_E_ARG;
    return rm_dog_taps(dog, &out2[0], &out2[1]);
}

static int rm_mask_check(int N, int C, int H, int W, const p3d_rmline_dog* dog, RmMask* m, dim3* grid) {
    if (N <= 0 || H <= 0 || W <= 0) return P3D_E_ARG;
    int rc = rm_dog_taps(dog, &m->k0, &m->k1);
    if (rc) return rc;
    if ((C != 1 && C != 3 && C != 4) || H > 32768 || W > 32768 || N > 65535) return P3D_E_RANGE;
    m->C = C, m->H = H, m->W = W, m->d = dog->d, m->t = (float)dog->t, m->eps = (float)dog->epsilon;
    m->tiles_x = (W + RM_MT_W - 1) / RM_MT_W;
    rm_gauss(m->k0, dog->sigma, m->w0);
    rm_gauss(m->k1, dog->sigma * dog->k, m->w1);
    *grid = dim3((unsigned)(m->tiles_x * ((H + RM_MT_H - 1) / RM_MT_H)), (unsigned)N);
    return 0;
}

extern "C" int p3d_rmline_mask_f32(const float* img, int N, int C, int H, int W, const float* hull, const p3d_rmline_dog* dog, float* mask,
                                   float* image, float* response, void* stream) {
    if (!img || !mask || !dog || (image && C < 3)) return P3D_E_ARG;
    RmMask m;
    dim3 grid;
    const int rc = rm_mask_check(N, C, H, W, dog, &m, &grid);
    if (rc) return rc;
    m.img = img, m.hull = hull, m.mask = mask, m.image = image, m.response = response;
    hipLaunchKernelGGL(k_rm_mask, grid, dim3(RM_WG), 0, (hipStream_t)stream, m);
    return (int)hipGetLastError();
}

// ---- one layer ------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float rm_act(float v, int act, float slope) {
    if (act == P3D_RMLINE_ACT_LEAKY) return v > 0.f ? v : v * slope;
    if (act == P3D_RMLINE_ACT_TANH) return tanhf(v);
    return v;
}

// The patch loads and the tile loop (rm_tile_mma, on __builtin_amdgcn_mfma_f32_16x16x4f32) are p3d_rmline_tile.hpp's, shared with the
// backward kernels of p3d_rmline_grad.hip.
template <int MB, int R, bool PT>
__global__ __launch_bounds__(RM_WG) void k_rm_conv(RmConv c) {
    constexpr int COT = 16 * MB, PH = 4 * R + 2, NB = 2 * R;
    extern __shared__ __attribute__((aligned(16))) float rm_lds[];
    float* Xs = rm_lds;                     // [PH][RM_PW][cip]: the input patch, channel-last
    float* Ws = rm_lds + PH * RM_PW * c.cip;  // [9][COT][cip]: the weights, a filter's channels contiguous
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = blockIdx.z, co0 = blockIdx.y * COT;
    const int x0 = (blockIdx.x % c.tiles_x) * RM_TW, y0 = (blockIdx.x / c.tiles_x) * (4 * R);
    // the weights: wk [9][Ci][Co] -> Ws[tap][co][ci], zeros beyond Ci and Co
    // Both staging loops issue RM_BATCH loads — every one unconditional, from a clamped index (element 0 where the operand is out of
    // range) — before they store any of them, so that a batch's loads are in flight together; the predicates are applied at the store.
    {
        constexpr int WSTEP = RM_WG / COT;
        const int col = tid % COT;  // a lane keeps its output channel: consecutive lanes read consecutive floats of a wk row
        const bool co_in = co0 + col < c.Co;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap)
            for (int cb = tid / COT; cb < c.ci4; cb += RM_BATCH * WSTEP) {
                float r[RM_BATCH];
#pragma unroll
                for (int j = 0; j < RM_BATCH; ++j) {
                    const int ci = cb + j * WSTEP;
                    r[j] = c.wk[co_in && ci < c.Ci ? ((int64_t)tap * c.Ci + ci) * c.Co + co0 + col : 0];
                }
#pragma unroll
                for (int j = 0; j < RM_BATCH; ++j) {
                    const int ci = cb + j * WSTEP;
                    if (ci < c.ci4) Ws[(tap * COT + col) * c.cip + ci] = co_in && ci < c.Ci ? r[j] : 0.f;
                }
            }
    }
    // the patch: pixels outside the input (a ragged tile) are zeros; they only feed outputs that are not stored
    if (c.flags & P3D_RMLINE_IN_STACK) rm_stage_stack(c, n, y0, x0, PH, Xs, c.cip, 4);
    else rm_stage_cl(c, n, y0, x0, 0, PH, Xs, c.cip, c.ci4);
    __syncthreads();
    rm_f32x4 acc[MB][NB];
#pragma unroll
    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[mb][nb] = rm_f32x4{0.f, 0.f, 0.f, 0.f};
    rm_tile_mma<MB, R, PT>(Xs, Ws, c.cip, c.ci4, wave, lane, acc);  // PT: P3D_RMLINE_SUM_PER_TAP
    const int l15 = lane & 15, kq = lane >> 4;
    const bool planar = (c.flags & P3D_RMLINE_OUT_PLANAR) != 0, lerp = (c.flags & P3D_RMLINE_OUT_LERP) != 0;
    const int64_t oplane = (int64_t)c.Ho * c.Wo;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        const int oy = y0 + wave * R + nb / 2, ox = x0 + 16 * (nb % 2) + l15;
        if (oy >= c.Ho || ox >= c.Wo) continue;
        const int64_t pix = (int64_t)oy * c.Wo + ox;
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) {
            const int cb = co0 + 16 * mb + 4 * kq;
            if (cb >= c.Co) continue;
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = cb + r < c.Co ? rm_act(acc[mb][nb][r] + c.bias[cb + r], c.act, c.slope) : 0.f;
            if (!planar) {
                float* dst = c.out + ((int64_t)n * oplane + pix) * c.Co + cb;
                if ((c.Co & 3) == 0) *(rm_f32x4*)dst = rm_f32x4{v[0], v[1], v[2], v[3]};
                else
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (cb + r < c.Co) dst[r] = v[r];
                continue;
            }
            const float w = lerp ? c.mask[(int64_t)n * oplane + pix] : 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (cb + r >= c.Co) continue;
                const int64_t at = ((int64_t)n * c.Co + cb + r) * oplane + pix;
                float res = v[r];
                if (lerp) {
                    const float a = c.image[at], diff = v[r] - a;
                    res = w < 0.5f ? a + w * diff : v[r] - diff * (1.f - w);
                }
                c.out[at] = res;
            }
        }
    }
}

extern "C" int p3d_rmline_conv_plan(int Ci, int Co, int force_plan, int* out3) {
    RmPlan p;
    const int rc = rm_conv_plan(Ci, Co, force_plan, &p);
    if (rc) return rc;
    if (out3) out3[0] = p.rows, out3[1] = p.cot, out3[2] = (int)p.lds;
    return p.plan;
}

// the checks of one layer; fills the kernel's sizes and the plan
static int rm_conv_check(int N, int Hin, int Win, int pad, int Ci, int Co, int act, float slope, int flags, int force_plan, bool has_x,
                         bool has_image, bool has_mask, bool has_hull, RmConv* c, RmPlan* p) {
    if (N <= 0 || Hin <= 0 || Win <= 0 || Ci <= 0 || Co <= 0) return P3D_E_ARG;
    const bool stack = (flags & P3D_RMLINE_IN_STACK) != 0, lerp = (flags & P3D_RMLINE_OUT_LERP) != 0;
    if (stack ? !has_image : !has_x) return P3D_E_ARG;
    if (lerp && (!has_image || !has_mask)) return P3D_E_ARG;
    if (flags & ~(P3D_RMLINE_IN_STACK | P3D_RMLINE_OUT_PLANAR | P3D_RMLINE_OUT_LERP | P3D_RMLINE_IN_NO_MASK | P3D_RMLINE_SUM_PER_TAP)) return P3D_E_RANGE;
    if (act != P3D_RMLINE_ACT_NONE && act != P3D_RMLINE_ACT_LEAKY && act != P3D_RMLINE_ACT_TANH) return P3D_E_RANGE;
    if (!isfinite(slope) || pad < 0 || pad > 4096 || Hin < 3 || Win < 3 || N > 65535) return P3D_E_RANGE;
    const int rc = rm_conv_plan(Ci, Co, force_plan, p);
    if (rc) return rc;
    if (stack) {
        if (Hin - 2 * pad < 1 || Win - 2 * pad < 1 || Ci != 3 + (has_hull ? 1 : 0)) return P3D_E_RANGE;
    } else if (pad != 0) {
        return P3D_E_RANGE;
    }
    if (lerp && (!(flags & P3D_RMLINE_OUT_PLANAR) || Co != 3 || (stack && pad != 1))) return P3D_E_RANGE;
    const int cmax = p->ci4 > Co ? p->ci4 : Co;
    if ((int64_t)N * Hin * Win >= ((int64_t)1 << 31) / cmax) return P3D_E_RANGE;
    c->Hin = Hin, c->Win = Win, c->Ho = Hin - 2, c->Wo = Win - 2, c->pad = pad, c->Ci = Ci, c->Co = Co, c->act = act, c->flags = flags;
    c->Hi = Hin - 2 * pad, c->Wi = Win - 2 * pad, c->ci4 = p->ci4, c->cip = p->cip, c->slope = slope;
    c->tiles_x = (c->Wo + RM_TW - 1) / RM_TW;
    return 0;
}

static int rm_conv_launch(RmConv& c, const RmPlan& p, int N, hipStream_t s) {
    static const void* const kernels[8] = {(const void*)k_rm_conv<1, 1, false>, (const void*)k_rm_conv<1, 2, false>, (const void*)k_rm_conv<2, 1, false>,
                                           (const void*)k_rm_conv<2, 2, false>, (const void*)k_rm_conv<1, 1, true>,  (const void*)k_rm_conv<1, 2, true>,
                                           (const void*)k_rm_conv<2, 1, true>,  (const void*)k_rm_conv<2, 2, true>};
    static bool raised[8][RM_MAX_DEVICES];  // the dynamic-LDS limit is a property of (kernel, device): raised once for each
    const int which = (p.cot == 32 ? 2 : 0) + (p.rows == 8 ? 1 : 0) + ((c.flags & P3D_RMLINE_SUM_PER_TAP) ? 4 : 0);
    const int rc = rm_raise_lds(kernels[which], p.lds, raised[which]);
    if (rc) return rc;
    const dim3 grid((unsigned)(c.tiles_x * ((c.Ho + p.rows - 1) / p.rows)), (unsigned)p.cblocks, (unsigned)N);
    void* args[] = {&c};
    return (int)hipLaunchKernel(kernels[which], grid, dim3(RM_WG), args, p.lds, s);
}

extern "C" int p3d_rmline_conv_f32(const float* x, const float* image, const float* mask, const float* hull, int N, int Hin, int Win, int pad,
                                   int Ci, const float* wk, const float* bias, int Co, int act, float slope, int flags, int force_plan,
                                   float* out, void* stream) {
    if (!wk || !bias || !out) return P3D_E_ARG;
    if (rm_misaligned(x, Ci) || (!(flags & P3D_RMLINE_OUT_PLANAR) && rm_misaligned(out, Co))) return P3D_E_ARG;
    RmConv c;
    RmPlan p;
    const bool stack = (flags & P3D_RMLINE_IN_STACK) != 0;
    const int rc = rm_conv_check(N, Hin, Win, pad, Ci, Co, act, slope, flags, force_plan, x != nullptr, image != nullptr, mask != nullptr,
                                 stack && hull != nullptr, &c, &p);
    if (rc) return rc;
    c.x = x, c.image = image, c.mask = mask, c.hull = stack ? hull : nullptr, c.wk = wk, c.bias = bias, c.out = out;
    return rm_conv_launch(c, p, N, (hipStream_t)stream);
}

extern "C" int p3d_rmline_struct_layout(int which, size_t* out, int cap) {
    if (!out || cap <= 0) return P3D_E_ARG;
    int n = 0;
#define RM_PUT(v) do { if (n >= cap) return P3D_E_RANGE; out[n++] = (size_t)(v); } while (0)
    if (which == 0) {
#define RM_OFF(f) RM_PUT(offsetof(p3d_rmline_dog, f))
        RM_PUT(sizeof(p3d_rmline_dog));
        RM_OFF(t); RM_OFF(sigma); RM_OFF(k); RM_OFF(epsilon); RM_OFF(kernel_factor); RM_OFF(d); RM_OFF(reserved);
#undef RM_OFF
    } else if (which == 1) {
#define RM_OFF(f) RM_PUT(offsetof(p3d_rmline_layer, f))
        RM_PUT(sizeof(p3d_rmline_layer));
        RM_OFF(Ci); RM_OFF(Co); RM_OFF(act); RM_OFF(plan); RM_OFF(slope); RM_OFF(reserved); RM_OFF(w_off); RM_OFF(b_off);
#undef RM_OFF
    } else {
        return P3D_E_RANGE;
    }
#undef RM_PUT
    return n;
}

// ---- the whole module -----------------------------------------------------------------------------------------------------------------
#define RM_MAX_LAYERS 64

extern "C" int p3d_rmline_forward_f32(const float* img, int N, int C, int H, int W, const float* hull, const p3d_rmline_dog* dog,
                                      const p3d_rmline_layer* layers, int n_layers, const float* weights, int64_t weight_floats, int pad,
                                      int flags, float* image, float* mask, float* act0, float* act1, int64_t act_floats, float* out,
                                      int* launches, void* stream) {
    if (launches) *launches = 0;
    if (!img || !layers || !weights || !out) return P3D_E_ARG;
    if (N <= 0 || H <= 0 || W <= 0 || n_layers <= 0 || weight_floats <= 0) return P3D_E_ARG;
    if (flags & ~(P3D_RMLINE_FWD_MASK_INPUT | P3D_RMLINE_FWD_LERP)) return P3D_E_RANGE;
    if (n_layers > RM_MAX_LAYERS || pad < 0 || pad > 4096) return P3D_E_RANGE;
    const bool lerp = (flags & P3D_RMLINE_FWD_LERP) != 0, mask_in = (flags & P3D_RMLINE_FWD_MASK_INPUT) != 0;
    if ((dog || lerp || mask_in) && !mask) return P3D_E_ARG;
    if (dog ? (C != 3 && C != 4) : C != 3) return P3D_E_RANGE;
    if (dog && C == 4 && !image) return P3D_E_ARG;
    if (n_layers > 1 && (!act0 || !act1 || act0 == act1)) return P3D_E_ARG;
    if (n_layers > 1 && (((uintptr_t)act0 | (uintptr_t)act1) & 15)) return P3D_E_ARG;  // (read and written in 16-byte vectors)
    if (lerp && pad != n_layers) return P3D_E_RANGE;
    if (H + 2 * (int64_t)pad - 2 * n_layers < 1 || W + 2 * (int64_t)pad - 2 * n_layers < 1) return P3D_E_RANGE;
    RmMask m;
    dim3 mgrid;
    if (dog) {
        const int rc = rm_mask_check(N, C, H, W, dog, &m, &mgrid);
        if (rc) return rc;
        m.img = img, m.hull = hull, m.mask = mask, m.image = C == 4 ? image : nullptr, m.response = nullptr;
    }
    const float* img3 = dog && C == 4 ? image : img;
    RmConv cs[RM_MAX_LAYERS];
    RmPlan ps[RM_MAX_LAYERS];
    for (int i = 0; i < n_layers; ++i) {  // every record, before any launch
        const p3d_rmline_layer& l = layers[i];
        const bool first = i == 0, last = i == n_layers - 1;
        if (l.reserved != 0 || (i > 0 && l.Ci != layers[i - 1].Co)) return P3D_E_RANGE;
        if (first && l.Ci == 4 && !hull) return P3D_E_ARG;
        const int lf = (first ? P3D_RMLINE_IN_STACK : 0) | (first && !mask_in ? P3D_RMLINE_IN_NO_MASK : 0) | (last ? P3D_RMLINE_OUT_PLANAR : 0) | (last && lerp ? P3D_RMLINE_OUT_LERP : 0);
        const int Hin = H + 2 * pad - 2 * i, Win = W + 2 * pad - 2 * i;
        const int rc = rm_conv_check(N, Hin, Win, first ? pad : 0, l.Ci, l.Co, l.act, l.slope, lf, l.plan, !first, true, mask != nullptr,
                                     first && l.Ci == 4, &cs[i], &ps[i]);
        if (rc) return rc;
        const int64_t nw = (int64_t)9 * l.Ci * l.Co;
        if (l.w_off < 0 || l.b_off < 0 || nw > weight_floats || l.w_off > weight_floats - nw || l.b_off > weight_floats - l.Co) return P3D_E_RANGE;
        if (!last && (int64_t)N * (Hin - 2) * (Win - 2) * l.Co > act_floats) return P3D_E_RANGE;
        RmConv& c = cs[i];
        c.x = first ? nullptr : (i & 1 ? act0 : act1);
        c.out = last ? out : (i & 1 ? act1 : act0);
        c.image = first || (last && lerp) ? img3 : nullptr;
        c.mask = (first && mask_in) || (last && lerp) ? mask : nullptr;
        c.hull = first && l.Ci == 4 ? hull : nullptr;
        c.wk = weights + l.w_off, c.bias = weights + l.b_off;
    }
    if (dog) {
        hipLaunchKernelGGL(k_rm_mask, mgrid, dim3(RM_WG), 0, (hipStream_t)stream, m);
        const int rc = (int)hipGetLastError();
        if (rc) return rc;
        if (launches) ++*launches;
    }
    for (int i = 0; i < n_layers; ++i) {
        const int rc = rm_conv_launch(cs[i], ps[i], N, (hipStream_t)stream);
        if (rc) return rc;
        if (launches) ++*launches;
    }
    return 0;
}
