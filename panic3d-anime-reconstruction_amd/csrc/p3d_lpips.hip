// p3d_lpips.hip — LPIPS, the AlexNet perceptual distance (include/p3d_lpips.h).
//
//   k_lpips_conv<LP_FWD>    convolution + bias + ReLU (optionally the scaling layer as the input is read): an implicit GEMM of
//                           64 channels x 64 pixels per workgroup over K = (tap, input channel) FLATTENED, in chunks of 64
//                           consecutive pairs (the 3-channel stem packs pairs, it pads no channels), the next chunk's operands in
//                           flight in registers while the matrix cores work on this one (sg_mma_chunk of p3d_corr_tile.hpp);
//   k_lpips_conv<LP_BWD1>,  a stride-1 layer's data gradient: the same loop over the cotangent — one finished tensor, or
//   k_lpips_conv<LP_BWD3>   a > 0 ? g_in + g_head : 0 formed from its parts — and the flipped, transposed weights; a plain store;
//   k_lpips_conv_bwd_phase  a strided layer's data gradient (the stem): one workgroup per 256 input pixels of one phase, the
//                           phase's taps alone, their weights in LDS, on the vector unit;
//   k_lpips_pool, k_lpips_pool_bwd   the 3 x 3 stride-2 maximum and its backward as a gather (first maximum in scan order);
//   k_lpips_head_d, k_lpips_head_mean, k_lpips_head_bwd   the normalised, weighted feature distance of one layer.
// Every sum runs in a fixed order and nothing is accumulated with atomics: the results are bitwise reproducible for the same sizes.
#include <hip/hip_runtime.h>

#include "../../include/p3d_lpips.h"
#include "p3d_corr_tile.hpp"

#define LP_KC 64  // K staged through LDS at a time: four of sg_mma_chunk's steps; sixteen operands per lane in flight meanwhile

// ---- the convolution's tile loop ------------------------------------------------------------------------------------------------
// in [N][Ci][Hi][Wi], wk [k^2][Ci][Co] -> [N][Co][Ho][Wo]; blockIdx = (pixel tile, channel tile, sample).  What `in` is:
//   LP_FWD   x, through the scaling layer when scale is given;
//   LP_BWD1  x as it is: a cotangent that is finished already (one tensor to read);
//   LP_BWD3  (mask == NULL || mask > 0) ? x (+ x2 when has2) : 0: the cotangent formed from its parts as they are read.
enum { LP_FWD = 0, LP_BWD1 = 1, LP_BWD3 = 2 };

struct LpConv {
    const float* x;
    const float* x2;     // LP_BWD3; a valid pointer also when has2 == 0 (the loads are unconditional, the value is dropped)
    const float* mask;   // LP_BWD3; likewise when has_mask == 0
    int has2, has_mask;
    const float* shift;  // LP_FWD: the scaling layer (both or neither)
    const float* scale;
    const float* wk;
    int Ci, Hi, Wi, k, Co, Ho, Wo, stride, pad;
    int K;  // k * k * Ci
};

// the cotangent of a layer's pre-activation: a > 0 ? g_in + g_head : 0 (a NULL pointer contributes 0; a NULL: nothing is masked here)
__device__ __forceinline__ float lp_cotangent(const float* g_in, const float* g_head, const float* a, int64_t idx) {
    float g = g_in ? g_in[idx] : 0.f;
    if (g_head) g = g + g_head[idx];
    return (!a || a[idx] > 0.f) ? g : 0.f;
}

template <int MODE, typename Store>
__device__ __forceinline__ void lp_conv_tile(const LpConv& c, float (*As)[SG_LD], float (*Bs)[SG_LD], Store store) {
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
    const int64_t P = (int64_t)c.Ho * c.Wo;
    const int64_t p0 = (int64_t)blockIdx.x * SG_TILE;
    const int co0 = blockIdx.y * SG_TILE;
    const int64_t n = blockIdx.z;
    const int64_t plane = (int64_t)c.Hi * c.Wi;
    const int64_t base = n * c.Ci * plane;
    const int col = lane;  // this lane stages column `col` of rows wave, wave + 4, ..., wave + LP_KC - 4 of a chunk
    const int64_t p = p0 + col;
    const bool pin = p < P;
    const int oy = pin ? (int)(p / c.Wo) : 0, ox = pin ? (int)(p % c.Wo) : 0;
    const int by = c.stride * oy - c.pad, bx = c.stride * ox - c.pad;
    const bool co_in = co0 + col < c.Co;
    // the K index this wave fetches next and its (ty, tx, ci): wave-uniform, stepped by 4 on the scalar unit (no division in the loop)
    int kidx = wave, kci = wave % c.Ci, ktx = (wave / c.Ci) % c.k, kty = (wave / c.Ci) / c.k;
    // fetch() only ISSUES loads — every one unconditional, from a clamped index (element 0 where the operand is out of range), so that
    // all of a chunk's loads are in flight together; commit() turns what arrived into operands (the predicates, the scaling layer, the
    // cotangent's sum and mask) as it writes them to LDS.  A load under a branch, or a value tested right after its load, makes the
    // compiler wait for each load in turn: sixteen round trips per chunk instead of one.
    float ra[LP_KC / 4], rb[LP_KC / 4], rb2[LP_KC / 4], rbm[LP_KC / 4];
    int rci[LP_KC / 4];
    unsigned pa = 0, pb = 0;
    auto fetch = [&]() {
        pa = pb = 0;
#pragma unroll
        for (int j = 0; j < LP_KC / 4; ++j) {
            const bool kin = kidx < c.K;
            const bool wa = kin && co_in;
            ra[j] = c.wk[wa ? (int64_t)kidx * c.Co + co0 + col : 0];
            pa |= (unsigned)wa << j;
            const int iy = by + kty, ix = bx + ktx;
            const bool wb = kin && pin && iy >= 0 && iy < c.Hi && ix >= 0 && ix < c.Wi;
            const int64_t idx = wb ? base + kci * plane + (int64_t)iy * c.Wi + ix : 0;
            rb[j] = c.x[idx];
            if (MODE == LP_BWD3) {
                rb2[j] = c.x2[idx];
                rbm[j] = c.mask[idx];
            }
            pb |= (unsigned)wb << j;
            rci[j] = kin ? kci : 0;
            kidx += 4;
            kci += 4;
            while (kci >= c.Ci) {
                kci -= c.Ci;
                if (++ktx == c.k) {
                    ktx = 0;
                    ++kty;
                }
            }
        }
    };
    sg_f32x4 acc[2][2];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v) acc[u][v] = sg_f32x4{0.f, 0.f, 0.f, 0.f};
    fetch();
    for (int k0 = 0; k0 < c.K; k0 += LP_KC) {
#pragma unroll
        for (int j = 0; j < LP_KC / 4; ++j) {  // commit
            float b = rb[j];
            if (MODE == LP_FWD && c.scale) b = (b - c.shift[rci[j]]) / c.scale[rci[j]];
            if (MODE == LP_BWD3) {
                b = c.has2 ? b + rb2[j] : b;
                b = (!c.has_mask || rbm[j] > 0.f) ? b : 0.f;
            }
            As[wave + 4 * j][col] = (pa >> j & 1) ? ra[j] : 0.f;
            Bs[wave + 4 * j][col] = (pb >> j & 1) ? b : 0.f;
        }
        __syncthreads();
        if (k0 + LP_KC < c.K) fetch();
#pragma unroll
        for (int s = 0; s < LP_KC; s += SG_KC) sg_mma_chunk(As + s, Bs + s, acc, wm, wn, lane);
        __syncthreads();
    }
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int co = co0 + wm + 16 * mi + 4 * (lane >> 4) + r;
                const int64_t pc = p0 + wn + 16 * ni + (lane & 15);
                if (co < c.Co && pc < P) store(n, co, pc, acc[mi][ni][r]);
            }
}

template <int MODE>
__global__ __launch_bounds__(SG_WG) void k_lpips_conv(LpConv c, const float* __restrict__ bias, float* __restrict__ out) {
    __shared__ float As[LP_KC][SG_LD];
    __shared__ float Bs[LP_KC][SG_LD];
    const int64_t P = (int64_t)c.Ho * c.Wo;
    lp_conv_tile<MODE>(c, As, Bs, [&](int64_t n, int co, int64_t pc, float v) {
        if (MODE == LP_FWD) v = __builtin_fmaxf(v + bias[co], 0.f);
        out[(n * c.Co + co) * P + pc] = v;
    });
}

// ---- a strided layer's data gradient, phase by phase ------------------------------------------------------------------------------
#define LP_PH_TAPS 6  // taps per axis of one phase: ceil(P3D_LPIPS_MAX_K / 2)
#define LP_PH_CO 64   // output channels staged at a time

struct LpPhase {
    const float* g_in;
    const float* g_head;
    const float* a;
    const float* wk;  // [k^2][Ci][Co]
    const float* scale;
    float* gx;
    int Co, Ho, Wo, k, Ci, Hi, Wi, stride, pad;
};

// ONE: the cotangent is one finished tensor (c.g_in); otherwise it is formed from its parts as they are read.
template <bool ONE>
__global__ __launch_bounds__(SG_WG) void k_lpips_conv_bwd_phase(LpPhase c) {
    __shared__ float Ws[LP_PH_TAPS * LP_PH_TAPS][P3D_LPIPS_BWD_MAX_CI][LP_PH_CO];
    const int tid = threadIdx.x;
    const int py = blockIdx.y / c.stride, px = blockIdx.y % c.stride;  // (y + pad) mod stride, (x + pad) mod stride
    const int64_t n = blockIdx.z;
    const int y0 = ((py - c.pad) % c.stride + c.stride) % c.stride, x0 = ((px - c.pad) % c.stride + c.stride) % c.stride;
    const int ny = y0 < c.Hi ? (c.Hi - y0 + c.stride - 1) / c.stride : 0, nx = x0 < c.Wi ? (c.Wi - x0 + c.stride - 1) / c.stride : 0;
    const int64_t cnt = (int64_t)ny * nx, e = (int64_t)blockIdx.x * SG_WG + tid;
    if ((int64_t)blockIdx.x * SG_WG >= cnt) return;  // the whole workgroup: this phase has fewer pixels than the largest one
    const bool active = e < cnt;
    const int y = active ? y0 + c.stride * (int)(e / nx) : 0, x = active ? x0 + c.stride * (int)(e % nx) : 0;
    const int qy = (y + c.pad - py) / c.stride, qx = (x + c.pad - px) / c.stride;  // exact; output row of tap jy: qy - jy
    const int nty = py < c.k ? (c.k - py + c.stride - 1) / c.stride : 0, ntx = px < c.k ? (c.k - px + c.stride - 1) / c.stride : 0;
    const int64_t oplane = (int64_t)c.Ho * c.Wo;
    float acc[P3D_LPIPS_BWD_MAX_CI] = {0.f, 0.f, 0.f, 0.f};
    for (int co0 = 0; co0 < c.Co; co0 += LP_PH_CO) {
        __syncthreads();
        for (int i = tid; i < nty * ntx * P3D_LPIPS_BWD_MAX_CI * LP_PH_CO; i += SG_WG) {
            const int cc = i % LP_PH_CO, ci = (i / LP_PH_CO) % P3D_LPIPS_BWD_MAX_CI, tt = i / (LP_PH_CO * P3D_LPIPS_BWD_MAX_CI);
            const int t = (py + c.stride * (tt / ntx)) * c.k + px + c.stride * (tt % ntx);
            Ws[tt][ci][cc] = (ci < c.Ci && co0 + cc < c.Co) ? c.wk[((int64_t)t * c.Ci + ci) * c.Co + co0 + cc] : 0.f;
        }
        __syncthreads();
        if (!active) continue;
        const int nco = c.Co - co0 < LP_PH_CO ? c.Co - co0 : LP_PH_CO;
        for (int jy = 0; jy < nty; ++jy) {
            const int oy = qy - jy;
            if (oy < 0 || oy >= c.Ho) continue;
            for (int jx = 0; jx < ntx; ++jx) {
                const int ox = qx - jx;
                if (ox < 0 || ox >= c.Wo) continue;
                const float(*w)[LP_PH_CO] = Ws[jy * ntx + jx];
                const int64_t o = (n * c.Co + co0) * oplane + (int64_t)oy * c.Wo + ox;
                for (int cc0 = 0; cc0 < nco; cc0 += 8) {  // eight channels' loads in flight, then their fmas in channel order
                    float gv[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const bool in = cc0 + u < nco;
                        const int64_t idx = o + (in ? cc0 + u : 0) * oplane;
                        const float g = ONE ? c.g_in[idx] : lp_cotangent(c.g_in, c.g_head, c.a, idx);
                        gv[u] = in ? g : 0.f;  // (the weights of the channels past Co are zeros in LDS)
                    }
#pragma unroll
                    for (int u = 0; u < 8; ++u)
#pragma unroll
                        for (int ci = 0; ci < P3D_LPIPS_BWD_MAX_CI; ++ci) acc[ci] = __builtin_fmaf(gv[u], w[ci][cc0 + u], acc[ci]);
                }
            }
        }
    }
    if (!active) return;
#pragma unroll
    for (int ci = 0; ci < P3D_LPIPS_BWD_MAX_CI; ++ci)
        if (ci < c.Ci) c.gx[((n * c.Ci + ci) * c.Hi + y) * c.Wi + x] = c.scale ? acc[ci] / c.scale[ci] : acc[ci];
}

// ---- the pool -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SG_WG) void k_lpips_pool(const float* __restrict__ x, int64_t total, int H, int W, int Ho, int Wo,
                                                      float* __restrict__ y) {
    const int64_t i = (int64_t)blockIdx.x * SG_WG + threadIdx.x;
    if (i >= total) return;
    const int ox = (int)(i % Wo), oy = (int)((i / Wo) % Ho);
    const float* w = x + (i / ((int64_t)Wo * Ho)) * H * W + (int64_t)(2 * oy) * W + 2 * ox;
    float best = w[0];
#pragma unroll
    for (int t = 1; t < 9; ++t) {
        const float v = w[(t / 3) * W + t % 3];
        if (v > best) best = v;
    }
    y[i] = best;
}

__global__ __launch_bounds__(SG_WG) void k_lpips_pool_bwd(const float* __restrict__ x, const float* __restrict__ g, int64_t total, int H,
                                                          int W, int Ho, int Wo, float* __restrict__ gx) {
    const int64_t i = (int64_t)blockIdx.x * SG_WG + threadIdx.x;
    if (i >= total) return;
    const int ix = (int)(i % W), iy = (int)((i / W) % H);
    const int64_t pl = i / ((int64_t)W * H);
    const float* xp = x + pl * H * W;
    const float* gp = g + pl * Ho * Wo;
    const float v = xp[(int64_t)iy * W + ix];
    const int oy_lo = iy >= 2 ? (iy - 1) / 2 : 0, oy_hi = iy / 2 < Ho - 1 ? iy / 2 : Ho - 1;
    const int ox_lo = ix >= 2 ? (ix - 1) / 2 : 0, ox_hi = ix / 2 < Wo - 1 ? ix / 2 : Wo - 1;
    float s = 0.f;
    for (int oy = oy_lo; oy <= oy_hi; ++oy)
        for (int ox = ox_lo; ox <= ox_hi; ++ox) {
            const float* w = xp + (int64_t)(2 * oy) * W + 2 * ox;
            const int me = (iy - 2 * oy) * 3 + (ix - 2 * ox);  // this pixel's place in the window's scan
            bool first = true;  // the first maximum: greater than everything before it, not less than anything after it
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const float u = w[(t / 3) * W + t % 3];
                if (t < me ? !(u < v) : (t > me && u > v)) first = false;
            }
            if (first) s = s + gp[(int64_t)oy * Wo + ox];
        }
    gx[i] = s;
}

// ---- the head -------------------------------------------------------------------------------------------------------------------
// 64 pixels x 4 channel quarters per workgroup: lane (tid & 63) is the pixel, wave q = tid >> 6 sums the channels q, q + 4, ...;
// the four partial sums meet in LDS and every wave forms ((q0 + q1) + q2) + q3 itself.
#define LP_HD_PX 64

__device__ __forceinline__ float lp_quarters(float (*red)[LP_HD_PX], float v, int q, int px) {
    __syncthreads();  // the previous round's reads are done
    red[q][px] = v;
    __syncthreads();
    return ((red[0][px] + red[1][px]) + red[2][px]) + red[3][px];
}

struct LpHead {
    const float* a0;
    const float* a1;
    const float* lin;
    int C;
    int64_t HW;
};

// (r0 + eps, r1 + eps, r0) of this lane's pixel; o: the pixel's offset in channel 0 of its sample
__device__ __forceinline__ void lp_head_norms(const LpHead& h, float (*red)[LP_HD_PX], int64_t o, bool in, int q, int px, float* i0,
                                              float* i1, float* r0) {
    float s0 = 0.f, s1 = 0.f;
    if (in)
        for (int c = q; c < h.C; c += 4) {
            const float v0 = h.a0[o + c * h.HW], v1 = h.a1[o + c * h.HW];
            s0 = s0 + v0 * v0;
            s1 = s1 + v1 * v1;
        }
    *r0 = sqrtf(lp_quarters(red, s0, q, px));
    *i0 = *r0 + P3D_LPIPS_EPS;
    *i1 = sqrtf(lp_quarters(red, s1, q, px)) + P3D_LPIPS_EPS;
}

__global__ __launch_bounds__(SG_WG) void k_lpips_head_d(LpHead h, float* __restrict__ d) {
    __shared__ float red[4][LP_HD_PX];
    const int px = threadIdx.x & 63, q = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t p = (int64_t)blockIdx.x * LP_HD_PX + px, n = blockIdx.y;
    const bool in = p < h.HW;
    const int64_t o = n * h.C * h.HW + p;
    float i0, i1, r0;
    lp_head_norms(h, red, o, in, q, px, &i0, &i1, &r0);
    float s = 0.f;
    if (in)
        for (int c = q; c < h.C; c += 4) {
            const float df = h.a0[o + c * h.HW] / i0 - h.a1[o + c * h.HW] / i1;
            s = s + h.lin[c] * (df * df);
        }
    s = lp_quarters(red, s, q, px);
    if (in && q == 0) d[n * h.HW + p] = s;
}

__global__ __launch_bounds__(SG_WG) void k_lpips_head_mean(const float* __restrict__ d, int64_t HW, float* __restrict__ v,
                                                           float* __restrict__ out, int accumulate) {
    __shared__ float red[SG_WG];
    const int64_t n = blockIdx.x;
    float s = 0.f;
    for (int64_t p = threadIdx.x; p < HW; p += SG_WG) s = s + d[n * HW + p];
    const float m = sg_block_sum(s, red) / (float)HW;
    if (threadIdx.x == 0) {
        v[n] = m;
        if (out) out[n] = accumulate ? out[n] + m : m;
    }
}

__global__ __launch_bounds__(SG_WG) void k_lpips_head_bwd(LpHead h, const float* __restrict__ g, const float* __restrict__ g_add,
                                                          int relu_mask, float* __restrict__ g_a0) {
    __shared__ float red[4][LP_HD_PX];
    const int px = threadIdx.x & 63, q = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t p = (int64_t)blockIdx.x * LP_HD_PX + px, n = blockIdx.y;
    const bool in = p < h.HW;
    const int64_t o = n * h.C * h.HW + p;
    float i0, i1, r0;
    lp_head_norms(h, red, o, in, q, px, &i0, &i1, &r0);
    const float gs = g[n] / (float)h.HW;
    float t = 0.f;
    if (in)
        for (int c = q; c < h.C; c += 4) {
            const float v0 = h.a0[o + c * h.HW];
            const float u = 2.f * h.lin[c] * (v0 / i0 - h.a1[o + c * h.HW] / i1) * gs;
            t = t + u * v0;
        }
    t = lp_quarters(red, t, q, px);
    if (!in) return;
    const float den = r0 * (i0 * i0);
    for (int c = q; c < h.C; c += 4) {
        const float v0 = h.a0[o + c * h.HW];
        const float u = 2.f * h.lin[c] * (v0 / i0 - h.a1[o + c * h.HW] / i1) * gs;
        float r = r0 > 0.f ? u / i0 - v0 * t / den : 0.f;
        if (g_add) r = g_add[o + c * h.HW] + r;
        g_a0[o + c * h.HW] = (!relu_mask || v0 > 0.f) ? r : 0.f;
    }
}

// ---- entry points -----------------------------------------------------------------------------------------------------------------
static const int64_t LP_MAX_ELEMS = (int64_t)1 << 40;

static int lp_conv_sizes(int N, int Ci, int Hi, int Wi, int k, int Co, int Ho, int Wo, int stride, int pad) {
    if (N <= 0 || Ci <= 0 || Hi <= 0 || Wi <= 0 || Co <= 0 || Ho <= 0 || Wo <= 0) return P3D_E_ARG;
    if (k < 1 || k > P3D_LPIPS_MAX_K || stride < 1 || stride > P3D_LPIPS_MAX_STRIDE || pad < 0 || pad >= k) return P3D_E_RANGE;
    if (Hi + 2 * pad < k || Wi + 2 * pad < k) return P3D_E_RANGE;
    if (Ho != (Hi + 2 * pad - k) / stride + 1 || Wo != (Wi + 2 * pad - k) / stride + 1) return P3D_E_RANGE;
    if ((int64_t)k * k * Ci > 0x7fffffff / 2 || (int64_t)k * k * Ci * Co > 0x7fffffff) return P3D_E_RANGE;
    if ((int64_t)N * Ci * Hi >= LP_MAX_ELEMS / Wi || (int64_t)N * Co * Ho >= LP_MAX_ELEMS / Wo) return P3D_E_RANGE;
    return 0;
}

extern "C" int p3d_lpips_conv_relu_f32(const float* x, int N, int Ci, int Hi, int Wi, const float* wk, int k, int Co, int Ho, int Wo,
                                       int stride, int pad, const float* bias, const float* shift, const float* scale, float* out,
                                       void* stream) {
    if (!x || !wk || !bias || !out || (shift == nullptr) != (scale == nullptr)) return P3D_E_ARG;
    const int rc = lp_conv_sizes(N, Ci, Hi, Wi, k, Co, Ho, Wo, stride, pad);
    if (rc) return rc;
    dim3 grid;
    if (!sg_corr_grid(N, Co, Ho, Wo, &grid)) return P3D_E_RANGE;
    const LpConv c = {x, x, x, 0, 0, shift, scale, wk, Ci, Hi, Wi, k, Co, Ho, Wo, stride, pad, k * k * Ci};
    hipLaunchKernelGGL(k_lpips_conv<LP_FWD>, grid, dim3(SG_WG), 0, (hipStream_t)stream, c, bias, out);
    return (int)hipGetLastError();
}

extern "C" int p3d_lpips_conv_relu_backward_f32(const float* g_in, const float* g_head, const float* a, int N, int Co, int Ho, int Wo,
                                                const float* wkb, int k, int Ci, int Hi, int Wi, int stride, int pad,
                                                const float* scale, float* gx, void* stream) {
    if ((!g_in && !g_head) || !wkb || !gx) return P3D_E_ARG;
    const int rc = lp_conv_sizes(N, Ci, Hi, Wi, k, Co, Ho, Wo, stride, pad);
    if (rc) return rc;
    if (stride == 1) {
        if (scale) return P3D_E_RANGE;  // the scaling layer sits in front of the strided stem only
        dim3 grid;
        if (!sg_corr_grid(N, Ci, Hi, Wi, &grid)) return P3D_E_RANGE;
        // a correlation of the cotangent [N][Co][Ho][Wo] with wkb [k^2][Co][Ci] and pad' = k - 1 - pad, giving [N][Ci][Hi][Wi]
        const float* g0 = g_in ? g_in : g_head;
        const int has2 = g_in && g_head;
        const LpConv c = {g0,      has2 ? g_head : g0, a ? a : g0, has2, a != nullptr, nullptr, nullptr, wkb, Co, Ho, Wo, k, Ci, Hi, Wi, 1,
                          k - 1 - pad, k * k * Co};
        if (has2 || a)
            hipLaunchKernelGGL(k_lpips_conv<LP_BWD3>, grid, dim3(SG_WG), 0, (hipStream_t)stream, c, (const float*)nullptr, gx);
        else
            hipLaunchKernelGGL(k_lpips_conv<LP_BWD1>, grid, dim3(SG_WG), 0, (hipStream_t)stream, c, (const float*)nullptr, gx);
        return (int)hipGetLastError();
    }
    if (Ci > P3D_LPIPS_BWD_MAX_CI || N > 65535) return P3D_E_RANGE;
    const int64_t per_phase = (int64_t)((Hi + stride - 1) / stride) * ((Wi + stride - 1) / stride);
    if ((per_phase + SG_WG - 1) / SG_WG > SG_MAX_GRID) return P3D_E_RANGE;
    const dim3 grid((unsigned)((per_phase + SG_WG - 1) / SG_WG), (unsigned)(stride * stride), (unsigned)N);
    if (!a && !(g_in && g_head)) {
        const LpPhase c = {g_in ? g_in : g_head, nullptr, nullptr, wkb, scale, gx, Co, Ho, Wo, k, Ci, Hi, Wi, stride, pad};
        hipLaunchKernelGGL(k_lpips_conv_bwd_phase<true>, grid, dim3(SG_WG), 0, (hipStream_t)stream, c);
    } else {
        const LpPhase c = {g_in, g_head, a, wkb, scale, gx, Co, Ho, Wo, k, Ci, Hi, Wi, stride, pad};
        hipLaunchKernelGGL(k_lpips_conv_bwd_phase<false>, grid, dim3(SG_WG), 0, (hipStream_t)stream, c);
    }
    return (int)hipGetLastError();
}

static int lp_pool_sizes(int64_t planes, int H, int W, int64_t* blocks_in, int64_t* blocks_out) {
    if (planes <= 0 || H <= 0 || W <= 0) return P3D_E_ARG;
    if (H < 3 || W < 3) return P3D_E_RANGE;
    if (planes >= LP_MAX_ELEMS / H / W) return P3D_E_RANGE;
    const int Ho = (H - 3) / 2 + 1, Wo = (W - 3) / 2 + 1;
    *blocks_in = (planes * H * W + SG_WG - 1) / SG_WG;
    *blocks_out = (planes * Ho * Wo + SG_WG - 1) / SG_WG;
    return *blocks_in > SG_MAX_GRID ? P3D_E_RANGE : 0;
}

extern "C" int p3d_lpips_pool_f32(const float* x, int64_t planes, int H, int W, float* y, void* stream) {
    if (!x || !y) return P3D_E_ARG;
    int64_t bi, bo;
    const int rc = lp_pool_sizes(planes, H, W, &bi, &bo);
    if (rc) return rc;
    const int Ho = (H - 3) / 2 + 1, Wo = (W - 3) / 2 + 1;
    hipLaunchKernelGGL(k_lpips_pool, dim3((unsigned)bo), dim3(SG_WG), 0, (hipStream_t)stream, x, planes * Ho * Wo, H, W, Ho, Wo, y);
    return (int)hipGetLastError();
}

extern "C" int p3d_lpips_pool_backward_f32(const float* x, const float* g, int64_t planes, int H, int W, float* gx, void* stream) {
    if (!x || !g || !gx) return P3D_E_ARG;
    int64_t bi, bo;
    const int rc = lp_pool_sizes(planes, H, W, &bi, &bo);
    if (rc) return rc;
    const int Ho = (H - 3) / 2 + 1, Wo = (W - 3) / 2 + 1;
    hipLaunchKernelGGL(k_lpips_pool_bwd, dim3((unsigned)bi), dim3(SG_WG), 0, (hipStream_t)stream, x, g, planes * H * W, H, W, Ho, Wo, gx);
    return (int)hipGetLastError();
}

static int lp_head_sizes(int N, int C, int64_t HW) {
    if (N <= 0 || C <= 0 || HW <= 0) return P3D_E_ARG;
    if (N > 65535 || (HW + LP_HD_PX - 1) / LP_HD_PX > SG_MAX_GRID || (int64_t)N * C >= LP_MAX_ELEMS / HW) return P3D_E_RANGE;
    return 0;
}

extern "C" size_t p3d_lpips_head_workspace_bytes(int N, int64_t HW) {
    if (lp_head_sizes(N, 1, HW)) return 0;
    return (size_t)N * (size_t)HW * sizeof(float);
}

extern "C" int p3d_lpips_head_f32(const float* a0, const float* a1, const float* lin, int N, int C, int64_t HW, float* v, float* out,
                                  int accumulate, void* workspace, size_t workspace_bytes, void* stream) {
    if (!a0 || !a1 || !lin || !v || !workspace) return P3D_E_ARG;
    const int rc = lp_head_sizes(N, C, HW);
    if (rc) return rc;
    if (workspace_bytes < p3d_lpips_head_workspace_bytes(N, HW)) return P3D_E_WORKSPACE;
    const LpHead h = {a0, a1, lin, C, HW};
    float* d = (float*)workspace;
    hipLaunchKernelGGL(k_lpips_head_d, dim3((unsigned)((HW + LP_HD_PX - 1) / LP_HD_PX), (unsigned)N), dim3(SG_WG), 0, (hipStream_t)stream, h, d);
    hipLaunchKernelGGL(k_lpips_head_mean, dim3((unsigned)N), dim3(SG_WG), 0, (hipStream_t)stream, (const float*)d, HW, v, out, accumulate);
    return (int)hipGetLastError();
}

extern "C" int p3d_lpips_head_backward_f32(const float* a0, const float* a1, const float* lin, const float* g, int N, int C, int64_t HW,
                                           const float* g_add, int relu_mask, float* g_a0, void* stream) {
    if (!a0 || !a1 || !lin || !g || !g_a0) return P3D_E_ARG;
    const int rc = lp_head_sizes(N, C, HW);
    if (rc) return rc;
    const LpHead h = {a0, a1, lin, C, HW};
    hipLaunchKernelGGL(k_lpips_head_bwd, dim3((unsigned)((HW + LP_HD_PX - 1) / LP_HD_PX), (unsigned)N), dim3(SG_WG), 0, (hipStream_t)stream, h,
                       g, g_add, relu_mask, g_a0);
    return (int)hipGetLastError();
}
