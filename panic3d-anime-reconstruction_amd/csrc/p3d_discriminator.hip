// p3d_discriminator.hip — the dual discriminator's layers (include/p3d_discriminator.h).
//
//   k_conv2d_act   Conv2dLayer's forward: the strided correlation's tile loop of p3d_corr_tile.hpp (the one the data gradient
//                  k_sg_dgrad runs) with the layer's epilogue in its store: + bias, lrelu, * gain, clamp, + residual;
//   k_mbstd        one workgroup per (group, statistic): mean and deviation over the group per (channel, pixel), the deviation map
//                  kept, its mean (lane-strided sums, then a fixed tree) broadcast into the statistic channel; optionally the copy of
//                  the group's own channels into the concatenated tensor;
//   k_mbstd_bwd    the same workgroup: the statistic's cotangent summed in a fixed order, then its share for every x.
// Every sum runs in a fixed order: the results are bitwise reproducible for the same sizes.
#include <hip/hip_runtime.h>

#include "../../include/p3d_discriminator.h"
#include "p3d_corr_tile.hpp"

struct DcEpilogue {
    const float* bias;
    const float* res;
    float* pre;
    float* out;
    int act;
    float alpha, gain, clamp;
};

__global__ __launch_bounds__(SG_WG) void k_conv2d_act(SgCorr a, DcEpilogue e) {
    __shared__ float As[SG_KC][SG_LD];
    __shared__ float Bs[SG_KC][SG_LD];
    const int64_t P = (int64_t)a.Ho * a.Wo;
    sg_corr_tile(a, As, Bs, [&](int64_t n, int co, int64_t pc, float v) {
        if (e.bias) v = v + e.bias[co];
        if (e.act == 1) v = v < 0.f ? v * e.alpha : v;
        v = v * e.gain;
        if (e.clamp >= 0.f) v = __builtin_fminf(__builtin_fmaxf(v, -e.clamp), e.clamp);
        const int64_t o = (n * a.Co + co) * P + pc;
        if (e.pre) e.pre[o] = v;
        if (e.res) v = v + e.res[o];
        e.out[o] = v;
    });
}

// ---- minibatch standard deviation -------------------------------------------------------------------------------------------
struct MbStd {
    const float* x;
    int N, C, G, M, F, c;
    int64_t HW;
};

__device__ __forceinline__ float mb_mean(const MbStd& a, int m, int64_t off) {
    float s = 0.f;
    for (int g = 0; g < a.G; ++g) s += a.x[((int64_t)g * a.M + m) * a.C * a.HW + off];
    return s / (float)a.G;
}

__global__ __launch_bounds__(SG_WG) void k_mbstd(MbStd a, int concat, float* __restrict__ y, float* __restrict__ sd) {
    __shared__ float red[SG_WG];
    const int m = blockIdx.x / a.F, f = blockIdx.x % a.F;
    const int64_t E = (int64_t)a.c * a.HW;
    const int64_t ch0 = (int64_t)f * a.c * a.HW;  // the statistic's first channel; its c channels are contiguous: offset ch0 + e
    const int Cy = concat ? a.C + a.F : a.F;
    float sum = 0.f;
    for (int64_t e = threadIdx.x; e < E; e += SG_WG) {
        const int64_t off = ch0 + e;
        const float mu = mb_mean(a, m, off);
        float var = 0.f;
        for (int g = 0; g < a.G; ++g) {
            const int64_t n = (int64_t)g * a.M + m;
            const float v = a.x[n * a.C * a.HW + off];
            const float d = v - mu;
            var += d * d;
            if (concat) y[n * Cy * a.HW + off] = v;
        }
        const float s = sqrtf(var / (float)a.G + 1e-8f);
        sd[(int64_t)m * a.C * a.HW + off] = s;
        sum += s;
    }
    const float stat = sg_block_sum(sum, red) / (float)E;
    for (int g = 0; g < a.G; ++g) {
        float* row = y + (((int64_t)g * a.M + m) * Cy + (concat ? a.C : 0) + f) * a.HW;
        for (int64_t p = threadIdx.x; p < a.HW; p += SG_WG) row[p] = stat;
    }
}

__global__ __launch_bounds__(SG_WG) void k_mbstd_bwd(MbStd a, const float* __restrict__ sd, const float* __restrict__ g_extra,
                                                     int64_t g_stride, float* __restrict__ g_x) {
    __shared__ float red[SG_WG];
    const int m = blockIdx.x / a.F, f = blockIdx.x % a.F;
    const int64_t E = (int64_t)a.c * a.HW;
    const int64_t ch0 = (int64_t)f * a.c * a.HW;
    float sum = 0.f;
    for (int g = 0; g < a.G; ++g) {
        const float* row = g_extra + ((int64_t)g * a.M + m) * g_stride + (int64_t)f * a.HW;
        for (int64_t p = threadIdx.x; p < a.HW; p += SG_WG) sum += row[p];
    }
    const float gs = sg_block_sum(sum, red);
    for (int64_t e = threadIdx.x; e < E; e += SG_WG) {
        const int64_t off = ch0 + e;
        const float mu = mb_mean(a, m, off);
        const float den = (float)a.G * sd[(int64_t)m * a.C * a.HW + off] * (float)E;
        for (int g = 0; g < a.G; ++g) {
            const int64_t o = ((int64_t)g * a.M + m) * a.C * a.HW + off;
            g_x[o] = gs * (a.x[o] - mu) / den;
        }
    }
}

// ---- entry points -----------------------------------------------------------------------------------------------------------
extern "C" int p3d_conv2d_act_f32(const float* x, int N, int Ci, int Hi, int Wi, const float* wk, int taps, int Co, int Ho, int Wo,
                                  int stride, int pad, const float* bias, int act, float alpha, float gain, float clamp, const float* res,
                                  float* pre_out, float* out, void* stream) {
    if (!x || !wk || !out) return P3D_E_ARG;
    if (N <= 0 || Ci <= 0 || Hi <= 0 || Wi <= 0 || Co <= 0 || Ho <= 0 || Wo <= 0) return P3D_E_ARG;
    if ((taps != 1 && taps != 9) || (stride != 1 && stride != 2) || pad < 0 || pad > 2 || (act != 0 && act != 1)) return P3D_E_RANGE;
    const int k = taps == 9 ? 3 : 1;
    if (Hi + 2 * pad < k || Wi + 2 * pad < k) return P3D_E_RANGE;
    if (Ho != (Hi + 2 * pad - k) / stride + 1 || Wo != (Wi + 2 * pad - k) / stride + 1) return P3D_E_RANGE;
    dim3 grid;
    if (!sg_corr_grid(N, Co, Ho, Wo, &grid)) return P3D_E_RANGE;
    const SgCorr a = {x, wk, Ci, Hi, Wi, taps, Co, Ho, Wo, stride, pad};
    const DcEpilogue e = {bias, res, pre_out, out, act, alpha, gain, clamp};
    hipLaunchKernelGGL(k_conv2d_act, grid, dim3(SG_WG), 0, (hipStream_t)stream, a, e);
    return (int)hipGetLastError();
}

static int mb_args(const float* x, int N, int C, int64_t HW, int group, int F, MbStd* a) {
    if (N <= 0 || C <= 0 || HW <= 0 || group <= 0 || F <= 0) return P3D_E_ARG;
    const int G = group < N ? group : N;
    if (N % G != 0 || C % F != 0) return P3D_E_RANGE;
    if ((int64_t)(N / G) * F > SG_MAX_GRID || (int64_t)N * (C + F) >= ((int64_t)1 << 40) / HW) return P3D_E_RANGE;
    a->x = x; a->N = N; a->C = C; a->G = G; a->M = N / G; a->F = F; a->c = C / F; a->HW = HW;
    return 0;
}

extern "C" int p3d_mbstd_f32(const float* x, int N, int C, int64_t HW, int group, int F, int concat, float* y, float* sd, void* stream) {
    if (!x || !y || !sd) return P3D_E_ARG;
    MbStd a;
    const int rc = mb_args(x, N, C, HW, group, F, &a);
    if (rc) return rc;
    hipLaunchKernelGGL(k_mbstd, dim3((unsigned)(a.M * F)), dim3(SG_WG), 0, (hipStream_t)stream, a, concat, y, sd);
    return (int)hipGetLastError();
}

extern "C" int p3d_mbstd_backward_f32(const float* x, const float* sd, const float* g_extra, int64_t g_extra_stride, int N, int C,
                                      int64_t HW, int group, int F, float* g_x, void* stream) {
    if (!x || !sd || !g_extra || !g_x) return P3D_E_ARG;
    MbStd a;
    const int rc = mb_args(x, N, C, HW, group, F, &a);
    if (rc) return rc;
    if (g_extra_stride < (int64_t)F * HW) return P3D_E_RANGE;
    hipLaunchKernelGGL(k_mbstd_bwd, dim3((unsigned)(a.M * F)), dim3(SG_WG), 0, (hipStream_t)stream, a, sd, g_extra, g_extra_stride, g_x);
    return (int)hipGetLastError();
}
