// p3d_r1.hip — the R1 penalty's device operators (include/p3d_r1.h).
//
//   k_conv2d_mask   the tangent layer: the strided correlation's tile loop of p3d_corr_tile.hpp (the one k_conv2d_act and k_sg_dgrad
//                   run) with the bias_act backward's rule sg_gz in its store, the mask read from the layer's saved output;
//   k_mbstd_bwd2    one workgroup per (group, statistic), like k_mbstd_bwd: the statistic's cotangent summed, then per (channel, pixel)
//                   the group's centred differences and the two results, in binary64;
//   k_r1_sumsq      one workgroup per sample: the squares of both gradient tensors summed in binary64.
// Every sum runs in a fixed order: the results are bitwise reproducible for the same sizes.
#include <hip/hip_runtime.h>

#include "../../include/p3d_r1.h"
#include "p3d_corr_tile.hpp"

__global__ __launch_bounds__(SG_WG) void k_conv2d_mask(SgCorr a, const float* pre, int act, float alpha, float gain, float clamp,
                                                       float* out) {
    __shared__ float As[SG_KC][SG_LD];
    __shared__ float Bs[SG_KC][SG_LD];
    const int64_t P = (int64_t)a.Ho * a.Wo;
    sg_corr_tile(a, As, Bs, [&](int64_t n, int co, int64_t pc, float v) {
        const int64_t o = (n * a.Co + co) * P + pc;
        out[o] = sg_gz(pre[o], v, act, alpha, gain, clamp);
    });
}

__device__ __forceinline__ double r1_block_sum(double v, double* red) {
    // fixed-order tree over the workgroup's SG_WG lanes
    const int tid = threadIdx.x;
    __syncthreads();  // red may still be read from an earlier sum
    red[tid] = v;
    __syncthreads();
    for (int s = SG_WG / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] = red[tid] + red[tid + s];
        __syncthreads();
    }
    return red[0];
}

struct Mb2 {
    const float* x;
    const float* g_extra;
    const float* h;
    int64_t g_stride, HW;
    int C, G, M, F, c;
};

__global__ __launch_bounds__(SG_WG) void k_mbstd_bwd2(Mb2 a, float* __restrict__ g_gextra, float* __restrict__ g_x2) {
    __shared__ double red[SG_WG];
    const int m = blockIdx.x / a.F, f = blockIdx.x % a.F;
    const int64_t E = (int64_t)a.c * a.HW;
    const int64_t ch0 = (int64_t)f * a.c * a.HW;  // the statistic's c channels are contiguous: offset ch0 + e
    const double G = (double)a.G, kE = 1.0 / (G * (double)E);
    double sum = 0.0;
    for (int g = 0; g < a.G; ++g) {
        const float* row = a.g_extra + ((int64_t)g * a.M + m) * a.g_stride + (int64_t)f * a.HW;
        for (int64_t p = threadIdx.x; p < a.HW; p += SG_WG) sum += (double)row[p];
    }
    const double gs = r1_block_sum(sum, red);
    double acc = 0.0;
    for (int64_t e = threadIdx.x; e < E; e += SG_WG) {
        const int64_t off = ch0 + e;
        double mu = 0.0, hbar = 0.0;
        for (int g = 0; g < a.G; ++g) {
            const int64_t o = ((int64_t)g * a.M + m) * a.C * a.HW + off;
            mu += (double)a.x[o];
            hbar += (double)a.h[o];
        }
        mu /= G;
        hbar /= G;
        double var = 0.0, s = 0.0;
        for (int g = 0; g < a.G; ++g) {
            const int64_t o = ((int64_t)g * a.M + m) * a.C * a.HW + off;
            const double d = (double)a.x[o] - mu;
            var += d * d;
            s += ((double)a.h[o] - hbar) * d;
        }
        const double sd = sqrt(var / G + 1e-8);
        acc += s / sd;
        const double q = s / (G * sd * sd * sd);
        for (int g = 0; g < a.G; ++g) {
            const int64_t o = ((int64_t)g * a.M + m) * a.C * a.HW + off;
            const double d = (double)a.x[o] - mu;
            g_x2[o] = (float)(kE * gs * (((double)a.h[o] - hbar) / sd - d * q));
        }
    }
    const float gg = (float)(kE * r1_block_sum(acc, red));
    for (int g = 0; g < a.G; ++g) {
        float* row = g_gextra + (((int64_t)g * a.M + m) * a.F + f) * a.HW;
        for (int64_t p = threadIdx.x; p < a.HW; p += SG_WG) row[p] = gg;
    }
}

__global__ __launch_bounds__(SG_WG) void k_r1_sumsq(const float* __restrict__ a, int64_t Ea, const float* __restrict__ b, int64_t Eb,
                                                    float* __restrict__ out) {
    __shared__ double red[SG_WG];
    const int64_t n = blockIdx.x;
    double sum = 0.0;
    const float* ar = a + n * Ea;
    for (int64_t e = threadIdx.x; e < Ea; e += SG_WG) sum += (double)ar[e] * (double)ar[e];
    if (b) {
        const float* br = b + n * Eb;
        for (int64_t e = threadIdx.x; e < Eb; e += SG_WG) sum += (double)br[e] * (double)br[e];
    }
    const double tot = r1_block_sum(sum, red);
    if (threadIdx.x == 0) out[n] = (float)tot;
}

// ---- entry points -----------------------------------------------------------------------------------------------------------
extern "C" int p3d_conv2d_mask_f32(const float* h, int N, int Ci, int Hi, int Wi, const float* wk, int taps, int Co, int Ho, int Wo,
                                   int stride, int pad, const float* pre, int act, float alpha, float gain, float clamp, float* out,
                                   void* stream) {
    if (!h || !wk || !pre || !out) return P3D_E_ARG;
    if (N <= 0 || Ci <= 0 || Hi <= 0 || Wi <= 0 || Co <= 0 || Ho <= 0 || Wo <= 0) return P3D_E_ARG;
    if ((taps != 1 && taps != 9) || (stride != 1 && stride != 2) || pad < 0 || pad > 2 || (act != 0 && act != 1)) return P3D_E_RANGE;
    const int k = taps == 9 ? 3 : 1;
    if (Hi + 2 * pad < k || Wi + 2 * pad < k) return P3D_E_RANGE;
    if (Ho != (Hi + 2 * pad - k) / stride + 1 || Wo != (Wi + 2 * pad - k) / stride + 1) return P3D_E_RANGE;
    dim3 grid;
    if (!sg_corr_grid(N, Co, Ho, Wo, &grid)) return P3D_E_RANGE;
    const SgCorr a = {h, wk, Ci, Hi, Wi, taps, Co, Ho, Wo, stride, pad};
    hipLaunchKernelGGL(k_conv2d_mask, grid, dim3(SG_WG), 0, (hipStream_t)stream, a, pre, act, alpha, gain, clamp, out);
    return (int)hipGetLastError();
}

extern "C" int p3d_mbstd_backward2_f32(const float* x, const float* g_extra, int64_t g_extra_stride, const float* h, int N, int C,
                                       int64_t HW, int group, int F, float* g_gextra, float* g_x2, void* stream) {
    if (!x || !g_extra || !h || !g_gextra || !g_x2) return P3D_E_ARG;
    if (N <= 0 || C <= 0 || HW <= 0 || group <= 0 || F <= 0) return P3D_E_ARG;
    const int G = group < N ? group : N;
    if (N % G != 0 || C % F != 0) return P3D_E_RANGE;
    if ((int64_t)(N / G) * F > SG_MAX_GRID || (int64_t)N * (C + F) >= ((int64_t)1 << 40) / HW) return P3D_E_RANGE;
    if (g_extra_stride < (int64_t)F * HW) return P3D_E_RANGE;
    const Mb2 a = {x, g_extra, h, g_extra_stride, HW, C, G, N / G, F, C / F};
    hipLaunchKernelGGL(k_mbstd_bwd2, dim3((unsigned)(a.M * F)), dim3(SG_WG), 0, (hipStream_t)stream, a, g_gextra, g_x2);
    return (int)hipGetLastError();
}

extern "C" int p3d_r1_sumsq_f32(const float* a, int64_t Ea, const float* b, int64_t Eb, int N, float* out, void* stream) {
    if (!a || !out) return P3D_E_ARG;
    if (N <= 0 || Ea <= 0 || Eb < 0 || (b == nullptr) != (Eb == 0)) return P3D_E_ARG;
    if (N > SG_MAX_GRID || Ea >= ((int64_t)1 << 40) / N || Eb >= ((int64_t)1 << 40) / N) return P3D_E_RANGE;
    hipLaunchKernelGGL(k_r1_sumsq, dim3((unsigned)N), dim3(SG_WG), 0, (hipStream_t)stream, a, Ea, b, Eb, out);
    return (int)hipGetLastError();
}
