// p3d_rmline_grad.hip — the training operators of the illustration-to-render module (include/p3d_rmline_grad.h).
//
//   k_rm_bn_part / k_rm_bn_merge   per-channel batch statistics by a centred algorithm: per-workgroup (count, mean, M2) partials from
//                                  two passes, merged in a fixed order; the merge applies the running update and bumps the counter;
//   k_rm_bn_fold                   a train-mode batch norm folded into the next convolution's operands, on the device;
//   k_rm_dgrad<MB, R>              the data gradient as the forward's implicit GEMM (p3d_rmline_tile.hpp) over g with a zero halo in
//                                  the load and the weights transposed and tap-flipped while staged; its store fuses the batch norm's
//                                  two statistic terms and LeakyReLU's derivative;
//   k_rm_wgrad<SETS> / k_rm_wgrad_sum   the weight and bias gradient: per slice of patches a GEMM of 9 Ci x Co over the pixels on the
//                                  matrix cores, the slices' partials added in slice order;
//   k_rm_bn_coef                   the batch norm's parameter gradients and the two coefficients of the data gradient's store;
//   k_rm_head / k_rm_head_grad     lerp, L1 and the crop; their backward.
// Every sum runs in a fixed order and nothing is accumulated with atomics.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/p3d_rmline_grad.h"
#include "p3d_rmline_grad_plan.hpp"
#include "p3d_rmline_tile.hpp"

// ---- batch statistics -------------------------------------------------------------------------------------------------------------------
#define RM_BN_C 64  // channels a workgroup's row of lanes covers (P3D_RMLINE_MAX_C)

// A partial's moments: count, mean as hi + lo (lo the part of the mean that hi's rounding lost: on values of mean 100 and deviation 0.01
// a mean rounded to binary32 is off by up to 4e-6, and the merge's d = mb - ma would carry that into M2), M2 about hi + lo.
struct RmMoments {
    float n, hi, lo, m2;
};

// a and b merged, a first
__device__ __forceinline__ void rm_chan(RmMoments& a, const RmMoments& b) {
    if (b.n == 0.f) return;
    if (a.n == 0.f) {
        a = b;
        return;
    }
    const float n = a.n + b.n, d = (b.hi - a.hi) + (b.lo - a.lo), t = d * b.n / n;
    const float hi = a.hi + t, bb = hi - a.hi, err = (a.hi - (hi - bb)) + (t - bb);  // hi + err = a.hi + t exactly (two-sum)
    a.m2 = a.m2 + b.m2 + d * d * a.n * b.n / n;
    a.lo = err + a.lo, a.hi = hi, a.n = n;
}

__global__ __launch_bounds__(RM_WG) void k_rm_bn_part(const float* x, int64_t K, int C, int G, float* ws) {
    __shared__ RmMoments part[4][RM_BN_C];
    const int tid = threadIdx.x, c = tid & (RM_BN_C - 1), q = tid / RM_BN_C, g = blockIdx.x;
    const int64_t r0 = (int64_t)g * K / G, r1 = (int64_t)(g + 1) * K / G;
    RmMoments m = {0.f, 0.f, 0.f, 0.f};
    if (c < C) {
        float sum = 0.f;
        for (int64_t r = r0 + q; r < r1; r += 4) sum += x[r * C + c], m.n += 1.f;
        if (m.n > 0.f) {
            m.hi = sum / m.n;
            float res = 0.f;
            for (int64_t r = r0 + q; r < r1; r += 4) {
                const float d = x[r * C + c] - m.hi;
                res += d, m.m2 += d * d;
            }
            m.lo = res / m.n;
            m.m2 = m.m2 - res * m.lo;  // about hi + lo
        }
    }
    part[q][c] = m;
    __syncthreads();
    if (q == 0 && c < C) {
        for (int j = 1; j < 4; ++j) rm_chan(m, part[j][c]);
        float* o = ws + (int64_t)g * 4 * RM_BN_C;
        o[c] = m.n, o[RM_BN_C + c] = m.hi, o[2 * RM_BN_C + c] = m.lo, o[3 * RM_BN_C + c] = m.m2;
    }
}

__global__ __launch_bounds__(RM_BN_C) void k_rm_bn_merge(const float* ws, int G, int64_t K, int C, float momentum, float* mean_out, float* var_out,
                                                         float* rmean, float* rvar, int64_t* counter) {
    const int c = threadIdx.x;
    if (c == 0 && counter) *counter += 1;
    if (c >= C) return;
    RmMoments m = {0.f, 0.f, 0.f, 0.f};
    for (int g = 0; g < G; ++g) {
        const float* o = ws + (int64_t)g * 4 * RM_BN_C;
        rm_chan(m, RmMoments{o[c], o[RM_BN_C + c], o[2 * RM_BN_C + c], o[3 * RM_BN_C + c]});
    }
    const float mean = m.hi + m.lo, m2 = m.m2 < 0.f ? 0.f : m.m2;
    mean_out[c] = mean;
    var_out[c] = m2 / (float)K;
    if (rmean) {
        rmean[c] = (1.f - momentum) * rmean[c] + momentum * mean;
        rvar[c] = (1.f - momentum) * rvar[c] + momentum * (m2 / (float)(K - 1));
    }
}

extern "C" int p3d_rmline_bn_stats_f32(const float* x, int64_t K, int C, float momentum, float* mean, float* var, float* running_mean,
                                       float* running_var, int64_t* counter, float* ws, int64_t ws_floats, void* stream) {
    if (!x || !mean || !var || !ws || K <= 0 || C <= 0) return P3D_E_ARG;
    if ((running_mean != nullptr) != (running_var != nullptr) || (running_mean != nullptr) != (counter != nullptr)) return P3D_E_ARG;
    if (!isfinite(momentum) || momentum < 0.f || momentum > 1.f) return P3D_E_ARG;
    if (C > P3D_RMLINE_MAX_C || K == 1 || K >= ((int64_t)1 << 31) / C) return P3D_E_RANGE;
    if (ws_floats < (int64_t)P3D_RMLINE_BN_MAX_GROUPS * 4 * RM_BN_C) return P3D_E_WORKSPACE;
    int64_t G = (K + P3D_RMLINE_BN_ROWS - 1) / P3D_RMLINE_BN_ROWS;
    if (G > P3D_RMLINE_BN_MAX_GROUPS) G = P3D_RMLINE_BN_MAX_GROUPS;
    hipLaunchKernelGGL(k_rm_bn_part, dim3((unsigned)G), dim3(RM_WG), 0, (hipStream_t)stream, x, K, C, (int)G, ws);
    int rc = (int)hipGetLastError();
    if (rc) return rc;
    hipLaunchKernelGGL(k_rm_bn_merge, dim3(1), dim3(RM_BN_C), 0, (hipStream_t)stream, (const float*)ws, (int)G, K, C, momentum, mean, var,
                       running_mean, running_var, counter);
    return (int)hipGetLastError();
}

// s + c <- s + c + a b with the product's and the sum's rounding errors kept in c (Ogita, Rump and Oishi's Dot2, in binary32): the
// folded bias shifts EVERY pixel of a layer alike, and the coefficients' two sums feed a difference that cancels (ds - mean dt): their
// own rounding must not be what is left
__device__ __forceinline__ void rm_dot2(float a, float b, float& s, float& c) {
    const float p = a * b, pe = __builtin_fmaf(a, b, -p);
    const float t = s + p, bb = t - s, se = (s - (t - bb)) + (p - bb);
    s = t;
    c = c + (pe + se);
}

// ---- the fold -----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RM_WG) void k_rm_bn_fold(const float* w, const float* bias, const float* gamma, const float* beta, const float* mean,
                                                      const float* var, float eps, int Ci, int Co, float* wk, float* bias_f) {
    __shared__ float s[P3D_RMLINE_MAX_C], sh[P3D_RMLINE_MAX_C];
    const int tid = threadIdx.x;
    if (tid < Ci) {
        float sc = 1.f, sf = 0.f;
        if (gamma) {
            const float r = 1.f / sqrtf(var[tid] + eps);
            sc = gamma[tid] * r;
            sf = beta[tid] - mean[tid] * sc;
        }
        s[tid] = sc, sh[tid] = sf;
    }
    __syncthreads();
    for (int i = tid; i < 9 * Ci * Co; i += RM_WG) {  // i walks wk [t][ci][co]
        const int co = i % Co, ci = (i / Co) % Ci, t = i / (Co * Ci);
        const float v = w[((int64_t)co * Ci + ci) * 9 + t];
        wk[i] = gamma ? v * s[ci] : v;
    }
    if (tid < Co) {
        float b = bias[tid];
        if (gamma) {
            float acc = 0.f, cor = 0.f;
            for (int t = 0; t < 9; ++t)
                for (int ci = 0; ci < Ci; ++ci) rm_dot2(w[((int64_t)tid * Ci + ci) * 9 + t], sh[ci], acc, cor);
            b = b + (acc + cor);
        }
        bias_f[tid] = b;
    }
}

extern "C" int p3d_rmline_bn_fold_f32(const float* w, const float* bias, const float* gamma, const float* beta, const float* mean,
                                      const float* var, float eps, int Ci, int Co, float* wk, float* bias_f, void* stream) {
    if (!w || !bias || !wk || !bias_f || Ci <= 0 || Co <= 0) return P3D_E_ARG;
    if (gamma && (!beta || !mean || !var || !isfinite(eps) || eps < 0.f)) return P3D_E_ARG;
    if (Ci > P3D_RMLINE_MAX_C || Co > P3D_RMLINE_MAX_C) return P3D_E_RANGE;
    hipLaunchKernelGGL(k_rm_bn_fold, dim3(1), dim3(RM_WG), 0, (hipStream_t)stream, w, bias, gamma, beta, mean, var, eps, Ci, Co, wk, bias_f);
    return (int)hipGetLastError();
}

// ---- the data gradient ------------------------------------------------------------------------------------------------------------------
// RmConv's roles here: x = g, (Hin, Win) = g's map, Ci = g's channels (the GEMM's k), Co = the layer's INPUT channels (the GEMM's rows),
// (Ho, Wo) = g's map + 2; wk the layer's own [9][Co][Ci] in these names.
struct RmDgrad {
    RmConv c;
    const float* a;
    const float* c0;
    const float* c1;
};

template <int MB, int R>
__global__ __launch_bounds__(RM_WG) void k_rm_dgrad(RmDgrad d) {
    const RmConv& c = d.c;
    constexpr int COT = 16 * MB, PH = 4 * R + 2, NB = 2 * R;
    extern __shared__ __attribute__((aligned(16))) float rm_lds[];
    float* Xs = rm_lds;                       // [PH][RM_PW][cip]: g's patch with its zero halo
    float* Ws = rm_lds + PH * RM_PW * c.cip;  // [9][COT][cip]: Ws[t'][ci][co] = wk[8 - t'][ci][co]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = blockIdx.z, m0 = blockIdx.y * COT;
    const int x0 = (blockIdx.x % c.tiles_x) * RM_TW, y0 = (blockIdx.x / c.tiles_x) * (4 * R);
    for (int i = tid; i < 9 * COT * c.ci4; i += RM_WG) {
        const int k = i % c.ci4, m = (i / c.ci4) % COT, tap = i / (c.ci4 * COT);
        const bool in = m0 + m < c.Co && k < c.Ci;
        const float v = c.wk[in ? ((int64_t)(8 - tap) * c.Co + m0 + m) * c.Ci + k : 0];
        Ws[(tap * COT + m) * c.cip + k] = in ? v : 0.f;
    }
    rm_stage_cl(c, n, y0, x0, 2, PH, Xs, c.cip, c.ci4);
    __syncthreads();
    rm_f32x4 acc[MB][NB];
#pragma unroll
    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[mb][nb] = rm_f32x4{0.f, 0.f, 0.f, 0.f};
    rm_tile_mma<MB, R, true>(Xs, Ws, c.cip, c.ci4, wave, lane, acc);  // per-tap chains: see the header
    const int l15 = lane & 15, kq = lane >> 4;
    const bool planar = (c.flags & P3D_RMLINE_OUT_PLANAR) != 0;
    const int64_t oplane = (int64_t)c.Ho * c.Wo;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        const int oy = y0 + wave * R + nb / 2, ox = x0 + 16 * (nb % 2) + l15;
        if (oy >= c.Ho || ox >= c.Wo) continue;
        const int64_t pix = (int64_t)oy * c.Wo + ox;
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) {
            const int cb = m0 + 16 * mb + 4 * kq;
            if (cb >= c.Co) continue;
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                v[r] = acc[mb][nb][r];
                if (d.a && cb + r < c.Co) {
                    const float av = d.a[((int64_t)n * oplane + pix) * c.Co + cb + r];
                    const float k0 = d.c0 ? d.c0[cb + r] : 0.f, k1 = d.c1 ? d.c1[cb + r] : 0.f;
                    v[r] = __builtin_fmaf(k1, av, v[r] + k0) * (av > 0.f ? 1.f : c.slope);
                }
            }
            if (planar) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (cb + r < c.Co) c.out[((int64_t)n * c.Co + cb + r) * oplane + pix] = v[r];
                continue;
            }
            float* dst = c.out + ((int64_t)n * oplane + pix) * c.Co + cb;
            if ((c.Co & 3) == 0) *(rm_f32x4*)dst = rm_f32x4{v[0], v[1], v[2], v[3]};
            else
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (cb + r < c.Co) dst[r] = v[r];
        }
    }
}

extern "C" int p3d_rmline_conv_dgrad_f32(const float* g, int N, int Hg, int Wg, int Co, const float* wk, int Ci, const float* a, const float* c0,
                                         const float* c1, float slope, int flags, float* out, void* stream) {
    if (!g || !wk || !out || N <= 0 || Hg <= 0 || Wg <= 0 || Ci <= 0 || Co <= 0) return P3D_E_ARG;
    if ((c0 != nullptr) != (c1 != nullptr) || (c0 && !a)) return P3D_E_ARG;
    if (a && (!isfinite(slope) || slope <= 0.f)) return P3D_E_ARG;
    if (flags & ~P3D_RMLINE_OUT_PLANAR) return P3D_E_RANGE;
    const bool planar = (flags & P3D_RMLINE_OUT_PLANAR) != 0;
    if (rm_misaligned(g, Co) || rm_misaligned(a, Ci) || (!planar && rm_misaligned(out, Ci))) return P3D_E_ARG;
    if (N > 65535 || Hg > 32768 || Wg > 32768) return P3D_E_RANGE;
    RmPlan p;
    const int rc = rm_conv_plan(Co, Ci, 0, &p);  // the GEMM's k is g's channels, its rows the layer's input channels
    if (rc) return rc;
    if ((int64_t)N * (Hg + 2) * (Wg + 2) >= ((int64_t)1 << 31) / P3D_RMLINE_MAX_C) return P3D_E_RANGE;
    RmDgrad d;
    RmConv& c = d.c;
    c.x = g, c.image = c.mask = c.hull = c.bias = nullptr, c.wk = wk, c.out = out;
    c.Hin = Hg, c.Win = Wg, c.Ho = Hg + 2, c.Wo = Wg + 2, c.pad = 0, c.Ci = Co, c.Co = Ci, c.act = 0, c.flags = flags, c.Hi = c.Wi = 0;
    c.ci4 = p.ci4, c.cip = p.cip, c.tiles_x = (c.Wo + RM_TW - 1) / RM_TW, c.slope = slope;
    d.a = a, d.c0 = c0, d.c1 = c1;
    static const void* const kernels[4] = {(const void*)k_rm_dgrad<1, 1>, (const void*)k_rm_dgrad<1, 2>, (const void*)k_rm_dgrad<2, 1>,
                                           (const void*)k_rm_dgrad<2, 2>};
    static bool raised[4][RM_MAX_DEVICES];
    const int which = (p.cot == 32 ? 2 : 0) + (p.rows == 8 ? 1 : 0);
    const int rl = rm_raise_lds(kernels[which], p.lds, raised[which]);
    if (rl) return rl;
    const dim3 grid((unsigned)(c.tiles_x * ((c.Ho + p.rows - 1) / p.rows)), (unsigned)p.cblocks, (unsigned)N);
    void* args[] = {&d};
    return (int)hipLaunchKernel(kernels[which], grid, dim3(RM_WG), args, p.lds, (hipStream_t)stream);
}

// ---- the weight / bias gradient ---------------------------------------------------------------------------------------------------------
struct RmWgrad {
    RmConv c;  // the input side, as the forward takes it (Ho, Wo: dz's map)
    const float* dz;
    float* ws;
    int N, slices, ci16, co16, nci, nco, tiles_y;
};

// v_mfma_f32_16x16x4_f32 with the INPUT as A (A[ci = l & 15][k = l >> 4]: four consecutive pixels of a tile row) and dz as B
// (B[k = l >> 4][co = l & 15]): D rows 4 (l >> 4) + r are input channels, its column l & 15 an output channel.  A wave owns whole
// (ci block, co block) pairs — nine taps' accumulators — for the slice's whole run of patches.  The bias gradient is a plain sum of dz
// whose terms cancel (a few units of 2^-24 of sum|dz| are a visible fraction of it), so it is taken on the vector ALU with a two-sum:
// lane (co = tid & 63, part = tid >> 6) adds the dz tile's rows part, part + 4, ... as a (sum, correction) pair.
// s + c <- s + c + x exactly, the rounding error of s + x kept in c
__device__ __forceinline__ void rm_two_sum(float& s, float& c, float x) {
    const float t = s + x, bb = t - s, e = (s - (t - bb)) + (x - bb);
    s = t;
    c = c + e;
}

template <int SETS>
__global__ __launch_bounds__(RM_WG) void k_rm_wgrad(RmWgrad w) {
    const RmConv& c = w.c;
    constexpr int PH = RM_WG_ROWS + 2;
    extern __shared__ __attribute__((aligned(16))) float rm_lds[];
    float* Xs = rm_lds;                         // [PH][RM_PW][ci16]
    float* Zs = rm_lds + PH * RM_PW * w.ci16;   // [RM_WG_ROWS][RM_TW][co16]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, kq = lane >> 4, pairs = w.nci * w.nco;
    int lo, hi;
    rm_wgrad_slice((int)blockIdx.x, w.slices, w.N, &lo, &hi);
    rm_f32x4 acc[SETS][9];
    float bs = 0.f, bc = 0.f;
    const int bco = tid & 63;
#pragma unroll
    for (int s = 0; s < SETS; ++s)
#pragma unroll
        for (int t = 0; t < 9; ++t) acc[s][t] = rm_f32x4{0.f, 0.f, 0.f, 0.f};
    const int nvz = w.co16 / 4;
    const bool vecz = (c.Co & 3) == 0;
    for (int n = lo; n < hi; ++n)
        for (int tyi = 0; tyi < w.tiles_y; ++tyi)
            for (int txi = 0; txi < c.tiles_x; ++txi) {
                const int y0 = tyi * RM_WG_ROWS, x0 = txi * RM_TW;
                __syncthreads();  // the tile before this one has been read
                if (c.flags & P3D_RMLINE_IN_STACK) rm_stage_stack(c, n, y0, x0, PH, Xs, w.ci16, w.ci16);
                else rm_stage_cl(c, n, y0, x0, 0, PH, Xs, w.ci16, w.ci16);
                for (int i = tid; i < RM_WG_ROWS * RM_TW * nvz; i += RM_WG) {
                    const int v = i % nvz, pix = i / nvz, oy = y0 + pix / RM_TW, ox = x0 + pix % RM_TW;
                    const bool in = oy < c.Ho && ox < c.Wo && 4 * v < c.Co;
                    const int64_t at = in ? (((int64_t)n * c.Ho + oy) * c.Wo + ox) * c.Co + 4 * v : 0;
                    rm_f32x4 r;
                    if (vecz) r = *(const rm_f32x4*)(w.dz + at);
                    else
#pragma unroll
                        for (int e = 0; e < 4; ++e) r[e] = w.dz[in && 4 * v + e < c.Co ? at + e : 0];
#pragma unroll
                    for (int e = 0; e < 4; ++e) Zs[pix * w.co16 + 4 * v + e] = in && 4 * v + e < c.Co ? r[e] : 0.f;
                }
                __syncthreads();
                const int rows = c.Ho - y0 < RM_WG_ROWS ? c.Ho - y0 : RM_WG_ROWS;
                if (bco < w.co16)
                    for (int py = wave; py < rows; py += 4)
                        for (int px = 0; px < RM_TW; ++px) rm_two_sum(bs, bc, Zs[(py * RM_TW + px) * w.co16 + bco]);
#pragma unroll
                for (int s = 0; s < SETS; ++s) {
                    const int pair = wave + 4 * s;
                    if (pair >= pairs) continue;
                    const int cib = pair / w.nco, cob = pair % w.nco;
                    const float* zb = Zs + cob * 16 + l15;
                    const float* xb = Xs + cib * 16 + l15;
                    for (int py = 0; py < rows; ++py) {  // a tile row: one chain from 0, then added to the slice's running sums
                        rm_f32x4 row[9];
#pragma unroll
                        for (int t = 0; t < 9; ++t) row[t] = rm_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
                        for (int step = 0; step < RM_TW / 4; ++step) {
                            const int px = 4 * step + kq;
                            const float b = zb[(py * RM_TW + px) * w.co16];
                            const float* xp = xb + (py * RM_PW + px) * w.ci16;
                            float a[9];
#pragma unroll
                            for (int t = 0; t < 9; ++t) a[t] = xp[((t / 3) * RM_PW + t % 3) * w.ci16];
#pragma unroll
                            for (int t = 0; t < 9; ++t) row[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t], b, row[t], 0, 0, 0);
                        }
#pragma unroll
                        for (int t = 0; t < 9; ++t)
#pragma unroll
                            for (int r = 0; r < 4; ++r) acc[s][t][r] = acc[s][t][r] + row[t][r];
                    }
                }
            }
    float* o = w.ws + (int64_t)blockIdx.x * (9 * (int64_t)c.Ci * c.Co + 2 * c.Co);
#pragma unroll
    for (int s = 0; s < SETS; ++s) {
        const int pair = wave + 4 * s;
        if (pair >= pairs) continue;
        const int cib = pair / w.nco, cob = pair % w.nco, co = cob * 16 + l15;
        if (co >= c.Co) continue;
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ci = cib * 16 + 4 * kq + r;
                if (ci < c.Ci) o[((int64_t)t * c.Ci + ci) * c.Co + co] = acc[s][t][r];
            }
    }
    // the bias: the four parts' (sum, correction) pairs through LDS, merged in part order
    __syncthreads();
    Zs[(2 * wave) * 64 + bco] = bs, Zs[(2 * wave + 1) * 64 + bco] = bc;
    __syncthreads();
    if (wave == 0 && bco < c.Co) {
        for (int q = 1; q < 4; ++q) {
            rm_two_sum(bs, bc, Zs[(2 * q) * 64 + bco]);
            bc = bc + Zs[(2 * q + 1) * 64 + bco];
        }
        o[9 * (int64_t)c.Ci * c.Co + bco] = bs, o[9 * (int64_t)c.Ci * c.Co + c.Co + bco] = bc;
    }
}

// out[i] = the slices' partials added in slice order from 0 (the bias: their (sum, correction) pairs by two-sum, rounded once at the
// end); the weight part optionally re-laid as [Co][Ci][3][3]
__global__ __launch_bounds__(RM_WG) void k_rm_wgrad_sum(const float* ws, int slices, int Ci, int Co, int oihw, float* dw, float* dbias) {
    const int nw = 9 * Ci * Co, total = nw + 2 * Co;
    const int i = blockIdx.x * RM_WG + threadIdx.x;
    if (i >= nw + Co) return;
    if (i >= nw) {
        float bs = 0.f, bc = 0.f;
        for (int s = 0; s < slices; ++s) {
            rm_two_sum(bs, bc, ws[(int64_t)s * total + i]);
            bc = bc + ws[(int64_t)s * total + i + Co];
        }
        dbias[i - nw] = bs + bc;
        return;
    }
    float acc = 0.f;
    for (int s = 0; s < slices; ++s) acc += ws[(int64_t)s * total + i];
    const int co = i % Co, ci = (i / Co) % Ci, t = i / (Co * Ci);
    dw[oihw ? (co * Ci + ci) * 9 + t : i] = acc;
}

extern "C" int p3d_rmline_wgrad_plan(int N, int Ci, int Co, int force_slices, int64_t* out4) {
    RmWgradPlan p;
    const int rc = rm_wgrad_plan(N, Ci, Co, force_slices, &p);
    if (rc) return rc;
    if (out4) out4[0] = p.slices, out4[1] = p.sets, out4[2] = (int64_t)p.lds, out4[3] = p.ws_floats;
    return p.slices;
}

extern "C" int p3d_rmline_conv_wgrad_f32(const float* x, const float* image, const float* mask, const float* hull, int N, int Hin, int Win,
                                         int pad, int Ci, const float* dz, int Co, int flags, int force_slices, float* dw, float* dbias,
                                         float* ws, int64_t ws_floats, void* stream) {
    if (!dz || !dw || !dbias || !ws || N <= 0 || Hin <= 0 || Win <= 0 || Ci <= 0 || Co <= 0) return P3D_E_ARG;
    const bool stack = (flags & P3D_RMLINE_IN_STACK) != 0;
    if (stack ? !image : !x) return P3D_E_ARG;
    if (flags & ~(P3D_RMLINE_IN_STACK | P3D_RMLINE_IN_NO_MASK | P3D_RMLINE_OUT_OIHW)) return P3D_E_RANGE;
    if ((!stack && rm_misaligned(x, Ci)) || rm_misaligned(dz, Co)) return P3D_E_ARG;
    if (pad < 0 || pad > 4096 || Hin < 3 || Win < 3 || Hin > 32768 || Win > 32768) return P3D_E_RANGE;
    RmWgradPlan p;
    const int rc = rm_wgrad_plan(N, Ci, Co, force_slices, &p);
    if (rc) return rc;
    if (stack) {
        if (Hin - 2 * pad < 1 || Win - 2 * pad < 1 || Ci != 3 + (hull ? 1 : 0)) return P3D_E_RANGE;
    } else if (pad != 0) {
        return P3D_E_RANGE;
    }
    if ((int64_t)N * Hin * Win >= ((int64_t)1 << 31) / P3D_RMLINE_MAX_C) return P3D_E_RANGE;
    if (ws_floats < p.ws_floats) return P3D_E_WORKSPACE;
    RmWgrad w;
    RmConv& c = w.c;
    c.x = x, c.image = image, c.mask = mask, c.hull = stack ? hull : nullptr, c.wk = c.bias = nullptr, c.out = nullptr;
    c.Hin = Hin, c.Win = Win, c.Ho = Hin - 2, c.Wo = Win - 2, c.pad = pad, c.Ci = Ci, c.Co = Co, c.act = 0, c.flags = flags;
    c.Hi = Hin - 2 * pad, c.Wi = Win - 2 * pad, c.ci4 = c.cip = 0, c.tiles_x = (c.Wo + RM_TW - 1) / RM_TW, c.slope = 0.f;
    w.dz = dz, w.ws = ws, w.N = N, w.slices = p.slices, w.ci16 = p.ci16, w.co16 = p.co16, w.nci = p.nci, w.nco = p.nco;
    w.tiles_y = (c.Ho + RM_WG_ROWS - 1) / RM_WG_ROWS;
    static const void* const kernels[2] = {(const void*)k_rm_wgrad<1>, (const void*)k_rm_wgrad<4>};
    static bool raised[2][RM_MAX_DEVICES];
    const int which = p.sets == 1 ? 0 : 1;
    const int rl = rm_raise_lds(kernels[which], p.lds, raised[which]);
    if (rl) return rl;
    void* args[] = {&w};
    const int r1 = (int)hipLaunchKernel(kernels[which], dim3((unsigned)p.slices), dim3(RM_WG), args, p.lds, (hipStream_t)stream);
    if (r1) return r1;
    const int total = 9 * Ci * Co + Co;
    hipLaunchKernelGGL(k_rm_wgrad_sum, dim3((unsigned)((total + RM_WG - 1) / RM_WG)), dim3(RM_WG), 0, (hipStream_t)stream, (const float*)ws,
                       p.slices, Ci, Co, (flags & P3D_RMLINE_OUT_OIHW) ? 1 : 0, dw, dbias);
    return (int)hipGetLastError();
}

// ---- the batch norm's backward coefficients ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RM_WG) void k_rm_bn_coef(const float* dwk_f, const float* db_f, const float* w, const float* gamma, const float* beta,
                                                      const float* mean, const float* var, float eps, float Kf, int Ci, int Co, float* dgamma, float* dbeta, float* dw,
                                                      float* c0, float* c1) {
    __shared__ float s[P3D_RMLINE_MAX_C], sh[P3D_RMLINE_MAX_C];
    const int tid = threadIdx.x;
    if (tid < Ci) {
        const int ci = tid;
        float ds = 0.f, dsc = 0.f, dt = 0.f, dtc = 0.f;
        for (int t = 0; t < 9; ++t)
            for (int co = 0; co < Co; ++co) {
                const float wv = w[((int64_t)co * Ci + ci) * 9 + t];
                rm_dot2(dwk_f[((int64_t)t * Ci + ci) * Co + co], wv, ds, dsc);
                rm_dot2(db_f[co], wv, dt, dtc);
            }
        const float r = 1.f / sqrtf(var[ci] + eps), g = gamma[ci], m = mean[ci], sc = g * r;
        s[ci] = sc, sh[ci] = beta[ci] - m * sc;
        const float cen = (__builtin_fmaf(-m, dt, ds) + dsc) - m * dtc;  // ds - mean dt from the sums' (value, correction) pairs
        ds = ds + dsc, dt = dt + dtc;
        if (dgamma) dgamma[ci] = cen * r;
        if (dbeta) dbeta[ci] = dt;
        const float c1h = ((cen * g) * (-0.5f * r * r * r)) / Kf;
        c0[ci] = -(sc * dt) / Kf - 2.f * m * c1h;
        c1[ci] = 2.f * c1h;
    }
    __syncthreads();
    if (dw)
        for (int i = tid; i < 9 * Ci * Co; i += RM_WG) {  // i walks dw [co][ci][t]
            const int t = i % 9, ci = (i / 9) % Ci, co = i / (9 * Ci);
            dw[i] = dwk_f[((int64_t)t * Ci + ci) * Co + co] * s[ci] + db_f[co] * sh[ci];
        }
}

extern "C" int p3d_rmline_bn_coef_f32(const float* dwk_f, const float* db_f, const float* w, const float* gamma, const float* beta,
                                      const float* mean, const float* var, float eps, int64_t K, int Ci, int Co, float* dgamma, float* dbeta, float* dw, float* c0,
                                      float* c1, void* stream) {
    if (!dwk_f || !db_f || !w || !gamma || !beta || !mean || !var || !c0 || !c1 || Ci <= 0 || Co <= 0 || K <= 1) return P3D_E_ARG;
    if (!isfinite(eps) || eps < 0.f) return P3D_E_ARG;
    if (Ci > P3D_RMLINE_MAX_C || Co > P3D_RMLINE_MAX_C) return P3D_E_RANGE;
    hipLaunchKernelGGL(k_rm_bn_coef, dim3(1), dim3(RM_WG), 0, (hipStream_t)stream, dwk_f, db_f, w, gamma, beta, mean, var, eps, (float)K, Ci, Co, dgamma,
                       dbeta, dw, c0, c1);
    return (int)hipGetLastError();
}

// ---- the head -------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RM_WG) void k_rm_head(const float* t, const float* image, const float* mask, const float* hull, int H, int W, int crop,
                                                   float* img, float* loss_l1, float* crop_img, float* crop_hull) {
    __shared__ float red[RM_WG];
    const int tid = threadIdx.x, n = blockIdx.x;
    const int plane = H * W, total = 3 * plane, Hc = H - 2 * crop, Wc = W - 2 * crop;
    float acc = 0.f;
    for (int i = tid; i < total; i += RM_WG) {
        const int ch = i / plane, pix = i % plane, y = pix / W, x = pix % W;
        const int64_t at = (int64_t)n * total + i;
        const float a = image[at], b = t[at], w = mask[(int64_t)n * plane + pix], diff = b - a;
        const float res = w < 0.5f ? a + w * diff : b - diff * (1.f - w);
        img[at] = res;
        acc += fabsf(res - a);
        if (crop_img && y >= crop && y < crop + Hc && x >= crop && x < crop + Wc)
            crop_img[(((int64_t)n * 3 + ch) * Hc + (y - crop)) * Wc + (x - crop)] = res;
    }
    if (crop_hull)
        for (int i = tid; i < Hc * Wc; i += RM_WG)
            crop_hull[(int64_t)n * Hc * Wc + i] = hull[(int64_t)n * plane + (i / Wc + crop) * W + (i % Wc + crop)];
    red[tid] = acc;
    __syncthreads();
    for (int s = RM_WG / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] = red[tid] + red[tid + s];
        __syncthreads();
    }
    if (tid == 0) loss_l1[n] = red[0] / (float)total;
}

extern "C" int p3d_rmline_head_f32(const float* t, const float* image, const float* mask, const float* hull, int N, int H, int W, int crop,
                                   float* img, float* loss_l1, float* crop_img, float* crop_hull, void* stream) {
    if (!t || !image || !mask || !img || !loss_l1 || N <= 0 || H <= 0 || W <= 0) return P3D_E_ARG;
    if (crop_hull && (!hull || !crop_img)) return P3D_E_ARG;
    if (crop < 0 || H - 2 * crop < 1 || W - 2 * crop < 1 || H > 4096 || W > 4096 || (int64_t)N * H * W >= ((int64_t)1 << 31) / 4) return P3D_E_RANGE;
    hipLaunchKernelGGL(k_rm_head, dim3((unsigned)N), dim3(RM_WG), 0, (hipStream_t)stream, t, image, mask, hull, H, W, crop, img, loss_l1, crop_img,
                       crop_hull);
    return (int)hipGetLastError();
}

struct RmStrides {
    int64_t n, c, y, x;
};

__global__ __launch_bounds__(RM_WG) void k_rm_head_grad(const float* t, const float* img, const float* image, const float* mask, const float* g_l1,
                                                        const float* d, RmStrides ds, int N, int H, int W, int crop, float* out) {
    const int64_t i = (int64_t)blockIdx.x * RM_WG + threadIdx.x;  // i walks out [n][y][x][c]
    const int plane = H * W;
    if (i >= (int64_t)N * plane * 3) return;
    const int ch = (int)(i % 3), pix = (int)((i / 3) % plane), n = (int)(i / (3 * (int64_t)plane)), y = pix / W, x = pix % W;
    const int64_t at = ((int64_t)n * 3 + ch) * plane + pix;
    float v = 0.f;
    if (g_l1) {
        const float e = img[at] - image[at];
        const float sg = e > 0.f ? 1.f : (e < 0.f ? -1.f : 0.f);
        v = g_l1[n] * sg / (float)(3 * plane);
    }
    const int Hc = H - 2 * crop, Wc = W - 2 * crop;
    if (d && y >= crop && y < crop + Hc && x >= crop && x < crop + Wc) v = v + d[n * ds.n + ch * ds.c + (y - crop) * ds.y + (x - crop) * ds.x];
    if (mask) v = mask[(int64_t)n * plane + pix] * v;
    if (t) {
        const float tv = t[at];
        v = __builtin_fmaf(-tv, tv, 1.f) * v;
    }
    out[i] = v;
}

extern "C" int p3d_rmline_head_grad_f32(const float* t, const float* img, const float* image, const float* mask, const float* g_l1, const float* d,
                                        const int64_t* ds4, int N, int H, int W, int crop, float* out, void* stream) {
    if (!out || N <= 0 || H <= 0 || W <= 0 || (g_l1 && (!img || !image)) || (d && !ds4)) return P3D_E_ARG;
    if (crop < 0 || H - 2 * crop < 1 || W - 2 * crop < 1 || H > 4096 || W > 4096 || (int64_t)N * H * W >= ((int64_t)1 << 31) / 4) return P3D_E_RANGE;
    RmStrides ds = {0, 0, 0, 0};
    if (d) ds = RmStrides{ds4[0], ds4[1], ds4[2], ds4[3]};
    const int64_t total = (int64_t)N * H * W * 3;
    hipLaunchKernelGGL(k_rm_head_grad, dim3((unsigned)((total + RM_WG - 1) / RM_WG)), dim3(RM_WG), 0, (hipStream_t)stream, t, img, image, mask, g_l1,
                       d, ds, N, H, W, crop, out);
    return (int)hipGetLastError();
}
