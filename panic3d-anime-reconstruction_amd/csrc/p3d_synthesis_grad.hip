// p3d_synthesis_grad.hip — backward of the synthesis network's layers (include/p3d_synthesis_grad.h).
//
//   k_sg_bias_act_bwd   one workgroup per (sample, channel) row: the bias_act mask from the output y, g_z * d written, the row sum
//                       of g_z (bias gradient per sample) reduced in a fixed tree;
//   k_sg_noise_bwd      sixteen lanes per pixel: the channel sum of g_z (noise gradient), in a fixed order;
//   k_sg_dgrad          the data gradient as an implicit GEMM on v_mfma_f32_16x16x4_f32: 64 output channels x 64 output pixels per
//                       workgroup, K = (tap, input channel) in 16-wide chunks staged through LDS, gathered with zero padding and a
//                       stride (1: the plain layer's transposed convolution with flipped weights; 2: the up-sampling layer's
//                       stride-2 correlation after the FIR adjoint);
//   k_sg_mod_bwd        one workgroup per (sample, channel) row: g_s = sum x * g, then g *= s;
//   k_sg_wgrad          the weight gradient as a GEMM [O] x [I] per tap whose K is the pixels of one sample, split into slabs
//                       (one partial [taps][O][I] slab per (sample, slab));
//   k_sg_reduce         slabs summed in slab order (per sample), then samples in sample order;
//   k_sg_gd             per (sample, output channel): sum over taps and input channels of w * dw_n, / d.
// Every sum runs in a fixed order: the results are bitwise reproducible for the same sizes.
#include <hip/hip_runtime.h>

#include "../../include/p3d_synthesis_grad.h"

#include "p3d_corr_tile.hpp"  // SG_* sizes, sg_mma_chunk, sg_corr_tile: shared with the forward convolution of p3d_discriminator.hip

static inline size_t sg_align(size_t b) { return (b + 255) & ~(size_t)255; }

// ---- bias_act backward (the rule itself, sg_gz, is in p3d_corr_tile.hpp: the R1 tangent layer of p3d_r1.hip applies it in its store) ----
__global__ __launch_bounds__(SG_WG) void k_sg_bias_act_bwd(const float* __restrict__ y, const float* g_y, int C, int64_t HW, int act,
                                                           float alpha, float gain, float clamp, const float* __restrict__ dscale,
                                                           float* g_out, float* __restrict__ g_bias_nc) {
    __shared__ float red[SG_WG];
    const int64_t row = blockIdx.x;
    const float ds = dscale ? dscale[row] : 1.f;
    const float* yr = y + row * HW;
    const float* gr = g_y + row * HW;
    float* outr = g_out + row * HW;
    float sum = 0.f;
    for (int64_t p = threadIdx.x; p < HW; p += SG_WG) {
        const float g = sg_gz(yr[p], gr[p], act, alpha, gain, clamp);
        sum += g;
        outr[p] = g * ds;
    }
    const float tot = sg_block_sum(sum, red);
    if (g_bias_nc && threadIdx.x == 0) g_bias_nc[row] = tot;
}

// 16 pixels x 16 channel slices per workgroup: slice j sums channels j, j + 16, ... of its pixel in order, then the 16 slice sums
// are added in slice order (fixed: reproducible).  Sixteen lanes per pixel keep the 4^2 .. 32^2 maps from running a handful of lanes
// through a 512-long dependent loop.
#define SG_NPIX 16
#define SG_NSL (SG_WG / SG_NPIX)
__global__ __launch_bounds__(SG_WG) void k_sg_noise_bwd(const float* __restrict__ y, const float* __restrict__ g_y, int N, int C,
                                                        int64_t HW, int act, float alpha, float gain, float clamp,
                                                        float* __restrict__ g_noise) {
    __shared__ float part[SG_NSL][SG_NPIX + 1];
    const int px = threadIdx.x % SG_NPIX, sl = threadIdx.x / SG_NPIX;
    const int64_t e = (int64_t)blockIdx.x * SG_NPIX + px;
    const bool in = e < (int64_t)N * HW;
    float sum = 0.f;
    if (in) {
        const int64_t n = e / HW, p = e % HW;
        for (int c = sl; c < C; c += SG_NSL) {
            const int64_t o = (n * C + c) * HW + p;
            sum += sg_gz(y[o], g_y[o], act, alpha, gain, clamp);
        }
    }
    part[sl][px] = sum;
    __syncthreads();
    if (sl == 0 && in) {
        float t = 0.f;
        for (int j = 0; j < SG_NSL; ++j) t += part[j][px];
        g_noise[e] = t;
    }
}

// ---- data gradient ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SG_WG) void k_sg_dgrad(SgCorr a, float* __restrict__ out) {
    __shared__ float As[SG_KC][SG_LD];
    __shared__ float Bs[SG_KC][SG_LD];
    const int64_t P = (int64_t)a.Ho * a.Wo;
    sg_corr_tile(a, As, Bs, [&](int64_t n, int co, int64_t pc, float v) { out[(n * a.Co + co) * P + pc] = v; });
}

// ---- modulation backward ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SG_WG) void k_sg_mod_bwd(const float* __restrict__ x, const float* __restrict__ s, int64_t HW,
                                                      float* __restrict__ g, float* __restrict__ g_s) {
    __shared__ float red[SG_WG];
    const int64_t row = blockIdx.x;
    const float sv = s[row];
    const float* xr = x + row * HW;
    float* gr = g + row * HW;
    float sum = 0.f;
    for (int64_t p = threadIdx.x; p < HW; p += SG_WG) {
        const float gv = gr[p];
        sum += xr[p] * gv;
        gr[p] = gv * sv;
    }
    const float tot = sg_block_sum(sum, red);
    if (threadIdx.x == 0) g_s[row] = tot;
}

// ---- weight gradient --------------------------------------------------------------------------------------------------------
struct SgWgrad {
    const float* g;
    int Hg, Wg, sg, ag, pg;
    const float* x;
    const float* s;
    int Hx, Wx, sx, ax, px0;
    int O, I, taps, Hd, Wd, slabs, slabK;
    float* part;
};

__global__ __launch_bounds__(SG_WG) void k_sg_wgrad(SgWgrad a) {
    __shared__ float As[SG_KC][SG_LD];
    __shared__ float Bs[SG_KC][SG_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
    const int tilesI = (a.I + SG_TILE - 1) / SG_TILE;
    const int o0 = (blockIdx.x / tilesI) * SG_TILE, i0 = (blockIdx.x % tilesI) * SG_TILE;
    const int t = blockIdx.y;
    const int ty = a.taps == 9 ? t / 3 : 0, tx = a.taps == 9 ? t % 3 : 0;
    const int64_t n = blockIdx.z / a.slabs;
    const int j = blockIdx.z % a.slabs;
    const int64_t P = (int64_t)a.Hd * a.Wd;
    const int64_t pbeg = (int64_t)j * a.slabK;
    const int64_t pend = pbeg + a.slabK < P ? pbeg + a.slabK : P;
    const int kk = tid & 15, m0 = tid >> 4;  // this lane stages K row kk of columns m0, m0 + 16, m0 + 32, m0 + 48
    const float* gn = a.g + n * a.O * (int64_t)a.Hg * a.Wg;
    const float* xn = a.x + n * a.I * (int64_t)a.Hx * a.Wx;
    float sv[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int i = i0 + m0 + 16 * q;
        sv[q] = (a.s && i < a.I) ? a.s[n * a.I + i] : 1.f;
    }
    sg_f32x4 acc[2][2];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v) acc[u][v] = sg_f32x4{0.f, 0.f, 0.f, 0.f};
    for (int64_t pc0 = pbeg; pc0 < pend; pc0 += SG_KC) {
        const int64_t p = pc0 + kk;
        const bool valid = p < pend;
        const int py = valid ? (int)(p / a.Wd) : 0, px = valid ? (int)(p % a.Wd) : 0;
        const int gy = a.sg * py + a.ag * ty - a.pg, gx = a.sg * px + a.ag * tx - a.pg;
        const int xy = a.sx * py + a.ax * ty - a.px0, xx = a.sx * px + a.ax * tx - a.px0;
        const bool gin = valid && gy >= 0 && gy < a.Hg && gx >= 0 && gx < a.Wg;
        const bool xin = valid && xy >= 0 && xy < a.Hx && xx >= 0 && xx < a.Wx;
        const int64_t goff = gin ? (int64_t)gy * a.Wg + gx : 0;
        const int64_t xoff = xin ? (int64_t)xy * a.Wx + xx : 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int m = m0 + 16 * q;
            const int o = o0 + m, i = i0 + m;
            As[kk][m] = (gin && o < a.O) ? gn[(int64_t)o * a.Hg * a.Wg + goff] : 0.f;
            Bs[kk][m] = (xin && i < a.I) ? xn[(int64_t)i * a.Hx * a.Wx + xoff] * sv[q] : 0.f;
        }
        __syncthreads();
        sg_mma_chunk(As, Bs, acc, wm, wn, lane);
        __syncthreads();
    }
    float* slab = a.part + ((int64_t)blockIdx.z * a.taps + t) * a.O * a.I;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int o = o0 + wm + 16 * mi + 4 * (lane >> 4) + r;
                const int i = i0 + wn + 16 * ni + (lane & 15);
                if (o < a.O && i < a.I) slab[(int64_t)o * a.I + i] = acc[mi][ni][r];
            }
}

// out[grp][e] = sum over c < cnt, in order, of in[grp * cnt + c][e]
__global__ __launch_bounds__(SG_WG) void k_sg_reduce(const float* __restrict__ in, int64_t E, int cnt, float* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * SG_WG + threadIdx.x;
    if (e >= E) return;
    const int64_t grp = blockIdx.y;
    float sum = 0.f;
    for (int c = 0; c < cnt; ++c) sum += in[(grp * cnt + c) * E + e];
    out[grp * E + e] = sum;
}

__global__ __launch_bounds__(SG_WG) void k_sg_gd(const float* __restrict__ wk, const float* __restrict__ dwn, const float* __restrict__ dscale,
                                                 int O, int I, int taps, float* __restrict__ g_d) {
    __shared__ float red[SG_WG];
    const int64_t row = blockIdx.x;  // n * O + o
    const int64_t n = row / O, o = row % O;
    float sum = 0.f;
    for (int t = 0; t < taps; ++t) {
        const float* w = wk + ((int64_t)t * O + o) * I;
        const float* d = dwn + ((n * taps + t) * O + o) * I;
        for (int i = threadIdx.x; i < I; i += SG_WG) sum += w[i] * d[i];
    }
    const float tot = sg_block_sum(sum, red);
    if (threadIdx.x == 0) g_d[row] = tot / dscale[row];
}

// ---- backward of a ToRGB layer finished by p3d_torgb_combine_f32 ---------------------------------------------------------------
// One thread per image value: the pre-clamp value rebuilt exactly as k_torgb_combine builds it (shares added in tile order, then the
// bias), and g_y = g_img where the clamp let the value through, 0 elsewhere.
__global__ __launch_bounds__(SG_WG) void k_sg_torgb_combine_bwd(const float* __restrict__ part, int tiles, int64_t slice, int R, int64_t HW,
                                                                const float* __restrict__ bias, float clamp, const float* __restrict__ g_img,
                                                                float* __restrict__ g_y) {
    const int64_t idx = (int64_t)blockIdx.x * SG_WG + threadIdx.x;
    if (idx >= slice) return;
    float v = part[idx];
    for (int t = 1; t < tiles; ++t) v += part[(int64_t)t * slice + idx];
    if (bias) v = v + bias[(idx / HW) % R];
    const bool keep = clamp < 0.f || fabsf(v) < clamp;
    g_y[idx] = keep ? g_img[idx] : 0.f;
}

// g_bias[r]: one workgroup per channel; lane j sums the pixels j, j + SG_WG, ... of sample 0, then of sample 1, ..., then the lanes
// are added in the fixed tree of sg_block_sum.
__global__ __launch_bounds__(SG_WG) void k_sg_torgb_bias_bwd(const float* __restrict__ g_y, int N, int R, int64_t HW, float* __restrict__ g_bias) {
    __shared__ float red[SG_WG];
    const int r = blockIdx.x;
    float sum = 0.f;
    for (int n = 0; n < N; ++n) {
        const float* row = g_y + ((int64_t)n * R + r) * HW;
        for (int64_t p = threadIdx.x; p < HW; p += SG_WG) sum += row[p];
    }
    const float tot = sg_block_sum(sum, red);
    if (threadIdx.x == 0) g_bias[r] = tot;
}

// The adjoint of the skip connection's up-sampling (k_torgb_combine's four polyphase taps): each skip value collects the image
// gradient at the 16 positions its taps reached, g_skip[u][v] = sum over fy, fx < 4 of skipf[fy][fx] * g_img[2u + 2 - fy][2v + 2 - fx]
// (outside the image: 0), in (fy, fx) order.
__global__ __launch_bounds__(SG_WG) void k_sg_torgb_skip_bwd(const float* __restrict__ g_img, int64_t planes, int H, int W,
                                                             const float* __restrict__ skipf, float* __restrict__ g_skip) {
    const int H2 = H >> 1, W2 = W >> 1;
    const int64_t idx = (int64_t)blockIdx.x * SG_WG + threadIdx.x;
    if (idx >= planes * H2 * W2) return;
    const int64_t pl = idx / ((int64_t)H2 * W2);
    const int q = (int)(idx - pl * H2 * W2), u = q / W2, v = q - u * W2;
    const float* g = g_img + pl * H * W;
    float sum = 0.f;
#pragma unroll
    for (int fy = 0; fy < 4; ++fy) {
        const int Y = 2 * u + 2 - fy;
#pragma unroll
        for (int fx = 0; fx < 4; ++fx) {
            const int X = 2 * v + 2 - fx;
            const bool in = Y >= 0 && Y < H && X >= 0 && X < W;
            sum = __builtin_fmaf(in ? skipf[fy * 4 + fx] : 0.f, g[in ? (int64_t)Y * W + X : 0], sum);
        }
    }
    g_skip[idx] = sum;
}

// ---- entry points -----------------------------------------------------------------------------------------------------------
extern "C" int p3d_torgb_combine_backward_f32(const float* partial, int tiles, int N, int R, int H, int W, const float* bias, float clamp,
                                              const float* g_img, float* g_y, float* g_bias, const float* skip_fir, float* g_skip,
                                              void* stream) {
    if (!partial || !g_img || !g_y || (g_skip && !skip_fir)) return P3D_E_ARG;
    if (tiles <= 0 || N <= 0 || R <= 0 || H <= 0 || W <= 0) return P3D_E_ARG;
    if (g_skip && ((H | W) & 1)) return P3D_E_RANGE;
    const int64_t HW = (int64_t)H * W, slice = (int64_t)N * R * HW;
    if (slice * tiles >= ((int64_t)1 << 40) || (slice + SG_WG - 1) / SG_WG > SG_MAX_GRID || R > 65535) return P3D_E_RANGE;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_sg_torgb_combine_bwd, dim3((unsigned)((slice + SG_WG - 1) / SG_WG)), dim3(SG_WG), 0, st, partial, tiles, slice, R, HW,
                       bias, clamp, g_img, g_y);
    if (g_bias) hipLaunchKernelGGL(k_sg_torgb_bias_bwd, dim3((unsigned)R), dim3(SG_WG), 0, st, (const float*)g_y, N, R, HW, g_bias);
    if (g_skip) {
        const int64_t E = (int64_t)N * R * (H / 2) * (W / 2);
        hipLaunchKernelGGL(k_sg_torgb_skip_bwd, dim3((unsigned)((E + SG_WG - 1) / SG_WG)), dim3(SG_WG), 0, st, g_img, (int64_t)N * R, H, W,
                           skip_fir, g_skip);
    }
    return (int)hipGetLastError();
}

extern "C" int p3d_bias_act_backward_f32(const float* y, const float* g_y, int N, int C, int64_t HW, int act, float alpha, float gain,
                                         float clamp, const float* dscale, float* g_out, float* g_bias_nc, float* g_noise, void* stream) {
    if (!y || !g_y || !g_out) return P3D_E_ARG;
    if (N <= 0 || C <= 0 || HW <= 0) return P3D_E_ARG;
    if (act != 0 && act != 1) return P3D_E_RANGE;
    if ((int64_t)N * C > SG_MAX_GRID || ((int64_t)N * HW + SG_NPIX - 1) / SG_NPIX > SG_MAX_GRID) return P3D_E_RANGE;
    hipStream_t st = (hipStream_t)stream;
    if (g_noise)  // first: g_out may alias g_y
        hipLaunchKernelGGL(k_sg_noise_bwd, dim3((unsigned)(((int64_t)N * HW + SG_NPIX - 1) / SG_NPIX)), dim3(SG_WG), 0, st, y, g_y, N, C, HW,
                           act, alpha, gain, clamp, g_noise);
    hipLaunchKernelGGL(k_sg_bias_act_bwd, dim3((unsigned)((int64_t)N * C)), dim3(SG_WG), 0, st, y, g_y, C, HW, act, alpha, gain, clamp,
                       dscale, g_out, g_bias_nc);
    return (int)hipGetLastError();
}

extern "C" int p3d_conv_dgrad_f32(const float* g, int N, int Ci, int Hi, int Wi, const float* wk, int taps, int Co, int Ho, int Wo,
                                  int stride, int pad, float* out, void* stream) {
    if (!g || !wk || !out) return P3D_E_ARG;
    if (N <= 0 || Ci <= 0 || Hi <= 0 || Wi <= 0 || Co <= 0 || Ho <= 0 || Wo <= 0) return P3D_E_ARG;
    if ((taps != 1 && taps != 9) || (stride != 1 && stride != 2) || pad < 0 || pad > 2) return P3D_E_RANGE;
    dim3 grid;
    if (!sg_corr_grid(N, Co, Ho, Wo, &grid)) return P3D_E_RANGE;
    const SgCorr a = {g, wk, Ci, Hi, Wi, taps, Co, Ho, Wo, stride, pad};
    hipLaunchKernelGGL(k_sg_dgrad, grid, dim3(SG_WG), 0, (hipStream_t)stream, a, out);
    return (int)hipGetLastError();
}

extern "C" int p3d_mod_backward_f32(const float* x, const float* s, int N, int C, int64_t HW, float* g, float* g_s, void* stream) {
    if (!x || !s || !g || !g_s) return P3D_E_ARG;
    if (N <= 0 || C <= 0 || HW <= 0) return P3D_E_ARG;
    if ((int64_t)N * C > SG_MAX_GRID) return P3D_E_RANGE;
    hipLaunchKernelGGL(k_sg_mod_bwd, dim3((unsigned)((int64_t)N * C)), dim3(SG_WG), 0, (hipStream_t)stream, x, s, HW, g, g_s);
    return (int)hipGetLastError();
}

// Split of the K dimension (the pixels of one sample): enough (sample, slab) workgroups to fill the chip, slabs of >= 256 pixels.
struct SgSplit {
    int slabs, slabK;
    size_t part_bytes, dwn_bytes;
};

static SgSplit sg_split(int N, int O, int I, int taps, int Hd, int Wd) {
    SgSplit r;
    const int64_t P = (int64_t)Hd * Wd;
    const int64_t tiles = (int64_t)taps * ((O + SG_TILE - 1) / SG_TILE) * ((I + SG_TILE - 1) / SG_TILE);
    int64_t want = (2048 + tiles * N - 1) / (tiles * N);
    const int64_t most = (P + 255) / 256;
    if (want > most) want = most;
    if (want < 1) want = 1;
    int64_t K = (P + want - 1) / want;
    K = (K + SG_KC - 1) / SG_KC * SG_KC;
    r.slabK = (int)K;
    r.slabs = (int)((P + K - 1) / K);
    const size_t slab = (size_t)taps * O * I * sizeof(float);
    r.part_bytes = sg_align(slab * (size_t)N * r.slabs);
    r.dwn_bytes = sg_align(slab * (size_t)N);
    return r;
}

static bool sg_wgrad_sizes_ok(int N, int O, int I, int taps, int Hd, int Wd) {
    return N > 0 && O > 0 && I > 0 && Hd > 0 && Wd > 0 && (taps == 1 || taps == 9) && N <= 4096 && O <= 4096 && I <= 4096 &&
           (int64_t)Hd * Wd <= ((int64_t)1 << 26);
}

extern "C" size_t p3d_conv_wgrad_workspace_bytes(int N, int O, int I, int taps, int Hd, int Wd) {
    if (!sg_wgrad_sizes_ok(N, O, I, taps, Hd, Wd)) return 0;
    const SgSplit s = sg_split(N, O, I, taps, Hd, Wd);
    return s.part_bytes + s.dwn_bytes;
}

extern "C" int p3d_conv_wgrad_f32(const float* g, int Hg, int Wg, int sg, int ag, int pg, const float* x, const float* s, int Hx, int Wx,
                                  int sx, int ax, int px0, int N, int O, int I, int taps, int Hd, int Wd, float* dw, const float* wk,
                                  const float* dscale, float* g_d, void* workspace, size_t workspace_bytes, void* stream) {
    if (!g || !x || !dw || !workspace) return P3D_E_ARG;
    if (g_d && (!wk || !dscale)) return P3D_E_ARG;
    if (N <= 0 || O <= 0 || I <= 0 || Hd <= 0 || Wd <= 0 || Hg <= 0 || Wg <= 0 || Hx <= 0 || Wx <= 0) return P3D_E_ARG;
    if (!sg_wgrad_sizes_ok(N, O, I, taps, Hd, Wd) || sg < 1 || sg > 2 || sx < 1 || sx > 2 || ag < 0 || ag > 1 || ax < 0 || ax > 1 ||
        pg < 0 || pg > 2 || px0 < 0 || px0 > 2)
        return P3D_E_RANGE;
    if (((uintptr_t)workspace & 255) != 0) return P3D_E_ARG;
    const SgSplit sp = sg_split(N, O, I, taps, Hd, Wd);
    if (workspace_bytes < sp.part_bytes + sp.dwn_bytes) return P3D_E_WORKSPACE;
    if ((int64_t)N * sp.slabs > 65535) return P3D_E_RANGE;
    hipStream_t st = (hipStream_t)stream;
    float* part = (float*)workspace;
    float* dwn = (float*)((char*)workspace + sp.part_bytes);
    SgWgrad a;
    a.g = g; a.Hg = Hg; a.Wg = Wg; a.sg = sg; a.ag = ag; a.pg = pg;
    a.x = x; a.s = s; a.Hx = Hx; a.Wx = Wx; a.sx = sx; a.ax = ax; a.px0 = px0;
    a.O = O; a.I = I; a.taps = taps; a.Hd = Hd; a.Wd = Wd; a.slabs = sp.slabs; a.slabK = sp.slabK; a.part = part;
    const int tiles = ((O + SG_TILE - 1) / SG_TILE) * ((I + SG_TILE - 1) / SG_TILE);
    hipLaunchKernelGGL(k_sg_wgrad, dim3((unsigned)tiles, (unsigned)taps, (unsigned)(N * sp.slabs)), dim3(SG_WG), 0, st, a);
    const int64_t E = (int64_t)taps * O * I;
    const unsigned gx = (unsigned)((E + SG_WG - 1) / SG_WG);
    hipLaunchKernelGGL(k_sg_reduce, dim3(gx, (unsigned)N), dim3(SG_WG), 0, st, (const float*)part, E, sp.slabs, dwn);  // per sample
    hipLaunchKernelGGL(k_sg_reduce, dim3(gx, 1u), dim3(SG_WG), 0, st, (const float*)dwn, E, N, dw);                     // over samples
    if (g_d) hipLaunchKernelGGL(k_sg_gd, dim3((unsigned)((int64_t)N * O)), dim3(SG_WG), 0, st, wk, (const float*)dwn, dscale, O, I, taps, g_d);
    return (int)hipGetLastError();
}
