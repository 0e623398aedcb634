// p3d_corr_tile.hpp — the strided correlation's tile loop on v_mfma_f32_16x16x4_f32, defined once.
//
//   acc[co][p] = sum over t < taps (in order), ci < Ci (in order) of x[n][ci][stride*oy + ty - pad][stride*ox + tx - pad] * wk[t][ci][co]
//
// for one workgroup's 64 output channels x 64 output pixels (out-of-range positions read 0).  Instantiated by the data gradient of the
// synthesis layers (k_sg_dgrad, p3d_synthesis_grad.hip: a plain store) and by the discriminator's forward convolution (k_conv2d_act,
// p3d_discriminator.hip: bias, activation, gain, clamp and residual in the store).  Both kernels therefore take every sum in the same
// order; the matrix-core step sg_mma_chunk is also what the weight gradient's GEMM (k_sg_wgrad) runs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define SG_TILE 64           // GEMM tile (rows x columns) per workgroup
#define SG_KC 16             // K chunk staged through LDS
#define SG_LD (SG_TILE + 4)  // LDS row pitch in floats
#define SG_WG 256            // four waves, each a 32 x 32 quarter of the tile

typedef float sg_f32x4 __attribute__((ext_vector_type(4)));

// ---- the matrix-core step shared by the GEMMs ---------------------------------------------------------------------------------
// As[k][m], Bs[k][n]: one K chunk.  Wave quarter (wm, wn); 2 x 2 blocks of v_mfma_f32_16x16x4_f32 (A[l&15][k=l>>4],
// B[k=l>>4][l&15]; D col = l&15, row = 4*(l>>4) + r), four k steps per chunk in k order.
__device__ __forceinline__ void sg_mma_chunk(const float (*As)[SG_LD], const float (*Bs)[SG_LD], sg_f32x4 (&acc)[2][2], int wm, int wn,
                                             int lane) {
#pragma unroll
    for (int kk = 0; kk < SG_KC; kk += 4) {
        const int k = kk + (lane >> 4), r = lane & 15;
        const float a0 = As[k][wm + r], a1 = As[k][wm + 16 + r];
        const float b0 = Bs[k][wn + r], b1 = Bs[k][wn + 16 + r];
        acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
    }
}

__device__ __forceinline__ float sg_block_sum(float v, float* red) {
    // fixed-order tree over the workgroup's SG_WG lanes
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int s = SG_WG / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] = red[tid] + red[tid + s];
        __syncthreads();
    }
    return red[0];
}

// The bias_act backward's rule for one value, defined once: y is the layer's output before any residual, gy its cotangent.  Used by
// k_sg_bias_act_bwd / k_sg_noise_bwd (p3d_synthesis_grad.hip) and in the store of k_conv2d_mask (p3d_r1.hip).
__device__ __forceinline__ float sg_gz(float y, float gy, int act, float alpha, float gain, float clamp) {
    if (clamp >= 0.f && !(fabsf(y) < clamp)) return 0.f;
    float g = gy * gain;
    if (act == 1 && !(y > 0.f)) g = g * alpha;
    return g;
}

// x [N][Ci][Hi][Wi], wk [taps][Ci][Co] -> [N][Co][Ho][Wo]; blockIdx = (pixel tile, channel tile, sample)
struct SgCorr {
    const float* x;
    const float* wk;
    int Ci, Hi, Wi, taps, Co, Ho, Wo, stride, pad;
};

// The whole tile: K = (tap, input channel) in SG_KC-wide chunks staged through LDS, gathered with zero padding and a stride, then
// store(n, co, pixel, value) for every value of the tile that lies inside the output.
template <typename Store>
__device__ __forceinline__ void sg_corr_tile(const SgCorr& a, float (*As)[SG_LD], float (*Bs)[SG_LD], Store store) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
    const int64_t P = (int64_t)a.Ho * a.Wo;
    const int64_t p0 = (int64_t)blockIdx.x * SG_TILE;
    const int co0 = blockIdx.y * SG_TILE;
    const int64_t n = blockIdx.z;
    const int64_t plane = (int64_t)a.Hi * a.Wi;
    const float* gn = a.x + n * a.Ci * plane;
    const int col = tid & 63, kr = tid >> 6;  // this lane stages column `col` of rows kr, kr + 4, kr + 8, kr + 12
    const int64_t p = p0 + col;
    const bool pin = p < P;
    const int oy = pin ? (int)(p / a.Wo) : 0, ox = pin ? (int)(p % a.Wo) : 0;
    const bool co_in = co0 + col < a.Co;
    sg_f32x4 acc[2][2];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v) acc[u][v] = sg_f32x4{0.f, 0.f, 0.f, 0.f};
    for (int t = 0; t < a.taps; ++t) {
        const int ty = a.taps == 9 ? t / 3 : 0, tx = a.taps == 9 ? t % 3 : 0;
        const int iy = a.stride * oy + ty - a.pad, ix = a.stride * ox + tx - a.pad;
        const bool bin = pin && iy >= 0 && iy < a.Hi && ix >= 0 && ix < a.Wi;
        const int64_t goff = bin ? (int64_t)iy * a.Wi + ix : 0;
        const float* wt = a.wk + (int64_t)t * a.Ci * a.Co;
        for (int ci0 = 0; ci0 < a.Ci; ci0 += SG_KC) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int kk = kr + 4 * j, ci = ci0 + kk;
                As[kk][col] = (ci < a.Ci && co_in) ? wt[(int64_t)ci * a.Co + co0 + col] : 0.f;
                Bs[kk][col] = (ci < a.Ci && bin) ? gn[(int64_t)ci * plane + goff] : 0.f;
            }
            __syncthreads();
            sg_mma_chunk(As, Bs, acc, wm, wn, lane);
            __syncthreads();
        }
    }
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int co = co0 + wm + 16 * mi + 4 * (lane >> 4) + r;
                const int64_t pc = p0 + wn + 16 * ni + (lane & 15);
                if (co < a.Co && pc < P) store(n, co, pc, acc[mi][ni][r]);
            }
}

static const int64_t SG_MAX_GRID = 0x7fffffff;

// the launch grid of sg_corr_tile, or false when a dimension is out of range
static inline bool sg_corr_grid(int N, int Co, int Ho, int Wo, dim3* grid) {
    const int64_t P = (int64_t)Ho * Wo;
    if ((P + SG_TILE - 1) / SG_TILE > SG_MAX_GRID || (Co + SG_TILE - 1) / SG_TILE > 65535 || N > 65535) return false;
    *grid = dim3((unsigned)((P + SG_TILE - 1) / SG_TILE), (unsigned)((Co + SG_TILE - 1) / SG_TILE), (unsigned)N);
    return true;
}
