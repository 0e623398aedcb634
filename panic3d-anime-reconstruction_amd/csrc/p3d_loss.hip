// p3d_loss.hip — the training loss's operators (include/p3d_loss.h).
//
//   k_blur         separable "same"-size FIR, both passes in one launch.  One workgroup takes a 64-wide tile of one plane: it stages
//                  the tile with its R-wide halo in LDS (zero outside the image), runs the row pass from there into a second LDS
//                  buffer for the tile's 64 columns and every staged row, and the column pass from that buffer to global memory: the
//                  intermediate never leaves the CU.  Lanes run along x in both passes: every LDS access of a wave is 64 consecutive
//                  words (conflict-free) and every global store a full row segment.
//   k_l1           |a - b| summed by lane-strided chains and a fixed tree per workgroup, sign(a - b) * scale on the way;
//   k_view_terms   one 16 x 16 tile of one sample's render-resolution map: the resized alpha with a 2-texel halo in LDS for the box
//                  filter, then per texel the masks, both terms and both gradients;
//   k_sum_rows     the fixed tree over the per-workgroup partials.
// Every sum runs in a fixed order: the results are bitwise reproducible for the same sizes.
#include <hip/hip_runtime.h>

#include "../../include/p3d_loss.h"
#include "p3d_paste_common.hpp"

#define LS_WG 256
#define LS_MAX_GRID 0x7fffffffLL

// fixed-order tree over the workgroup's LS_WG lanes
DEV float ls_block_sum(float v, float* red) {
    const int tid = threadIdx.x;
    __syncthreads();  // red may still be read from a previous sum
    red[tid] = v;
    __syncthreads();
    for (int s = LS_WG / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] = red[tid] + red[tid + s];
        __syncthreads();
    }
    return red[0];
}

// out[row] = sum of partial[row][0 .. nb): lane-strided chains, then the tree.  One workgroup per row.
__global__ __launch_bounds__(LS_WG) void k_sum_rows(const float* __restrict__ partial, int nb, float* __restrict__ out) {
    __shared__ float red[LS_WG];
    const float* p = partial + (int64_t)blockIdx.x * nb;
    float s = 0.f;
    for (int i = threadIdx.x; i < nb; i += LS_WG) s += p[i];
    s = ls_block_sum(s, red);
    if (threadIdx.x == 0) out[blockIdx.x] = s;
}

// ---- the blur -----------------------------------------------------------------------------------------------------------------------
#define BL_TW 64  // tile width = one wave of lanes along x

// LDS of one workgroup: the staged tile [TH + 2R][BL_TW + 2R] and the row pass's output [TH + 2R][BL_TW]
static inline size_t blur_lds_bytes(int TH, int R) { return sizeof(float) * (size_t)(TH + 2 * R) * (size_t)(2 * BL_TW + 2 * R); }

// 32 rows while two workgroups fit a CU's 160 KiB (R <= 34: 69 KiB at R = 30), 16 rows above (141 KiB at R = 63)
static inline int blur_tile_h(int R) { return blur_lds_bytes(32, R) <= 80 * 1024 ? 32 : 16; }

__global__ __launch_bounds__(LS_WG) void k_blur(const float* __restrict__ x, int H, int W, const float* __restrict__ f, int taps, int TH,
                                                int tiles_x, int tiles_y, float* __restrict__ y) {
    extern __shared__ __attribute__((aligned(16))) char ls_smem[];
    const int R = (taps - 1) >> 1, SW = BL_TW + 2 * R, SH = TH + 2 * R;
    float* st = (float*)ls_smem;  // [SH][SW]
    float* mid = st + SH * SW;    // [SH][BL_TW]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t b = blockIdx.x;
    const int x0 = (int)(b % tiles_x) * BL_TW, y0 = (int)((b / tiles_x) % tiles_y) * TH;
    const int64_t plane = b / ((int64_t)tiles_x * tiles_y) * ((int64_t)H * W);
    const float* xp = x + plane;
    // every wave stages, and then filters, the rows wave, wave + 4, ...
    for (int sy = wave; sy < SH; sy += LS_WG / 64) {
        const int gy = y0 - R + sy;
        if (gy < 0 || gy >= H) continue;  // a row outside the image: its row pass is 0 (below)
        const float* row = xp + (int64_t)gy * W;
        for (int sx = lane; sx < SW; sx += 64) {
            const int gx = x0 - R + sx;
            st[sy * SW + sx] = (gx >= 0 && gx < W) ? row[gx] : 0.f;
        }
    }
    __syncthreads();
    for (int sy = wave; sy < SH; sy += LS_WG / 64) {
        const int gy = y0 - R + sy;
        float acc = 0.f;
        if (gy >= 0 && gy < H) {
            const float* s = st + sy * SW + lane;
#pragma unroll 8
            for (int t = 0; t < taps; ++t) acc = __builtin_fmaf(f[t], s[t], acc);
        }
        mid[sy * BL_TW + lane] = acc;
    }
    __syncthreads();
    const int gx = x0 + lane;
    for (int oy = wave; oy < TH; oy += LS_WG / 64) {
        const int gy = y0 + oy;
        if (gy >= H || gx >= W) continue;
        const float* s = mid + oy * BL_TW + lane;
        float acc = 0.f;
#pragma unroll 8
        for (int t = 0; t < taps; ++t) acc = __builtin_fmaf(f[t], s[t * BL_TW], acc);
        y[plane + (int64_t)gy * W + gx] = acc;
    }
}

extern "C" int p3d_blur_f32(const float* x, int64_t NC, int H, int W, const float* f, int taps, float* y, void* stream) {
    if (!x || !f || !y) return P3D_E_ARG;
    if (NC <= 0 || H <= 0 || W <= 0) return P3D_E_ARG;
    if (taps < 1 || taps > P3D_BLUR_MAX_TAPS || (taps & 1) == 0) return P3D_E_RANGE;
    if (H > 32768 || W > 32768) return P3D_E_RANGE;
    const int R = (taps - 1) / 2, TH = blur_tile_h(R);
    const int tiles_x = (W + BL_TW - 1) / BL_TW, tiles_y = (H + TH - 1) / TH;
    if (NC > LS_MAX_GRID / ((int64_t)tiles_x * tiles_y)) return P3D_E_RANGE;
    const size_t lds = blur_lds_bytes(TH, R);
    if (lds > 64 * 1024) {  // above the default limit of a launch's dynamic LDS (per device: asked for on every such call)
        const hipError_t attr = hipFuncSetAttribute((const void*)k_blur, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (attr != hipSuccess) {
            (void)hipGetLastError();
            return (int)attr;
        }
    }
    hipLaunchKernelGGL(k_blur, dim3((unsigned)(NC * tiles_x * tiles_y)), dim3(LS_WG), lds, (hipStream_t)stream, x, H, W, f, taps, TH, tiles_x,
                       tiles_y, y);
    return (int)hipGetLastError();
}

// ---- L1 -----------------------------------------------------------------------------------------------------------------------------
#define L1_MAX_BLOCKS 1024

static inline int l1_blocks(int64_t n) {
    const int64_t nb = (n + 4 * LS_WG - 1) / (4 * LS_WG);
    return (int)(nb < L1_MAX_BLOCKS ? nb : L1_MAX_BLOCKS);
}

__global__ __launch_bounds__(LS_WG) void k_l1(const float* __restrict__ a, const float* __restrict__ b, int64_t n, float scale,
                                              float* __restrict__ g_a, float* __restrict__ partial) {
    __shared__ float red[LS_WG];
    float s = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * LS_WG + threadIdx.x; i < n; i += (int64_t)gridDim.x * LS_WG) {
        const float d = a[i] - b[i];
        s += __builtin_fabsf(d);
        if (g_a) g_a[i] = d > 0.f ? scale : (d < 0.f ? -scale : 0.f);
    }
    s = ls_block_sum(s, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

extern "C" size_t p3d_l1_workspace_bytes(int64_t n) { return n > 0 ? sizeof(float) * (size_t)l1_blocks(n) : 0; }

extern "C" int p3d_l1_f32(const float* a, const float* b, int64_t n, float scale, float* sum, float* g_a, void* workspace,
                          size_t workspace_bytes, void* stream) {
    if (!a || !b || !sum || !workspace) return P3D_E_ARG;
    if (n <= 0) return P3D_E_ARG;
    if (n >= ((int64_t)1 << 40)) return P3D_E_RANGE;
    if (workspace_bytes < p3d_l1_workspace_bytes(n)) return P3D_E_WORKSPACE;
    const int nb = l1_blocks(n);
    hipLaunchKernelGGL(k_l1, dim3((unsigned)nb), dim3(LS_WG), 0, (hipStream_t)stream, a, b, n, scale, g_a, (float*)workspace);
    hipLaunchKernelGGL(k_sum_rows, dim3(1), dim3(LS_WG), 0, (hipStream_t)stream, (const float*)workspace, nb, sum);
    return (int)hipGetLastError();
}

// ---- the terms of one supervised view -----------------------------------------------------------------------------------------------
#define VT_T 16                 // tile edge: 256 lanes, one texel each
#define VT_HALO 2               // the 5 x 5 box filter
#define VT_L (VT_T + 2 * VT_HALO)

struct VtArgs {
    const float *w, *xyz, *gt_alpha, *gt_xyz, *q;
    int N, r, S, tiles, mode;
    float s_alpha, s_depth;
    float *g_w, *g_xyz;
};

__global__ __launch_bounds__(LS_WG) void k_view_terms(VtArgs a, float* __restrict__ partial) {
    __shared__ float as[VT_L][VT_L];
    __shared__ float red[LS_WG];
    const int b = blockIdx.x, r = a.r, S = a.S;
    const int tx = b % a.tiles, ty = (b / a.tiles) % a.tiles, n = b / (a.tiles * a.tiles);
    const float scale = (float)S / (float)r;
    const int64_t SS = (int64_t)S * S, rr = (int64_t)r * r;
    const float* ga = a.gt_alpha + n * SS;
    for (int i = threadIdx.x; i < VT_L * VT_L; i += LS_WG) {
        const int ly = i / VT_L, lx = i % VT_L;
        const int y = ty * VT_T - VT_HALO + ly, x = tx * VT_T - VT_HALO + lx;
        float v = 0.f;  // the box filter's zero padding
        if (y >= 0 && y < r && x >= 0 && x < r) v = bilerp(ga, S, up_index(y, scale, S), up_index(x, scale, S));
        as[ly][lx] = v;
    }
    __syncthreads();
    const int ly = threadIdx.x / VT_T, lx = threadIdx.x % VT_T;
    const int y = ty * VT_T + ly, x = tx * VT_T + lx;
    float ta = 0.f, td = 0.f;
    if (y < r && x < r) {
        float box = 0.f;
#pragma unroll
        for (int dy = 0; dy < 2 * VT_HALO + 1; ++dy)
#pragma unroll
            for (int dx = 0; dx < 2 * VT_HALO + 1; ++dx) box += as[ly + dy][lx + dx];
        const float av = as[ly + VT_HALO][lx + VT_HALO];
        const int64_t o = n * rr + (int64_t)y * r + x;
        const float w = a.w[o];
        const float qv = a.q ? a.q[o] : 1.f;
        const bool m = __builtin_fabsf(box / 25.f - 0.5f) * 2.f > 0.5f;
        const bool mz = m && w > 0.5f && av > 0.5f;
        const float mq = m ? qv : 0.f, mzq = mz ? qv : 0.f;
        const float dw = w - av;
        ta = dw * dw * mq;
        if (a.g_w) a.g_w[o] = a.s_alpha * (2.f * dw) * mq;
        const UpIdx uy = up_index(y, scale, S), ux = up_index(x, scale, S);
        const float* gx = a.gt_xyz + 3 * n * SS;
        const int64_t o3 = 3 * n * rr + (int64_t)y * r + x;
        float g3[3] = {0.f, 0.f, 0.f};
        if (a.mode == P3D_DEPTH_NORM) {
            float e[3], ss = 0.f;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                e[c] = a.xyz[o3 + c * rr] - bilerp(gx + c * SS, S, uy, ux);
                ss += e[c] * e[c];
            }
            const float d = __builtin_sqrtf(ss);
            td = d * mzq;
#pragma unroll
            for (int c = 0; c < 3; ++c) g3[c] = d > 0.f ? a.s_depth * (e[c] / d) * mzq : 0.f;
        } else {
            const int c = a.mode == P3D_DEPTH_Z ? 2 : 0;
            const float e = a.xyz[o3 + c * rr] - bilerp(gx + c * SS, S, uy, ux);
            td = e * e * mzq;
            g3[c] = a.s_depth * (2.f * e) * mzq;
        }
        if (a.g_xyz) {
#pragma unroll
            for (int c = 0; c < 3; ++c) a.g_xyz[o3 + c * rr] = g3[c];
        }
    }
    ta = ls_block_sum(ta, red);
    td = ls_block_sum(td, red);
    if (threadIdx.x == 0) {
        partial[b] = ta;
        partial[gridDim.x + b] = td;
    }
}

static inline int64_t vt_blocks(int N, int r) {
    const int64_t tiles = (r + VT_T - 1) / VT_T;
    return (int64_t)N * tiles * tiles;
}

static int vt_range(int N, int r) {
    if (N <= 0 || r <= 0) return P3D_E_ARG;
    if (r > 16384 || vt_blocks(N, r) > LS_MAX_GRID / 2) return P3D_E_RANGE;
    return 0;
}

extern "C" size_t p3d_view_terms_workspace_bytes(int N, int r) { return vt_range(N, r) ? 0 : 2 * sizeof(float) * (size_t)vt_blocks(N, r); }

extern "C" int p3d_view_terms_f32(const float* weights, const float* xyz, const float* gt_alpha, const float* gt_xyz, const float* q, int N,
                                  int r, int S, int depth_mode, float s_alpha, float s_depth, float* sums, float* g_weights, float* g_xyz,
                                  void* workspace, size_t workspace_bytes, void* stream) {
    if (!weights || !xyz || !gt_alpha || !gt_xyz || !sums || !workspace) return P3D_E_ARG;
    if (S <= 0) return P3D_E_ARG;
    const int rc = vt_range(N, r);
    if (rc) return rc;
    if (r > S || S > 16384) return P3D_E_RANGE;
    if (depth_mode != P3D_DEPTH_Z && depth_mode != P3D_DEPTH_X && depth_mode != P3D_DEPTH_NORM) return P3D_E_RANGE;
    if (workspace_bytes < p3d_view_terms_workspace_bytes(N, r)) return P3D_E_WORKSPACE;
    const int nb = (int)vt_blocks(N, r);
    const VtArgs a = {weights, xyz, gt_alpha, gt_xyz, q, N, r, S, (r + VT_T - 1) / VT_T, depth_mode, s_alpha, s_depth, g_weights, g_xyz};
    hipLaunchKernelGGL(k_view_terms, dim3((unsigned)nb), dim3(LS_WG), 0, (hipStream_t)stream, a, (float*)workspace);
    hipLaunchKernelGGL(k_sum_rows, dim3(2), dim3(LS_WG), 0, (hipStream_t)stream, (const float*)workspace, nb, sums);
    return (int)hipGetLastError();
}
