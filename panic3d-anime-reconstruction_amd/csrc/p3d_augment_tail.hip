// p3d_augment_tail.hip — the augmentation pipe's tail (include/p3d_augment_tail.h).
//
//   k_tail          the per-sample separable filter on the reflected image, the noise and the cutout in one launch.  One workgroup takes
//                   a 64-wide tile of one plane, on the pattern of k_blur (p3d_loss.hip): it stages the tile with its R-wide halo in LDS
//                   through the reflect index, runs the row pass from there into a second LDS buffer for the tile's 64 columns and every
//                   staged row, and the column pass from that buffer to global memory with the noise's fma and the cutout's select in
//                   the store.  Lanes run along x in both passes: every LDS access of a wave is 64 consecutive words and every global
//                   store a full row segment.  The sample's taps are uniform per workgroup.
//   k_tail_adjoint  gx = Fr^T Fc^T (mask . g) in one launch: the masked cotangent with its halo (zero outside the image) in LDS, the
//                   column pass's transposed correlation and its reflect fold into a second LDS buffer for the tile's rows and every
//                   staged column, then the row pass and its fold to global memory.  A source pixel's mirror images are read from the
//                   same staged halo: an image of a pixel within R of a border lies within R of that border.
//   k_tail_point    without a filter: the noise and the cutout (or the mask alone, the adjoint) per element.
// Every sum runs in a fixed order with no atomics: the results are bitwise reproducible.
#include <hip/hip_runtime.h>

#include "../../include/p3d_augment_tail.h"
#include "p3d_paste_common.hpp"

#define TL_WG 256
#define TL_TW P3D_TAIL_TILE_W
#define TL_MAX_GRID 0x7fffffffLL

// forward: the staged tile [TH + 2R][TW + 2R] and the row pass's output [TH + 2R][TW]
static inline size_t tail_lds_bytes(int TH, int R) { return sizeof(float) * (size_t)(TH + 2 * R) * (size_t)(2 * TL_TW + 2 * R); }
// adjoint: the staged cotangent [TH + 2R][TW + 2R] and the column pass's output [TH][TW + 2R]
static inline size_t tail_adj_lds_bytes(int TH, int R) { return sizeof(float) * (size_t)(2 * TH + 2 * R) * (size_t)(TL_TW + 2 * R); }

// the tallest tile of which two workgroups fit a CU's LDS: a taller tile repeats less of the row pass over its halo rows
static inline int tail_tile_h(int R, bool adjoint) {
    for (int th = 64; th > 16; th >>= 1)
        if ((adjoint ? tail_adj_lds_bytes(th, R) : tail_lds_bytes(th, R)) <= P3D_TAIL_LDS_BYTES) return th;
    return 16;
}

DEV int tl_reflect(int q, int n) { return q < 0 ? -q : (q >= n ? 2 * (n - 1) - q : q); }

DEV bool tl_cut(const int* __restrict__ rect, int n, int i, int j) {
    if (!rect) return false;
    const int* r = rect + 4 * (int64_t)n;
    return j >= r[0] && j < r[1] && i >= r[2] && i < r[3];
}

__global__ __launch_bounds__(TL_WG) void k_tail(const float* __restrict__ x, const float* __restrict__ taps, int K, const float* __restrict__ z,
                                                const float* __restrict__ sigma, const int* __restrict__ rect, int C, int H, int W, int TH,
                                                int tiles_x, int tiles_y, float* __restrict__ y) {
    extern __shared__ __attribute__((aligned(16))) char tl_smem[];
    const int R = K >> 1, SW = TL_TW + 2 * R, SH = TH + 2 * R;
    float* st = (float*)tl_smem;  // [SH][SW]
    float* mid = st + SH * SW;    // [SH][TL_TW]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t b = blockIdx.x;
    const int x0 = (int)(b % tiles_x) * TL_TW, y0 = (int)((b / tiles_x) % tiles_y) * TH;
    const int64_t pl = b / ((int64_t)tiles_x * tiles_y);
    const int n = (int)(pl / C);
    const int64_t plane = pl * ((int64_t)H * W);
    const float* xp = x + plane;
    const float* h = taps + (int64_t)n * K;
    // the padded rows (columns) an output of this tile reads end at H - 1 + R (W - 1 + R): a ragged tile stages no further
    const int nrows = min(SH, H - y0 + 2 * R), ncols = min(SW, W - x0 + 2 * R);
    for (int sy = wave; sy < nrows; sy += TL_WG / 64) {
        const float* row = xp + (int64_t)tl_reflect(y0 - R + sy, H) * W;
        for (int sx = lane; sx < ncols; sx += 64) st[sy * SW + sx] = row[tl_reflect(x0 - R + sx, W)];
    }
    __syncthreads();
    const int gx = x0 + lane;
    if (gx < W) {
        for (int sy = wave; sy < nrows; sy += TL_WG / 64) {
            const float* s = st + sy * SW + lane;
            float acc = 0.f;
#pragma unroll 8
            for (int t = 0; t < K; ++t) acc = __builtin_fmaf(h[t], s[t], acc);
            mid[sy * TL_TW + lane] = acc;
        }
    }
    __syncthreads();
    if (gx >= W) return;
    const float sg = sigma ? sigma[n] : 0.f;
    for (int oy = wave; oy < TH; oy += TL_WG / 64) {
        const int gy = y0 + oy;
        if (gy >= H) break;
        const float* s = mid + oy * TL_TW + lane;
        float acc = 0.f;
#pragma unroll 8
        for (int t = 0; t < K; ++t) acc = __builtin_fmaf(h[t], s[t * TL_TW], acc);
        const int64_t o = plane + (int64_t)gy * W + gx;
        if (z) acc = __builtin_fmaf(sg, z[o], acc);
        y[o] = tl_cut(rect, n, gy, gx) ? 0.f : acc;
    }
}

// sum over k ascending with 0 <= q - k + R < n of h[k] m[(q - k + R - origin) * stride]: one padded position's transposed correlation
DEV float tl_adj_chain(const float* __restrict__ h, int K, int R, const float* m, int stride, int origin, int q, int n) {
    const int klo = max(0, q + R - (n - 1)), khi = min(K - 1, q + R);
    float acc = 0.f;
    for (int k = klo; k <= khi; ++k) acc = __builtin_fmaf(h[k], m[(q - k + R - origin) * stride], acc);
    return acc;
}

__global__ __launch_bounds__(TL_WG) void k_tail_adjoint(const float* __restrict__ g, const float* __restrict__ taps, int K,
                                                        const int* __restrict__ rect, int C, int H, int W, int TH, int tiles_x, int tiles_y,
                                                        float* __restrict__ gx_out) {
    extern __shared__ __attribute__((aligned(16))) char tl_smem[];
    const int R = K >> 1, SW = TL_TW + 2 * R, SH = TH + 2 * R;
    float* st = (float*)tl_smem;  // [SH][SW]: mask . g, zero outside the image
    float* mid = st + SH * SW;    // [TH][SW]: the column pass's result for the tile's rows, zero outside the image
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t b = blockIdx.x;
    const int x0 = (int)(b % tiles_x) * TL_TW, y0 = (int)((b / tiles_x) % tiles_y) * TH;
    const int64_t pl = b / ((int64_t)tiles_x * tiles_y);
    const int n = (int)(pl / C);
    const int64_t plane = pl * ((int64_t)H * W);
    const float* gp = g + plane;
    const float* h = taps + (int64_t)n * K;
    for (int sy = wave; sy < SH; sy += TL_WG / 64) {
        const int gy = y0 - R + sy;
        const bool in_y = gy >= 0 && gy < H;
        for (int sx = lane; sx < SW; sx += 64) {
            const int gx = x0 - R + sx;
            float v = 0.f;
            if (in_y && gx >= 0 && gx < W && !tl_cut(rect, n, gy, gx)) v = gp[(int64_t)gy * W + gx];
            st[sy * SW + sx] = v;
        }
    }
    __syncthreads();
    // columns: a[i] = P[i] + P[-i] + P[2 (H - 1) - i].  A row of the tile is uniform per wave, so are its images and their tap ranges.
    for (int oy = wave; oy < TH; oy += TL_WG / 64) {
        const int i = y0 + oy;
        for (int sx = lane; sx < SW; sx += 64) {
            const int gx = x0 - R + sx;
            float v = 0.f;
            if (i < H && gx >= 0 && gx < W) {
                const float* m = st + sx;
                const float* s = m + (oy + 2 * R) * SW;  // itself: the staged rows i + R - k, zero where the image ends
#pragma unroll 8
                for (int k = 0; k < K; ++k) v = __builtin_fmaf(h[k], s[-k * SW], v);
                if (i >= 1 && i <= R) v += tl_adj_chain(h, K, R, m, SW, y0 - R, -i, H);
                if (i >= H - 1 - R && i <= H - 2) v += tl_adj_chain(h, K, R, m, SW, y0 - R, 2 * (H - 1) - i, H);
            }
            mid[oy * SW + sx] = v;
        }
    }
    __syncthreads();
    const int j = x0 + lane;
    if (j >= W) return;
    for (int oy = wave; oy < TH; oy += TL_WG / 64) {
        const int i = y0 + oy;
        if (i >= H) break;
        const float* m = mid + oy * SW;
        const float* s = m + lane + 2 * R;  // itself: the staged columns j + R - k
        float v = 0.f;
#pragma unroll 8
        for (int k = 0; k < K; ++k) v = __builtin_fmaf(h[k], s[-k], v);
        if (j >= 1 && j <= R) v += tl_adj_chain(h, K, R, m, 1, x0 - R, -j, W);
        if (j >= W - 1 - R && j <= W - 2) v += tl_adj_chain(h, K, R, m, 1, x0 - R, 2 * (W - 1) - j, W);
        gx_out[plane + (int64_t)i * W + j] = v;
    }
}

__global__ __launch_bounds__(TL_WG) void k_tail_point(const float* __restrict__ x, const float* __restrict__ z, const float* __restrict__ sigma,
                                                      const int* __restrict__ rect, int64_t total, int C, int H, int W, float* __restrict__ y) {
    const int64_t o = (int64_t)blockIdx.x * TL_WG + threadIdx.x;
    if (o >= total) return;
    const int j = (int)(o % W), i = (int)((o / W) % H), n = (int)(o / ((int64_t)W * H * C));
    float v = x[o];
    if (z) v = __builtin_fmaf(sigma[n], z[o], v);
    y[o] = tl_cut(rect, n, i, j) ? 0.f : v;
}

extern "C" int p3d_augment_tail_plan(int K, int* out, int out_len) {
    if (!out || out_len < 4) return P3D_E_ARG;
    if (K == 0) {
        out[0] = out[1] = out[2] = out[3] = 0;
        return 0;
    }
    if (K < 1 || K > P3D_TAIL_MAX_TAPS || (K & 1) == 0) return P3D_E_RANGE;
    const int R = K / 2;
    out[0] = tail_tile_h(R, false);
    out[1] = (int)tail_lds_bytes(out[0], R);
    out[2] = tail_tile_h(R, true);
    out[3] = (int)tail_adj_lds_bytes(out[2], R);
    return 0;
}

static int tail_check(const float* x, const float* taps, int K, int N, int C, int H, int W, const float* y) {
    if (!x || !y || x == y) return P3D_E_ARG;
    if (N <= 0 || C <= 0 || H <= 0 || W <= 0) return P3D_E_ARG;
    if ((taps == nullptr) != (K == 0)) return P3D_E_ARG;
    if (H > P3D_TAIL_MAX_SIDE || W > P3D_TAIL_MAX_SIDE) return P3D_E_RANGE;
    if (taps) {
        if (K < 1 || K > P3D_TAIL_MAX_TAPS || (K & 1) == 0) return P3D_E_RANGE;
        if (K / 2 >= (H < W ? H : W)) return P3D_E_RANGE;  // the reflect index would leave the image
    }
    if ((int64_t)N * C > TL_MAX_GRID) return P3D_E_RANGE;
    return 0;
}

template <typename Kern>
static int tail_lds_attr(Kern kern, size_t lds) {
    if (lds <= 64 * 1024) return 0;  // above the default limit of a launch's dynamic LDS (per device: asked for on every such call)
    const hipError_t attr = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, P3D_TAIL_LDS_BYTES);
    if (attr != hipSuccess) {
        (void)hipGetLastError();
        return (int)attr;
    }
    return 0;
}

static int tail_point(const float* x, const float* z, const float* sigma, const int* rect, int N, int C, int H, int W, float* y, void* stream) {
    const int64_t total = (int64_t)N * C * H * W, blocks = (total + TL_WG - 1) / TL_WG;
    if (blocks > TL_MAX_GRID) return P3D_E_RANGE;
    hipLaunchKernelGGL(k_tail_point, dim3((unsigned)blocks), dim3(TL_WG), 0, (hipStream_t)stream, x, z, sigma, rect, total, C, H, W, y);
    return (int)hipGetLastError();
}

extern "C" int p3d_augment_tail_f32(const float* x, const float* taps, int K, const float* z, const float* sigma, const int* rect, int N,
                                    int C, int H, int W, float* y, void* stream) {
    const int rc = tail_check(x, taps, K, N, C, H, W, y);
    if (rc) return rc;
    if ((z == nullptr) != (sigma == nullptr)) return P3D_E_ARG;
    if (!taps) return tail_point(x, z, sigma, rect, N, C, H, W, y, stream);
    const int R = K / 2, TH = tail_tile_h(R, false);
    const int tiles_x = (W + TL_TW - 1) / TL_TW, tiles_y = (H + TH - 1) / TH;
    if ((int64_t)N * C > TL_MAX_GRID / ((int64_t)tiles_x * tiles_y)) return P3D_E_RANGE;
    const size_t lds = tail_lds_bytes(TH, R);
    const int attr = tail_lds_attr(k_tail, lds);
    if (attr) return attr;
    hipLaunchKernelGGL(k_tail, dim3((unsigned)((int64_t)N * C * tiles_x * tiles_y)), dim3(TL_WG), lds, (hipStream_t)stream, x, taps, K, z, sigma,
                       rect, C, H, W, TH, tiles_x, tiles_y, y);
    return (int)hipGetLastError();
}

extern "C" int p3d_augment_tail_adjoint_f32(const float* g, const float* taps, int K, const int* rect, int N, int C, int H, int W, float* gx,
                                            void* stream) {
    const int rc = tail_check(g, taps, K, N, C, H, W, gx);
    if (rc) return rc;
    if (!taps) return tail_point(g, nullptr, nullptr, rect, N, C, H, W, gx, stream);
    const int R = K / 2, TH = tail_tile_h(R, true);
    const int tiles_x = (W + TL_TW - 1) / TL_TW, tiles_y = (H + TH - 1) / TH;
    if ((int64_t)N * C > TL_MAX_GRID / ((int64_t)tiles_x * tiles_y)) return P3D_E_RANGE;
    const size_t lds = tail_adj_lds_bytes(TH, R);
    const int attr = tail_lds_attr(k_tail_adjoint, lds);
    if (attr) return attr;
    hipLaunchKernelGGL(k_tail_adjoint, dim3((unsigned)((int64_t)N * C * tiles_x * tiles_y)), dim3(TL_WG), lds, (hipStream_t)stream, g, taps, K, rect,
                       C, H, W, TH, tiles_x, tiles_y, gx);
    return (int)hipGetLastError();
}
