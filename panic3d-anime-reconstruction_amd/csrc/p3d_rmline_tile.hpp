// p3d_rmline_tile.hpp — what the forward layer (p3d_rmline.hip) and the backward kernels (p3d_rmline_grad.hip) of the
// illustration-to-render module share, each defined ONCE: the record of a layer, the two loads that stage a tile's input patch in LDS
// (the reference's `stackin` built from image / mask / hull, or a channel-last activation), and the tile loop itself, an implicit GEMM of
// an unpadded 3 x 3 convolution on v_mfma_f32_16x16x4_f32.  Device code only.
#ifndef P3D_RMLINE_TILE_HPP
#define P3D_RMLINE_TILE_HPP
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/p3d_rmline.h"
#include "p3d_rmline_plan.hpp"

#define RM_WG 256   // four waves
#define RM_BATCH 4  // loads a lane has in flight while it stages operands

typedef float rm_f32x4 __attribute__((ext_vector_type(4)));
typedef float rm_f32x2 __attribute__((ext_vector_type(2)));

struct RmConv {
    const float* x;
    const float* image;
    const float* mask;
    const float* hull;
    const float* wk;
    const float* bias;
    float* out;
    int Hin, Win, Ho, Wo, pad, Ci, Co, act, flags;
    int Hi, Wi;  // the image's size under IN_STACK
    int ci4, cip, tiles_x;
    float slope;
};

__device__ __forceinline__ int rm_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// The patch of `ph` x RM_PW pixels whose first pixel is (y0, x0) of the PADDED input, from image / mask / hull with the replicate padding
// as a coordinate clamp: Xs[pixel][pitch], channels 0 .. 3 written (hull absent: 0), channels 4 .. cw - 1 zeroed (cw a multiple of 4).
__device__ __forceinline__ void rm_stage_stack(const RmConv& c, int n, int y0, int x0, int ph, float* Xs, int pitch, int cw) {
    const int tid = threadIdx.x;
    const int64_t plane = (int64_t)c.Hi * c.Wi;
    for (int i = tid; i < ph * RM_PW; i += RM_WG) {
        const int py = i / RM_PW, px = i % RM_PW;
        const int cy = rm_clamp(y0 + py - c.pad, c.Hi - 1), cx = rm_clamp(x0 + px - c.pad, c.Wi - 1);
        const int64_t at = (int64_t)cy * c.Wi + cx;
        const float* p = c.image + (int64_t)n * 3 * plane + at;
        float v0 = p[0], v1 = p[plane], v2 = p[2 * plane];
        if (c.mask && !(c.flags & P3D_RMLINE_IN_NO_MASK)) {
            const float s = 1.f - c.mask[(int64_t)n * plane + at];
            v0 = v0 * s, v1 = v1 * s, v2 = v2 * s;
        }
        const float v3 = c.hull ? c.hull[(int64_t)n * plane + at] : 0.f;
        *(rm_f32x2*)(Xs + i * pitch) = rm_f32x2{v0, v1};
        *(rm_f32x2*)(Xs + i * pitch + 2) = rm_f32x2{v2, v3};
        for (int k = 4; k < cw; k += 2) *(rm_f32x2*)(Xs + i * pitch + k) = rm_f32x2{0.f, 0.f};
    }
}

// The same patch from the channel-last tensor c.x [N][c.Hin][c.Win][c.Ci]; patch pixel (py, px) is tensor pixel (y0 + py - off,
// x0 + px - off).  Pixels outside the tensor and channels c.Ci .. cw - 1 are zeros: a ragged tile's surplus, and with off > 0 the zero
// halo of a full correlation, which therefore never exists in memory.  RM_BATCH loads — every one unconditional, from a clamped index
// (element 0 where the operand is out of range) — are issued before any of them is stored, so that a batch's loads are in flight
// together; the predicates are applied at the store.
__device__ __forceinline__ void rm_stage_cl(const RmConv& c, int n, int y0, int x0, int off, int ph, float* Xs, int pitch, int cw) {
    const int tid = threadIdx.x;
    const int nvec = cw / 4, total = ph * RM_PW * nvec;
    const bool vec = (c.Ci & 3) == 0;
    for (int base = tid; base < total; base += RM_BATCH * RM_WG) {
        rm_f32x4 r[RM_BATCH];
#pragma unroll
        for (int j = 0; j < RM_BATCH; ++j) {
            const int i = base + j * RM_WG, v = i % nvec, pix = i / nvec, gy = y0 + pix / RM_PW - off, gx = x0 + pix % RM_PW - off;
            const bool in = i < total && gy >= 0 && gx >= 0 && gy < c.Hin && gx < c.Win && 4 * v < c.Ci;
            const int64_t at = in ? (((int64_t)n * c.Hin + gy) * c.Win + gx) * c.Ci + 4 * v : 0;
            if (vec) r[j] = *(const rm_f32x4*)(c.x + at);
            else
#pragma unroll
                for (int e = 0; e < 4; ++e) r[j][e] = c.x[in && 4 * v + e < c.Ci ? at + e : 0];
        }
#pragma unroll
        for (int j = 0; j < RM_BATCH; ++j) {
            const int i = base + j * RM_WG, v = i % nvec, pix = i / nvec, gy = y0 + pix / RM_PW - off, gx = x0 + pix % RM_PW - off;
            if (i >= total) continue;
            const bool in = gy >= 0 && gx >= 0 && gy < c.Hin && gx < c.Win;
            float val[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) val[e] = in && 4 * v + e < c.Ci ? r[j][e] : 0.f;
            *(rm_f32x2*)(Xs + pix * pitch + 4 * v) = rm_f32x2{val[0], val[1]};
            *(rm_f32x2*)(Xs + pix * pitch + 4 * v + 2) = rm_f32x2{val[2], val[3]};
        }
    }
}

// The tile loop.  Waves: wave w takes rows w R .. w R + R - 1 of the tile, each 32 pixels = two 16-pixel blocks.
// v_mfma_f32_16x16x4_f32 with the weights as A (A[co = l & 15][k = l >> 4]) and the pixels as B (B[k = l >> 4][pixel = l & 15]): D col
// = l & 15 is the pixel, rows 4 (l >> 4) + r are four consecutive output channels — one 16-byte store per lane into a channel-last
// output.  Xs [4R + 2][RM_PW][cip] is the patch, Ws [9][16 MB][cip] the weights (a filter's channels contiguous).  acc must come in
// as zeros.  PER_TAP = false (the inference forward, whose bits are pinned): a value's sum is ONE fma chain over K = (tap outer, channel inner)
// ascending.  PER_TAP = true (the training forward and the data gradient): each tap is a chain of its own from 0 over its channels, and the nine tap sums are
// added in tap order — no chain longer than the channel count.
// one tap's k-steps into acc: the chain continues from whatever acc holds
template <int MB, int R>
__device__ __forceinline__ void rm_tile_tap(const float* wbase, const float* xbase, int cip, int ci4, int tap, rm_f32x4 (&acc)[MB][2 * R]) {
    constexpr int COT = 16 * MB, NB = 2 * R;
    const int ty = tap / 3, tx = tap % 3;
    auto load = [&](int c4, float* a, float* b) {
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) a[mb] = wbase[(tap * COT + 16 * mb) * cip + c4];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) b[nb] = xbase[((nb / 2 + ty) * RM_PW + 16 * (nb % 2) + tx) * cip + c4];
    };
    auto step = [&](const float* a, const float* b) {
#pragma unroll
        for (int mb = 0; mb < MB; ++mb)
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) acc[mb][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mb], b[nb], acc[mb][nb], 0, 0, 0);
    };
    // two k-steps at a time: the second one's LDS reads are issued before the first one's MFMAs (the same k order)
    float a0[MB], b0[NB], a1[MB], b1[NB];
    int c4 = 0;
    for (; c4 + 4 < ci4; c4 += 8) {
        load(c4, a0, b0);
        load(c4 + 4, a1, b1);
        step(a0, b0);
        step(a1, b1);
    }
    if (c4 < ci4) {
        load(c4, a0, b0);
        step(a0, b0);
    }
}

template <int MB, int R, bool PER_TAP = false>
__device__ __forceinline__ void rm_tile_mma(const float* Xs, const float* Ws, int cip, int ci4, int wave, int lane, rm_f32x4 (&total)[MB][2 * R]) {
    constexpr int NB = 2 * R;
    const int l15 = lane & 15, kq = lane >> 4;
    const float* wbase = Ws + l15 * cip + kq;
    const float* xbase = Xs + (wave * R * RM_PW + l15) * cip + kq;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
        if constexpr (PER_TAP) {
            rm_f32x4 part[MB][NB];
#pragma unroll
            for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) part[mb][nb] = rm_f32x4{0.f, 0.f, 0.f, 0.f};
            rm_tile_tap<MB, R>(wbase, xbase, cip, ci4, tap, part);
#pragma unroll
            for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                    for (int r = 0; r < 4; ++r) total[mb][nb][r] = total[mb][nb][r] + part[mb][nb][r];
        } else {
            rm_tile_tap<MB, R>(wbase, xbase, cip, ci4, tap, total);
        }
    }
}

#define RM_MAX_DEVICES 64

// a launch whose dynamic LDS exceeds the default limit: the limit is a property of (kernel, device) and is raised once for each
static inline int rm_raise_lds(const void* kernel, size_t lds, bool* raised /* [RM_MAX_DEVICES] of this kernel */) {
    if (lds <= 64 * 1024) return 0;
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) return (int)hipGetLastError();
    const bool known = dev >= 0 && dev < RM_MAX_DEVICES;
    if (!known || !raised[dev]) {
        const hipError_t attr = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, RM_LDS_LIMIT);
        if (attr != hipSuccess) {
            (void)hipGetLastError();
            return (int)attr;
        }
        if (known) raised[dev] = true;
    }
    return 0;
}

// a channel-last tensor whose channel count is a multiple of 4 is read and written in 16-byte vectors
static inline bool rm_misaligned(const void* p, int channels) { return p && (channels & 3) == 0 && ((uintptr_t)p & 15) != 0; }
#endif
