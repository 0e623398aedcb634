// p3d_paste_common.hpp — the index arithmetic the front-view paste (p3d_paste.hip) and its backward (p3d_paste_grad.hip) share, so
// that the backward's taps are the forward's bits: the r -> S bilinear up-sampling (F.interpolate, align_corners=False) and the
// bilinear sampling of the transposed illustration (sample_orthofront, triplane.py:555-564; F.grid_sample, padding_mode='border').
#pragma once
#include <hip/hip_runtime.h>

#define DEV __device__ __forceinline__

struct UpIdx { int i0, i1; float l; };
DEV UpIdx up_index(int i, float scale, int r) {
    float src = ((float)i + 0.5f) * scale - 0.5f;
    src = src < 0.0f ? 0.0f : src;
    UpIdx u;
    u.i0 = (int)src;  // src >= 0: truncation = floor
    u.i0 = u.i0 < r - 1 ? u.i0 : r - 1;
    u.i1 = u.i0 + 1 < r ? u.i0 + 1 : r - 1;
    u.l = src - (float)u.i0;
    return u;
}
DEV float bilerp(const float* m, int r, const UpIdx& y, const UpIdx& x) {
    const float a00 = m[y.i0 * r + x.i0], a01 = m[y.i0 * r + x.i1], a10 = m[y.i1 * r + x.i0], a11 = m[y.i1 * r + x.i1];
    const float w0 = 1.0f - x.l, h0 = 1.0f - y.l;
    return h0 * (w0 * a00 + x.l * a01) + y.l * (w0 * a10 + x.l * a11);
}

// sample_orthofront: vij = 1 - (xyz[[1,0]] + bw/2) / bw; grid = vij * 2 - 1 on the TRANSPOSED illustration (grid x <- xyz channel 1,
// grid y <- channel 0); ix = clamp(((gx + 1) * S - 1) / 2, 0, S - 1), taps at floor / floor + 1 (the out-of-range tap has weight 0).
// clamped_x / clamped_y: the unclamped coordinate lay at or beyond the border (F.grid_sample's backward passes no gradient there).
struct FrontTaps { int x0, y0; float tx, ty, wnw, wne, wsw, wse; bool clamped_x, clamped_y; };
DEV FrontTaps front_taps(float upx, float upy, float box_warp, int S) {
    FrontTaps t;
    const float v0 = 1.0f - (upy + box_warp * 0.5f) / box_warp, v1 = 1.0f - (upx + box_warp * 0.5f) / box_warp;
    const float gx = v0 * 2.0f - 1.0f, gy = v1 * 2.0f - 1.0f;  // grid x <- vij[0], grid y <- vij[1]
    float ix = ((gx + 1.0f) * (float)S - 1.0f) * 0.5f, iy = ((gy + 1.0f) * (float)S - 1.0f) * 0.5f;
    t.clamped_x = !(ix > 0.0f && ix < (float)(S - 1));
    t.clamped_y = !(iy > 0.0f && iy < (float)(S - 1));
    ix = fminf(fmaxf(ix, 0.0f), (float)(S - 1));
    iy = fminf(fmaxf(iy, 0.0f), (float)(S - 1));
    const float fx0 = floorf(ix), fy0 = floorf(iy);
    t.x0 = (int)fx0;
    t.y0 = (int)fy0;
    t.tx = ix - fx0;
    t.ty = iy - fy0;
    t.wnw = (1.0f - t.tx) * (1.0f - t.ty);
    t.wne = t.tx * (1.0f - t.ty);
    t.wsw = (1.0f - t.tx) * t.ty;
    t.wse = t.tx * t.ty;
    return t;
}
