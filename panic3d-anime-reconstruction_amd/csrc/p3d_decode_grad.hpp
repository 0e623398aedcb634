// p3d_decode_grad.hpp — one-sample-per-lane decode on the exact contract, keeping what the backward needs.
//
// The fused forward kernels (p3d_decode.hpp) decode 32 samples per wave on the matrix cores and keep only sigma and the colours.
// The backward needs more per sample: the 12 tap offsets and bilinear weights, the plane mean X, the hidden pre-activations and
// the colour pre-activations.  This is the same sequence of binary32 operations as include/p3d_numerics.h states (the one the CPU
// oracle restates), written per lane: sigma, the mask decision and the colours are the exact forward's bits.
//
// Reference: training/volumetric_rendering/renderer.py:52-81,138-153,266-280; training/triplane.py:516-544.
#pragma once
#include "p3d_math.hpp"
#include "../../include/panic3d_hip.h"

#define P3D_G_NOTAP 0xffffffffu  // tap outside the plane (grid_sample zero padding): no value, no gradient

struct P3dGradTaps {
    uint32_t off[12];  // float offset of the texel's channel 0 inside ONE image [3][H][W][32]; P3D_G_NOTAP if out of range
    float wt[12];      // bilinear weight (nw, ne, sw, se per plane); 0 where the whole plane reads zero
};

// One plane: F.grid_sample(bilinear, zeros, align_corners=False) geometry, numerics as p3d_numerics.h "triplane sample".
// inside = false: the point is outside (-1, W) x (-1, H) and the contract gives the plane feature 0 without reading any tap.
P3D_DEV bool p3d_g_plane_taps(int H, int W, uint32_t plane_off, float gx, float gy, uint32_t* off, float* wt) {
    float ix = (gx + 1.0f) * (0.5f * (float)W) - 0.5f;
    float iy = (gy + 1.0f) * (0.5f * (float)H) - 0.5f;
    if (!(ix > -1.0f && ix < (float)W && iy > -1.0f && iy < (float)H)) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            off[k] = P3D_G_NOTAP;
            wt[k] = 0.0f;
        }
        return false;
    }
    float fx0 = __builtin_floorf(ix), fy0 = __builtin_floorf(iy);
    float wx1 = ix - fx0, wy1 = iy - fy0;
    float wx0 = 1.0f - wx1, wy0 = 1.0f - wy1;
    wt[0] = wy0 * wx0;
    wt[1] = wy0 * wx1;
    wt[2] = wy1 * wx0;
    wt[3] = wy1 * wx1;
    int x0 = (int)fx0, y0 = (int)fy0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int x = x0 + (k & 1), y = y0 + (k >> 1);
        off[k] = (x >= 0 && x < W && y >= 0 && y < H) ? plane_off + ((uint32_t)y * (uint32_t)W + (uint32_t)x) * P3D_C : P3D_G_NOTAP;
    }
    return true;
}

// Tap geometry of the three planes (generate_planes, renderer.py:26-50; plane 2 = (y,z) if plane_mode else (z,x)).
P3D_DEV void p3d_g_taps(int H, int W, float coord_scale, int plane_mode, float px, float py, float pz, P3dGradTaps& tp) {
    float qx = px * coord_scale, qy = py * coord_scale, qz = pz * coord_scale;
    const uint32_t psz = (uint32_t)H * (uint32_t)W * P3D_C;
    p3d_g_plane_taps(H, W, 0, qx, qy, tp.off + 0, tp.wt + 0);
    p3d_g_plane_taps(H, W, psz, qx, qz, tp.off + 4, tp.wt + 4);
    if (plane_mode)
        p3d_g_plane_taps(H, W, 2 * psz, qy, qz, tp.off + 8, tp.wt + 8);
    else
        p3d_g_plane_taps(H, W, 2 * psz, qz, qx, tp.off + 8, tp.wt + 8);
}

// X[c] = ((f0 + f1) + f2) * P3D_THIRD, each f = nw*v00; fma(ne, v01); fma(sw, v10); fma(se, v11) (zero-padded taps read 0).
P3D_DEV void p3d_g_features(const float* __restrict__ img, const P3dGradTaps& tp, float X[P3D_C]) {
    float f[3][P3D_C];
#pragma unroll
    for (int p = 0; p < 3; ++p) {
#pragma unroll
        for (int c = 0; c < P3D_C; ++c) f[p][c] = 0.0f;
        if (tp.off[4 * p] == P3D_G_NOTAP && tp.off[4 * p + 1] == P3D_G_NOTAP && tp.off[4 * p + 2] == P3D_G_NOTAP &&
            tp.off[4 * p + 3] == P3D_G_NOTAP)
            continue;  // outside the plane (or no tap in range): feature 0
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t o = tp.off[4 * p + k];
            const float w = tp.wt[4 * p + k];
#pragma unroll
            for (int c4 = 0; c4 < P3D_C / 4; ++c4) {
                f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
                if (o != P3D_G_NOTAP) v = *reinterpret_cast<const f32x4*>(img + o + 4 * c4);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int c = 4 * c4 + e;
                    f[p][c] = (k == 0) ? w * v[e] : p3d_fma(w, v[e], f[p][c]);
                }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < P3D_C; ++c) X[c] = ((f[0][c] + f[1][c]) + f[2][c]) * P3D_THIRD;
}

// Hidden layer: pre[n] = b0[n] + w0[n] . X in the contract's k order; h[n] = p3d_softplus(pre[n]).
P3D_DEV void p3d_g_hidden(const float* __restrict__ w0, const float* __restrict__ b0, const float X[P3D_C], float pre[P3D_HID],
                          float h[P3D_HID]) {
#pragma unroll
    for (int n = 0; n < P3D_HID; ++n) {
        float a = b0[n];
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            a = p3d_fma(w0[n * P3D_C + s], X[s], a);
            a = p3d_fma(w0[n * P3D_C + 16 + s], X[16 + s], a);
        }
        pre[n] = a;
        h[n] = p3d_softplus(a);
    }
}

// Output layer row o (0: sigma as the two half chains, 1..32: a colour pre-activation).
P3D_DEV float p3d_g_out_row(const float* __restrict__ w1, const float* __restrict__ b1, int o, const float h[P3D_HID]) {
    if (o == 0) {
        float alo = b1[0], ahi = 0.0f;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                const int nlo = 32 * t + (s & 3) + 8 * (s >> 2), nhi = nlo + 4;
                alo = p3d_fma(w1[nlo], h[nlo], alo);
                ahi = p3d_fma(w1[nhi], h[nhi], ahi);
            }
        return alo + ahi;
    }
    float a = b1[o];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const int nlo = 32 * t + (s & 3) + 8 * (s >> 2), nhi = nlo + 4;
            a = p3d_fma(w1[o * P3D_HID + nlo], h[nlo], a);
            a = p3d_fma(w1[o * P3D_HID + nhi], h[nhi], a);
        }
    return a;
}

P3D_DEV float p3d_g_rgb(float a, bool force_sigmoid) {
    const float sg = p3d_sigmoid(a);
    return force_sigmoid ? sg : sg * 1.002f - 0.001f;
}

// Crop / cull / binarize on the raw sigma (renderer.py:138-153,187-198).  Returns the density the forward composites and sets
// *masked when a mask overwrote it (its gradient is then zero: the reference writes a constant into that slot).
P3D_DEV float p3d_g_masks(float sigma, float px, float pz, const p3d_opts& o, bool* masked) {
    bool m = false;
    if (o.flags & P3D_FLAG_CROP) {
        if (__builtin_fabsf(px) > o.crop_limit || __builtin_fabsf(pz) > o.crop_limit) {
            sigma = P3D_SIGMA_MASKED;
            m = true;
        }
    }
    if (o.flags & (P3D_FLAG_CULL | P3D_FLAG_BINARIZE)) {
        const float a = 1.0f - p3d_exp_nonpos(-p3d_softplus(sigma - 1.0f));
        if (o.flags & P3D_FLAG_BINARIZE) {
            sigma = (a < o.cull_thresh) ? P3D_SIGMA_MASKED : P3D_SIGMA_SOLID;
            m = true;
        } else if (a < o.cull_thresh) {
            sigma = P3D_SIGMA_MASKED;
            m = true;
        }
    }
    *masked = m;
    return sigma;
}

// torch's Softplus backward factor (beta 1, threshold 20): 1 above the threshold, sigmoid(x) below.
P3D_DEV float p3d_g_softplus_grad(float x) { return (x > P3D_SOFTPLUS_THRESHOLD) ? 1.0f : p3d_sigmoid(x); }
