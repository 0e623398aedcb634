// p3d_paste_grad.hip — backward of the front-view paste (p3d_paste_front_f32, csrc/p3d_paste.hip) on gfx950; the contract is
// include/p3d_paste_grad.h.
//
// Two launches, both bandwidth-bound and a few microseconds at 512^2:
//   k_paste_bwd_pixel   one thread per output pixel: g_image = g_out (1 - mask); g_paste = g_out mask + g_paste_direct; with
//                       grad_sample the pixel recomputes the forward's up-sampled x / y and its four sampling taps
//                       (p3d_paste_common.hpp: the forward's own expressions), writes the gradient with respect to the up-sampled
//                       x and y to the workspace and scatters g_paste x tap weight onto the illustration's gradient with
//                       global_atomic_add_f32 (no return value) — the only atomics, and only when g_front is asked for;
//   k_paste_bwd_xyz     one thread per render-resolution texel and channel: the adjoint of the r -> S bilinear resize as a GATHER
//                       over the pixels whose up-sampling taps touch the texel, rows then columns in ascending order — a fixed order,
//                       so g_xyz is bitwise reproducible.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/p3d_paste_grad.h"
#include "p3d_paste_common.hpp"

static_assert(sizeof(p3d_paste_grad_args) == 112, "p3d_paste_grad_args: _lib.PasteGradArgs mirrors this layout");

__global__ __launch_bounds__(256) void k_paste_bwd_pixel(p3d_paste_grad_args a, float* g_up) {
    const int S = a.S, r = a.r;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)a.N * S * S) return;
    const int X = (int)(idx % S), Y = (int)((idx / S) % S), n = (int)(idx / ((long long)S * S));
    const size_t SS = (size_t)S * S, pix = (size_t)Y * S + X, img = (size_t)n * 3 * SS;
    const float mask = a.mask[(size_t)n * SS + pix];
    float gp[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const size_t o = img + (size_t)c * SS + pix;
        const float go = a.g_out ? a.g_out[o] : 0.0f;
        if (a.g_image) a.g_image[o] = go * (1.0f - mask);
        gp[c] = go * mask + (a.g_paste ? a.g_paste[o] : 0.0f);
    }
    if (!g_up && !a.g_front) return;
    const float scale = (float)r / (float)S;
    const size_t rr = (size_t)r * r;
    const float* xyz = a.xyz + (size_t)n * 3 * rr;
    const UpIdx uy = up_index(Y, scale, r), ux = up_index(X, scale, r);
    const float upx = bilerp(xyz, r, uy, ux), upy = bilerp(xyz + rr, r, uy, ux);
    const FrontTaps t = front_taps(upx, upy, a.box_warp, S);
    const int x0 = t.x0, y0 = t.y0, x1 = x0 + 1, y1 = y0 + 1;
    const bool bx = x1 < S, by = y1 < S;
    const size_t fbase = (size_t)(a.front_shared ? 0 : n) * 3 * SS;
    if (g_up) {
        const float* front = a.front + fbase;
        float gix = 0.0f, giy = 0.0f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            // transposed input: the tap at (row yy, column xx) of front^T is front[c][xx][yy]; an out-of-range tap counts 0
            const float* f = front + (size_t)c * SS;
            auto at = [&](int yy, int xx) { float v = f[(size_t)xx * S + yy]; return a.normalize_images ? v * 2.0f - 1.0f : v; };
            const float nw = at(y0, x0), ne = bx ? at(y0, x1) : 0.0f, sw = by ? at(y1, x0) : 0.0f, se = (bx && by) ? at(y1, x1) : 0.0f;
            gix += gp[c] * ((ne - nw) * (1.0f - t.ty) + (se - sw) * t.ty);
            giy += gp[c] * ((sw - nw) * (1.0f - t.tx) + (se - ne) * t.tx);
        }
        const float dcoord = -(float)S / a.box_warp;  // d ix / d up_y = d iy / d up_x
        g_up[(size_t)n * 2 * SS + pix] = t.clamped_y ? 0.0f : giy * dcoord;       // up-sampled x (xyz channel 0) drives grid y
        g_up[(size_t)n * 2 * SS + SS + pix] = t.clamped_x ? 0.0f : gix * dcoord;  // up-sampled y (xyz channel 1) drives grid x
    }
    if (a.g_front) {
        float* gfront = a.g_front + fbase;
        const float k = a.normalize_images ? 2.0f : 1.0f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float* f = gfront + (size_t)c * SS;
            const float g = gp[c] * k;
            if (g == 0.0f) continue;
            unsafeAtomicAdd(f + (size_t)x0 * S + y0, g * t.wnw);
            if (bx) unsafeAtomicAdd(f + (size_t)x1 * S + y0, g * t.wne);
            if (by) unsafeAtomicAdd(f + (size_t)x0 * S + y1, g * t.wsw);
            if (bx && by) unsafeAtomicAdd(f + (size_t)x1 * S + y1, g * t.wse);
        }
    }
}

// The output rows (or columns) whose up-sampling taps can touch texel j: src = (i + 0.5) * scale - 0.5 in (j - 1, j + 1), widened by
// one on each side against rounding and clamped to the image; the caller tests every candidate with up_index itself.
DEV void touch_range(int j, float inv_scale, int S, int& lo, int& hi) {
    lo = (int)floorf(((float)j - 0.5f) * inv_scale - 0.5f) - 1;
    hi = (int)ceilf(((float)j + 1.5f) * inv_scale - 0.5f) + 1;
    lo = lo < 0 ? 0 : lo;
    hi = hi > S - 1 ? S - 1 : hi;
}
DEV float touch_weight(const UpIdx& u, int j) { return (u.i0 == j ? 1.0f - u.l : 0.0f) + (u.i1 == j ? u.l : 0.0f); }

__global__ __launch_bounds__(256) void k_paste_bwd_xyz(p3d_paste_grad_args a, const float* g_up) {
    const int S = a.S, r = a.r;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)a.N * 3 * r * r) return;
    const int i = (int)(idx % r), j = (int)((idx / r) % r), c = (int)((idx / ((long long)r * r)) % 3), n = (int)(idx / ((long long)3 * r * r));
    if (c == 2) {  // the paste samples the illustration at (x, y) only
        a.g_xyz[idx] = 0.0f;
        return;
    }
    const float scale = (float)r / (float)S, inv_scale = (float)S / (float)r;
    const float* g = g_up + ((size_t)n * 2 + c) * S * S;
    int ylo, yhi, xlo, xhi;
    touch_range(j, inv_scale, S, ylo, yhi);
    touch_range(i, inv_scale, S, xlo, xhi);
    float acc = 0.0f;
    for (int Y = ylo; Y <= yhi; ++Y) {
        const float wy = touch_weight(up_index(Y, scale, r), j);
        if (wy == 0.0f) continue;
        float row = 0.0f;
        for (int X = xlo; X <= xhi; ++X) {
            const float wx = touch_weight(up_index(X, scale, r), i);
            if (wx != 0.0f) row += g[(size_t)Y * S + X] * wx;
        }
        acc += row * wy;
    }
    a.g_xyz[idx] = acc;
}

extern "C" size_t p3d_paste_front_backward_workspace_bytes(int N, int S) {
    if (N <= 0 || S <= 0) return 0;
    const size_t b = (size_t)N * 2 * S * S * sizeof(float);
    return (b + 255) / 256 * 256;
}

extern "C" int p3d_paste_front_backward_f32(const p3d_paste_grad_args* args, void* stream) {
    if (!args) return P3D_E_ARG;
    const p3d_paste_grad_args& a = *args;
    if (!a.mask || (!a.g_out && !a.g_paste) || (!a.g_image && !a.g_xyz && !a.g_front) || a.N <= 0 || a.r <= 0 || a.S <= 0) return P3D_E_ARG;
    if ((a.g_xyz || a.g_front) && (!a.grad_sample || !a.xyz || !a.front)) return P3D_E_ARG;
    if (a.r > 4096 || a.S > 8192) return P3D_E_RANGE;
    float* g_up = nullptr;
    if (a.g_xyz) {
        if (!a.workspace || ((uintptr_t)a.workspace & 255)) return P3D_E_ARG;
        if (a.workspace_bytes < p3d_paste_front_backward_workspace_bytes(a.N, a.S)) return P3D_E_WORKSPACE;
        g_up = (float*)a.workspace;
    }
    hipStream_t st = (hipStream_t)stream;
    if (a.g_front) {
        hipError_t e = hipMemsetAsync(a.g_front, 0, (size_t)(a.front_shared ? 1 : a.N) * 3 * a.S * a.S * sizeof(float), st);
        if (e != hipSuccess) return (int)e;
    }
    const long long total = (long long)a.N * a.S * a.S;
    hipLaunchKernelGGL(k_paste_bwd_pixel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, a, g_up);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    if (a.g_xyz) {
        const long long texels = (long long)a.N * 3 * a.r * a.r;
        hipLaunchKernelGGL(k_paste_bwd_xyz, dim3((unsigned)((texels + 255) / 256)), dim3(256), 0, st, a, (const float*)g_up);
        e = hipGetLastError();
    }
    return e == hipSuccess ? P3D_OK : (int)e;
}
