// p3d_conv_common.hpp — what the translation units of the StyleGAN2 synthesis operators share: the launch parameters of the
// convolution kernels, the two-term operand scaling, the XCD-aware workgroup order, the inline-asm LDS-DMA helpers and the steps
// every convolution kernel takes the same way ("the shared steps" below: the K slice of a workgroup, accumulator zeroing and the
// accumulator-to-channel map, the tap table of the transposed convolution, the patch / weight DMA plans of the
// image-fed kernels, the raw four-phase store).  k_modconv_up4 (p3d_conv_up4.hip) includes this header only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <type_traits>

#include "p3d_conv_plan.hpp"


typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
#define DEV __device__ __forceinline__

#define XS_ROW (CONV_TW + 2)
#define XS_PLANE ((CONV_TH + 2) * XS_ROW)
// a K chunk = 8 input channels (72 k values for 3x3, 8 for 1x1)
template <int MODE> struct ConvTaps;
// N taps; dy, dx: input offset of tap t relative to the output position (tap t is element ky*3+kx of the 3x3 kernel)
template <> struct ConvTaps<0> { static constexpr int N = 9; static constexpr int dy[9] = {-1,-1,-1,0,0,0,1,1,1}; static constexpr int dx[9] = {-1,0,1,-1,0,1,-1,0,1}; };
template <> struct ConvTaps<1> { static constexpr int N = 1; static constexpr int dy[1] = {0}; static constexpr int dx[1] = {0}; };

struct ConvParams {
    const float* x;       // [N][I][H][W]
    const float* w;       // [O][I][ks][ks]
    const void* wh;       // f16 copy [O][ks*ks][I] (f16-operand kernels) or null
    int wsplit;           // wh holds hi parts followed by lo parts (two-term operands)
    int wlayout;          // P3D_WLAYOUT_*: how the two-term copy of the 3x3 weights is laid out (round 6): 0 = [hi|lo][O][9][I]; 1 / 2 = the
                          // consuming kernel's own LDS image per (16-channel chunk, channel tile), see include/panic3d_hip.h
    const float* styles;  // [N][I]
    const float* dcoef;   // [N][O] or null
    const float* noise;   // [OH*OW] (shared) or [N][OH*OW] or null; already multiplied by noise_strength
    const float* bias;    // [O] or null
    float* y;             // [N][O][OH][OW]
    int N, I, O, H, W;    // input dims
    int GH, GW;           // output grid of this launch (phase grid for MODE >= 2)
    int OH, OW;           // output tensor dims
    int ks;               // kernel size of w (1 or 3)
    int noise_per_sample;
    int act;              // 0 linear, 1 lrelu
    float alpha, gain, clamp;
    int epilogue;         // 1: dcoef/noise/bias/act applied here; 0: raw store (transposed-conv intermediate)
    int tox;              // up = 2: the intermediate T [N][O][2H+1][OW = pitch] stores column ox at index ox + tox (tox = 1, pitch = 2W + 4: the
                          // FIR pass reads its 36-column windows — columns X0 - 1 .. X0 + 34 — as aligned 16-byte loads); 0 elsewhere
    int ksplit;           // input channels split over ksplit workgroups (blockIdx.z = n*ksplit + kz); > 1 => raw partials
    int xcd;              // k_modconv_w3 / k_modconv_up3: XCD-aware workgroup order (p3d_wg_order)
    unsigned int* sat;    // caller-owned device word, OR-ed with 1 when a two-term operand left its domain (or null: not reported)
    // ---- the activation IMAGE path (the producer prepares the consumer's operand; see "activation IMAGE" below)
    const void* ximg;     // input as an image [hi | lo][N][I/8][H][W] of 16-byte pieces, or null (then x + styles are used)
    long long ximg_lo;    // byte offset of the lo half of ximg (= N*I*H*W*2)
    // k_modconv_w3 only: ALSO write the result as the image of a following layer with styles ystyles [N][O] (next to the fp32 y)
    void* yimg;
    long long yimg_lo;    // = N*O*OH*OW*2
    const float* ystyles;
    const float* fir;     // k_modconv_up3<true>: the 4x4 filter of the FIR pass it contains (flipped, times up^2)
    // k_modconv_w3<true> only: the block's ToRGB layer (networks_stylegan2.py:366-380, <= 4 output channels) applied to the result in
    // the epilogue — each 64-channel workgroup adds its channels' share into rgbp [O/64][N][rgbo][H][W] (p3d_torgb_combine_f32 sums
    // the shares, adds the bias and the up-sampled skip image); y may then be null (nobody reads the fp32 activation)
    const float* rgbw;    // [rgbo][O] ToRGB weights
    const float* rgbs;    // [N][O] ToRGB styles (already multiplied by the layer's weight_gain)
    float* rgbp;
    int rgbo;
};

DEV float act_apply(float v, int act, float alpha, float gain, float clamp) {
    if (act == 1) v = v < 0.0f ? v * alpha : v;
    v = v * gain;
    if (clamp >= 0.0f) v = __builtin_fminf(__builtin_fmaxf(v, -clamp), clamp);
    return v;
}


#define CONV_OOB ((int)0x80000000)
#define CONV_RSRC_FLAGS 0x00020000

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

// The matrix cores flush f16 subnormals, so the operands are scaled by a power of two before they are split — the weights by
// 2^6 (lo parts of |w| >= 2^-8 stay normal), the modulated activations s*x by 2^4 (|s*x| >= 2^-6; more headroom at the top:
// hi saturates, it does not overflow, at |s*x| = 65504 / 16 = 4094) — and the accumulators are scaled back by 2^-10
// when they are stored; all exact.  A value below those thresholds loses its lo part (absolute error <= 2^-11 |v|, i.e.
// below 8e-6 / 2e-6): rare and small next to the 2^-22 relative rounding of the ordinary terms.
#define HX_SPLIT_SCALE_X 16.0f
#define HX_SPLIT_SCALE_W 64.0f
#define HX_SPLIT_UNSCALE (1.0f / 1024.0f)
// Out of domain: a scaled operand beyond the f16 range (|s*x| > 65504 / 16 = 4094, or NaN) is clamped to +-65504 — finite, wrong —
// and the CALLER's flag word (ConvParams::sat, the `saturated` argument of p3d_modconv2d_f16x2mma_f32) is OR-ed with 1: no state
// lives in the library.
#define WX_ROW (WX_TW + 2)                         // patch columns = LDS row pitch (px)

#define U3_WB (2 * 9 * 64 * 16)                    // one buffer of weights: 18 432

// Workgroup order of the image-fed kernels.  The dispatcher deals consecutive workgroup ids round-robin to the 8 XCDs, each with an L2
// of its own, and in (tile, channel tile) order the four channel tiles of a spatial tile — which read the SAME patch — landed on four
// different XCDs at four different times: 256 -> 256 @256^2 staged 356 MB of patches out of a 67 MB image, all of it past the L2s.
// Here XCD x is given a CONTIGUOUS range of the (slice, tile, channel tile) sequence, channel tile fastest: the channel tiles of a
// tile, and neighbouring tiles with their shared halos, run back to back on one XCD and meet in its L2.
struct WgOrder { int tile, otile, z; };
DEV WgOrder p3d_wg_order(bool xcd) {
    const int T = gridDim.x * gridDim.y * gridDim.z;
    int L = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
    WgOrder r;
    if (!xcd) { r.tile = blockIdx.x; r.otile = blockIdx.y; r.z = blockIdx.z; return r; }
    const int q = T >> 3, rem = T & 7, x = L & 7, m = L >> 3;
    L = x * q + (x < rem ? x : rem) + m;
    r.otile = L % gridDim.y;
    L /= gridDim.y;
    r.tile = L % gridDim.x;
    r.z = L / gridDim.x;
    return r;
}

DEV i32x4 w3_rsrc(const void* base, uint32_t bytes) {
    const uint64_t a = (uint64_t)base;
    i32x4 r;
    r[0] = __builtin_amdgcn_readfirstlane((int)(uint32_t)a);
    r[1] = __builtin_amdgcn_readfirstlane((int)(uint32_t)(a >> 32));
    r[2] = __builtin_amdgcn_readfirstlane((int)bytes);
    r[3] = CONV_RSRC_FLAGS;
    return r;
}
// 64 lanes x 16 bytes from rsrc[voff] to LDS [lds_addr + lane * 16] (lds_addr wave-uniform); one wait state between the M0 write
// and the LDS-DMA (what the compiler inserts for its own: s_nop 0)
DEV void w3_dma16(uint32_t lds_addr, i32x4 rsrc, int voff) {
    lds_addr = (uint32_t)__builtin_amdgcn_readfirstlane((int)lds_addr);  // ("s" alone does not make a value uniform: s_mov_b32 m0, v75 was emitted)
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds" : : "s"(lds_addr), "v"(voff), "s"(rsrc) : "memory");
}
#define W3_VMWAIT(N) asm volatile("s_waitcnt vmcnt(" #N ")" ::: "memory")

// =====================================================================================================================
// The shared steps of the convolution kernels: each is defined here ONCE (the 8 x 16 tile origin and the ordinary epilogue of
// the register-staged kernels: p3d_conv_stage.hpp).  Address arithmetic and stores only — every DMA issue, barrier, counted
// wait and sched_barrier stays in the kernel bodies, which hand-count their vmcnt.
// =====================================================================================================================

// The K slice of a workgroup: z = n * ksplit + kz (blockIdx.z, WgOrder::z or k_modconv_up5's own order) -> sample n and input
// channels [ic_beg, ic_end) = nch 16-channel chunks (the DMA kernels: I % 16 == 0).  The host plan (p3d_conv_plan.hpp:
// conv_ksplit / conv_ksplit_up3) chooses ksplit and nothing else — the slice width is THIS function's: ceil(I / ksplit) rounded
// up to 32 channels, so that every slice starts on a whole chunk of every kernel (8 / 16 channels) and of the image weight layouts
// ([chunk][...], indexed ic0 >> 4).  The rounding can leave the last slices short or empty (ic_beg >= I: nch = 0, every load out of
// range): such a workgroup stores a zero partial sum, which the plan's reduction (it sums all ksplit slices) relies on.
// (Z: blockIdx.z as the unsigned it is, or an int — the quotient of an unsigned division is known to be non-negative, which the
// 64-bit output addressing of the kernels that pass blockIdx.z is compiled with)
struct ConvSlice { int n, kz, ic_beg, ic_end, nch; };
template <typename Z>
DEV ConvSlice conv_slice(const ConvParams& p, Z z) {
    ConvSlice s;
    s.n = z / p.ksplit;
    s.kz = z - s.n * p.ksplit;
    const int ic_per = ((p.I + p.ksplit - 1) / p.ksplit + 31) / 32 * 32;
    s.ic_beg = s.kz * ic_per;
    s.ic_end = (s.ic_beg + ic_per < p.I) ? s.ic_beg + ic_per : p.I;
    s.nch = s.ic_end > s.ic_beg ? (s.ic_end - s.ic_beg) >> 4 : 0;
    return s;
}
// ksplit > 1: a launch stores raw partial sums into slice kz of the partial buffer
DEV float* conv_yout(const ConvParams& p, int kz) { return p.y + (p.ksplit > 1 ? (size_t)kz * p.N * p.O * p.OH * p.OW : 0); }

// acc = 0 for the accumulator arrays the kernels hold ([tile] or [phase | channel tile][row])
template <int M>
DEV void conv_zero(f32x16 (&acc)[M]) {
#pragma unroll
    for (int t = 0; t < M; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
}
template <int M, int N>
DEV void conv_zero(f32x16 (&acc)[M][N]) {
#pragma unroll
    for (int a = 0; a < M; ++a)
#pragma unroll
        for (int b = 0; b < N; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.0f;
}
// register r of a 32x32 accumulator on lane half `half` holds this output channel of the tile's 32
DEV constexpr int conv_acc_ch(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

// The nine products of the stride-2 transposed 3x3 convolution in the order every kernel issues them: product q adds tap TP[q] times
// input BO[q] (0 = x[y][x], 1 = x[y][x-1], 2 = x[y-1][x], 3 = x[y-1][x-1]) into output phase PH[q] = 2 py + px
struct UpTaps {
    static constexpr int PH[9] = {0, 1, 2, 3, 0, 2, 0, 1, 0}, TP[9] = {0, 1, 3, 4, 2, 5, 6, 7, 8}, BO[9] = {0, 0, 0, 0, 1, 1, 2, 2, 3};
};

// ---- the patch of an image-fed kernel: sub-image (hi|lo = which, k half = kh) of the activation image, one 16-byte item per pixel.
// Byte offset of item `it` (row pitch `pitch`, origin one above / left of the tile origin) inside a chunk's [k half][H][W] pieces;
// CONV_OOB (the DMA then writes zeros) for padding and for `item` false (past the sub-image)
DEV int conv_patch_voff(const ConvParams& p, int it, bool item, int pitch, int gy0, int gx0, int kh) {
    const int r = it / pitch, c = it - r * pitch;
    const int iy = gy0 - 1 + r, ix = gx0 - 1 + c;
    const bool ok = item && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
    return ok ? ((kh * p.H + iy) * p.W + ix) * 16 : CONV_OOB;
}
DEV const char* conv_img_base(const ConvParams& p, int HW, int n, int which) {
    return (const char*)p.ximg + (which ? p.ximg_lo : 0) + (size_t)n * (p.I >> 3) * HW * 16;
}
// (The per-chunk buffer resources — base = the chunk's first channel, zero length past the slice — stay lambdas of the kernels: the
// scalar code of the K loops follows the way each kernel writes that select, and one shared form changed three of the loops.)
// ---- the weights of the transposed kernels: 1152 pieces q = (hi|lo, tap, k half, o of 32) per chunk = 18 DMA instructions, wave w
// of NW issues instructions w, w + NW, ...: byte offset of this lane's piece of the wave's i-th instruction.  wlds
// (P3D_WLAYOUT_UP): the weights arrive as the kernels' LDS image [chunk][O/32][hi|lo][tap][k half][32 o][8] (18 KB of consecutive
// bytes per chunk and channel tile, a request = 1 KB of them); else 16-byte pieces gathered out of [hi|lo][O][9][I].  The o0 + o < O
// guard of the gathered form is ALWAYS there: k_modconv_up4's plan has O % 32 == 0 and needs none, and pays one compare per piece
// in its prologue for the single definition.
// (LO = O * 9 * I * 2: bytes of the hi tensor, the lo parts follow it)
template <int NW>
DEV int up_weight_voff(const ConvParams& p, int LO, int wave, int lane, int i, int o0, bool wlds) {
    const int q = (wave + NW * i) * 64 + lane, which = q / 576, rem = q - which * 576;
    const int tap = rem >> 6, kh = (rem >> 5) & 1, o = rem & 31;
    return q >= 1152 ? CONV_OOB : wlds ? q * 16 : (o0 + o < p.O) ? which * LO + (((o0 + o) * 9 + tap) * p.I + 8 * kh) * 2 : CONV_OOB;
}
// ---- raw store of the four output phases of an 8 x 32 tile of grid points (wave w = grid rows 2w, 2w + 1, lane j = column j) into
// the (2H+1) x (2W+1) intermediate or slice kz of the split-K partials: a lane owns both column phases (ox = 2 gx, 2 gx + 1) of its
// grid point: one 8-byte store per (row phase, channel), 32 lanes = 256 contiguous bytes; the last grid column (gx = W) has only
// px = 0: a 4-byte store of its own
DEV void up_store_phases(const ConvParams& p, const f32x16 (&acc)[4][2], const ConvSlice& s, int o0, int gy0, int gx0, int wave, int half, int j) {
    float* yout = conv_yout(p, s.kz) + (size_t)s.n * p.O * p.OH * p.OW;
    const int OHW = p.OH * p.OW;
    auto ry = __builtin_amdgcn_make_buffer_rsrc((void*)yout, 0, p.O * OHW * 4, CONV_RSRC_FLAGS);
    const int gx = gx0 + j;
    const bool edge_tile = gx0 + WX_TW > p.W;  // (uniform) this tile holds the column gx = W
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int gy = gy0 + 2 * wave + t;
#pragma unroll
        for (int py = 0; py < 2; ++py) {
            const bool row_ok = gy <= p.H - py;
            const int base = ((o0 + 4 * half) * OHW + (2 * gy + py) * p.OW + 2 * gx + p.tox) * 4;
            const int off2 = (row_ok && gx < p.W && o0 + 4 * half < p.O) ? base : CONV_OOB;
            const int off1 = (row_ok && gx == p.W && o0 + 4 * half < p.O) ? base : CONV_OOB;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int so = conv_acc_ch(r, 0) * OHW * 4;
                const float v0 = acc[2 * py][t][r] * HX_SPLIT_UNSCALE, v1 = acc[2 * py + 1][t][r] * HX_SPLIT_UNSCALE;
                typedef int i32x2 __attribute__((ext_vector_type(2)));
                __builtin_amdgcn_raw_buffer_store_b64((i32x2){__builtin_bit_cast(int, v0), __builtin_bit_cast(int, v1)}, ry, off2, so, 0);
                if (edge_tile) __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, v0), ry, off1, so, 0);
            }
        }
    }
}

struct FirParams {
    const float* x;  // [NC][H][W]
    const float* f;  // [fh][fw], already flipped for convolution and multiplied by gain
    float* y;        // [NC][OH][OW]
    const float* dcoef;  // [NC] (= [N][C]) or null
    const float* noise;  // [OH*OW] or [N][OH*OW] or null
    const float* bias;   // [C] or null
    long long NC;
    int C, H, W, OH, OW, fh, fw, up, down, padx0, pady0;
    int noise_per_sample, act, epilogue;
    float alpha, gain, clamp;
    const float* nstyles; // k_fir4x4_img: the consuming layer's styles [N][C] (the image holds split(16 * s * y))
    int ksplit;           // k_fir4x4_tiled: x holds ksplit split-K partial tensors, `slice` elements apart, summed in slice order
    long long slice;      // while the tile is loaded (shallow splits only: see modconv_impl); 1 / 0 otherwise
    int pitch, xoff;      // k_fir4x4_*: x rows are `pitch` floats apart and column v sits at index v + xoff (ConvParams::tox); the generic
                          // operator ignores them (pitch = W, xoff = 0)
};

// ---- host side: shared by the translation units of the synthesis operators
static inline int chk_launch() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? P3D_OK : (int)e;
}
// the launchers: each launches the kernel a plan names (p3d_conv_plan.hpp) and decides nothing
void p3d_launch_conv_plain(const ConvParams& p, ConvKernel k, ConvGrid g, hipStream_t st);  // p3d_conv_plain.hip
void p3d_launch_conv_up(const ConvParams& p, ConvKernel k, ConvGrid g, hipStream_t st);     // p3d_conv_up.hip
void p3d_launch_conv_up4(const ConvParams& p, ConvKernel k, ConvGrid g, hipStream_t st);    // p3d_conv_up4.hip
void p3d_launch_fir_pass(const FirParams& q, ConvTail t, ConvGrid g, char* yimg, long long lo_off, unsigned int* sat, hipStream_t st);  // p3d_fir.hip
