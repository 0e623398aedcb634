// p3d_conv_plan.hpp — which kernels run one modulated convolution (modconv_impl, p3d_synthesis.hip), decided in ONE place: the
// main kernel and its grid, the split-K depth, the conversion pass of an fp32 input, the reduction and the last pass, and the
// workspace carve-up.  Host code only (no HIP headers): tests/test_conv_plan.py compiles it into a plain host program.
//   p3d_conv_switches   the environment switches that pin one form against another (tests, A/B runs); read per call
//   p3d_conv_plan       the plan of one call, from its shape, operands and those switches
//   p3d_conv_workspace_bytes   what p3d_modconv2d_workspace_bytes answers: a bound on every plan's carve-up for that shape
// The launchers (p3d_conv_plain.hip, p3d_conv_up.hip, p3d_conv_up4.hip, p3d_fir.hip) launch what the plan names.
#pragma once
#include <stddef.h>
#include <stdlib.h>

#include "../../include/panic3d_hip.h"

#define CONV_TH 8
#define CONV_TW 16
#define WX_TW 32

#ifndef P3D_KSPLIT_TARGET
#define P3D_KSPLIT_TARGET 256  // workgroups a launch is split towards.  Batch-1 backbone, ms: 64 -> 1.31, 128 -> 1.15, 256 -> 1.08, 512 (rounds 1-2) -> 1.15, 1024 -> 1.36 (profiles/history/r03_notes.txt)
#endif
// narrowest map the pipelined plain 3x3 kernels (k_modconv_w3 / k_modconv_w2, a 32-column tile) take
#ifndef P3D_W3_MIN_W
#define P3D_W3_MIN_W 32
#endif
// k_modconv_up3 (image-fed, DMA-pipelined transposed convolution): two-term operands, 16-channel chunks, 32-channel output tiles,
// every map from 4^2 up: below W = 32 its 32-column tile is mostly empty, but the 4^2 .. 16^2 layers are latency, not arithmetic, and
// the pipelined kernel (+ the 5 us conversion pass of its input) still beats k_modconv_up_h there (measured, batch-1 backbone as a
// hipGraph replay: W >= 32 only 0.709 ms, >= 16 0.688, >= 8 0.680-0.689, >= 4 0.689; W = 32: 65.2 -> 47.7 + 4.8 us at 512 -> 512)
#ifndef P3D_UP3_MIN_W
#define P3D_UP3_MIN_W 4
#endif

enum class ConvKernel {
    MODCONV_3, MODCONV_1,    // k_modconv<0 / 1>: fp32 operands, 3x3 / 1x1                          (p3d_conv_plain.hip)
    H_3, H_3_X2, H_1, H_1_X2,  // k_modconv_h<MODE, SPLIT>: f16 / two-term operands, register-staged
    W2, W2_IMG,              // k_modconv_w2<IMG>: two-term 3x3, 32-column tile (fp32 input / an image, O % 64 != 0)
    W3, W3_RGB,              // k_modconv_w3<RGB>: the pipelined plain 3x3 kernel (image input; RGB: the ToRGB layer rides)
    UP, UP_H, UP_H_X2,       // k_modconv_up, k_modconv_up_h<SPLIT>: transposed 3x3, register-staged    (p3d_conv_up.hip)
    UP3, UP3_FUSED, UP5,     // k_modconv_up3<FUSED>, k_modconv_up5: image-fed transposed 3x3
    UP4_16, UP4_8,           // k_modconv_up4<8,2,3> / <4,2,2>: transposed 3x3 + FIR pass + epilogue    (p3d_conv_up4.hip)
};
enum class ConvReduce { NONE, REDUCE, REDUCE_IMG };  // the split-K sum: k_splitk_reduce / k_splitk_reduce_img (+ the next image)
enum class ConvTail {
    NONE,
    ACT_TO_IMAGE,            // up = 1: k_act_to_image of the finished y
    FIR_TILED,               // up = 2: k_fir4x4_tiled (fp32 out)                                        (p3d_fir.hip)
    FIR_IMG, FIR_IMG_ALIGNED,  //        k_fir4x4_img<false, 4, 2> / <true, 2, 3> (image out)
    FIR_IMG2_8, FIR_IMG2_32,   //        k_fir4x4_img2<8 / 32> (image out, few workgroups)
};

struct ConvGrid { unsigned x, y, z; };

// The per-call environment switches; -1: not set.  P3D_UP4=0 / 1: k_modconv_up4 never / wherever legal; P3D_UP4_RPW=0 / 2: its tile
// shape; P3D_UP3_FUSED=0 / 1: k_modconv_up3 without / with the FIR pass inside; P3D_UP5=0 / 1: k_modconv_up5 never / always where
// k_modconv_up3<false> would run; P3D_FIR_IMG2=0 / 8 / 32: k_fir4x4_img2 never / always with that tile height.
struct ConvSwitches { int up4, up4_rpw, up3_fused, up5, fir_img2; };
static inline ConvSwitches p3d_conv_switches() {
    const auto get = [](const char* name) { const char* e = getenv(name); return e ? atoi(e) : -1; };
    return {get("P3D_UP4"), get("P3D_UP4_RPW"), get("P3D_UP3_FUSED"), get("P3D_UP5"), get("P3D_FIR_IMG2")};
}

// ---- the rules the plan and the shape queries share
static inline bool conv_w_wide(int W) { return W >= P3D_W3_MIN_W; }  // k_modconv_w3 / w2
static inline bool conv_w3_applies(int I, int O, int W) { return I % 16 == 0 && O % 64 == 0 && conv_w_wide(W); }
static inline bool conv_up3_applies(int I, int O, int W) { return I % 16 == 0 && O % 32 == 0 && W >= P3D_UP3_MIN_W; }

// split-K factor: small feature maps (4^2..64^2) give too few workgroups for 256 CUs; split the K loop until ~P3D_KSPLIT_TARGET,
// down to ONE 8-channel chunk per workgroup: at batch 1 the 4^2..16^2 layers are a weight stream (9.4 MB for 512 -> 512 x 3x3) that
// 8..16 workgroups cannot pull in (profiles/history/r02_notes.txt)
static inline int conv_ksplit(int N, int I, int O, int GH, int GW, int tw) {
    const long long wgs = (long long)((GW + tw - 1) / tw) * ((GH + CONV_TH - 1) / CONV_TH) * ((O + 63) / 64) * N;
    int ks = 1;
    while (ks < 64 && wgs * ks < P3D_KSPLIT_TARGET && I / (ks * 2) >= 8) ks *= 2;
    return ks;
}
static inline int conv_ksplit_up3(int N, int I, int O, int H, int W) {  // (16-channel chunks)
    const long long wgs = (long long)((W + 1 + WX_TW - 1) / WX_TW) * ((H + 1 + 7) / 8) * (O / 32) * N;
    int ks = 1;
    while (ks < 64 && wgs * ks < P3D_KSPLIT_TARGET && I / (ks * 2) >= 16) ks *= 2;
    return ks;
}
// The launch that takes the ToRGB layer along: the pipelined plain 3x3 kernel, unsplit (the activation image as input is the caller's
// business: it is asked for p3d_conv_takes_image as well)
static inline bool conv_rgb_fusable(int N, int I, int O, int H, int W, int rgbo) {
    return rgbo >= 1 && rgbo <= 4 && conv_w3_applies(I, O, W) && conv_ksplit(N, I, O, H, W, WX_TW) == 1;
}
// the layout of the two-term weight copy the plan of a 3x3 layer consumes (W: the input map's width): the image layouts where the
// layer runs on the pipelined kernels whatever its batch size and split-K depth, OIK elsewhere
static inline int conv_weight_layout(int I, int O, int W, int up) {
    if (I <= 0 || O <= 0 || W <= 0) return P3D_WLAYOUT_OIK;
    if (up == 1 && conv_w3_applies(I, O, W)) return P3D_WLAYOUT_PLAIN;
    if (up == 2 && conv_up3_applies(I, O, W)) return P3D_WLAYOUT_UP;
    return P3D_WLAYOUT_OIK;
}
// when an image-consuming layer (p3d_conv_args.x_img) is accepted: the pipelined kernels
static inline bool conv_takes_image(int I, int O, int W, int up) {
    if (I <= 0 || O <= 0 || W <= 0 || I % 16 != 0) return false;
    return up == 1 ? conv_w_wide(W) : up == 2 && conv_up3_applies(I, O, W);
}

// ---- one call
struct ConvCall {
    int N, I, O, H, W, ks, up;
    int mma;          // P3D_CONV_MMA_*
    bool x_img;       // the input arrives as an activation image
    bool y_img;       // an image output for the next layer is wanted (up = 2: instead of y)
    bool rgb;         // the block's ToRGB layer rides (conv_rgb_fusable)
    int act;
    float alpha;
};

struct ConvPlan {
    ConvKernel main;
    ConvGrid grid;
    int ksplit;
    bool pre_image;   // k_act_to_image of the fp32 input into the workspace first (the main kernel stages from images only)
    bool main_img;    // the main kernel writes the image output itself
    ConvReduce reduce;
    ConvGrid reduce_grid;
    ConvTail tail;
    ConvGrid tail_grid;
    bool fir_sums;    // the FIR pass sums the split-K partials while it loads its tiles (no reduction launch)
    int OH, OW;       // the main kernel's output tensor; up = 2: the intermediate, OW its pitch
    size_t out_elems;
    // the workspace, in bytes from its (256-byte aligned) base: demodulation coefficients, the up = 2 intermediate, split-K partials,
    // the input image; `end`: one past the last byte this call uses
    size_t dcoef, inter, part, img, end;
};

static inline size_t conv_round256(size_t b) { return (b + 255) / 256 * 256; }

// Every decision of modconv_impl.  c: a call that passed modconv_impl's validation.
static inline ConvPlan p3d_conv_plan(const ConvCall& c, const ConvSwitches& s) {
    ConvPlan pl = {};
    const int N = c.N, I = c.I, O = c.O, H = c.H, W = c.W, up = c.up;
    const bool x2 = c.mma == P3D_CONV_MMA_F16X2, f16 = c.mma == P3D_CONV_MMA_F16;
    const bool wide = x2 && c.ks == 3 && up == 1 && conv_w_wide(W);  // k_modconv_w3 / w2
    const bool up3 = x2 && c.ks == 3 && up == 2 && conv_up3_applies(I, O, W);  // k_modconv_up3 / up5 / up4
    // k_modconv_up4 (round 6): transposed convolution + FIR pass + epilogue in one launch, no intermediate and no split-K — every
    // up-sampling layer whose 8-row tiling alone gives the chip enough workgroups (the 64^2 .. 512^2 maps of the backbone and of the
    // super-resolution: from 384 workgroups, measured in p3d_conv_up4.hip) and whose K loop is more than two chunks; smaller maps keep
    // the split-K form (k_modconv_up3 + reduction + FIR pass)
    const long long up4_wgs = (long long)((2 * W + 59) / 60) * ((2 * H + 11) / 12) * (O / 32) * N;
    const bool up4 = up3 && (c.act == 0 || (c.alpha >= 0.0f && c.alpha <= 1.0f)) && (s.up4 < 0 ? up4_wgs >= 384 && I >= 64 : s.up4 != 0);
    const int GH = up == 2 ? H + 1 : H, GW = up == 2 ? W + 1 : W;
    const int ks = pl.ksplit = up4 ? 1 : up3 ? conv_ksplit_up3(N, I, O, H, W) : conv_ksplit(N, I, O, GH, GW, wide ? WX_TW : CONV_TW);
    // An fp32 input of a layer the pipelined kernels run is first turned into the image they stage from (one pass, 8 bytes per value;
    // the generator's blocks hand over images and never need it): ONE kernel does the arithmetic of a layer whichever way its input
    // arrives, so both ways give the same bits.
    pl.pre_image = !c.x_img && (up3 || (wide && conv_w3_applies(I, O, W)));
    const bool ximg = c.x_img || pl.pre_image;
    // up = 2: the intermediate T has 2W + 1 columns, stored at a pitch of 2W + 4 floats with column ox at index ox + 1, so that the
    // FIR pass reads 16-byte aligned windows (k_fir4x4_*)
    pl.OH = up == 2 ? 2 * H + 1 : H;
    pl.OW = up == 2 ? 2 * W + 4 : W;
    pl.out_elems = (size_t)N * O * pl.OH * pl.OW;

    // the main kernel
    const unsigned z = (unsigned)(N * ks);
    if (up == 1 && wide) {
        pl.main = ximg && O % 64 == 0 ? (c.rgb ? ConvKernel::W3_RGB : ConvKernel::W3) : ximg ? ConvKernel::W2_IMG : ConvKernel::W2;
        pl.grid = {(unsigned)(((W + WX_TW - 1) / WX_TW) * ((H + CONV_TH - 1) / CONV_TH)), (unsigned)((O + 63) / 64), z};
    } else if (up == 1) {
        const bool k3 = c.ks == 3;
        pl.main = x2 ? (k3 ? ConvKernel::H_3_X2 : ConvKernel::H_1_X2) : f16 ? (k3 ? ConvKernel::H_3 : ConvKernel::H_1)
                     : (k3 ? ConvKernel::MODCONV_3 : ConvKernel::MODCONV_1);
        pl.grid = {(unsigned)(((W + CONV_TW - 1) / CONV_TW) * ((H + CONV_TH - 1) / CONV_TH)), (unsigned)((O + 63) / 64), z};
    } else if (up4) {
        // the tile shape: 2 = eight waves x 2 rows (16 x 32 grid points) once that tiling alone gives every CU two rounds of
        // workgroups, 0 = four waves x 2 rows (8 x 32) below that (measured: p3d_conv_up4.hip)
        const long long wg16 = (long long)((2 * W + 59) / 60) * ((2 * H + 27) / 28) * (O / 32) * N;
        const bool rows16 = s.up4_rpw == 0 || s.up4_rpw == 2 ? s.up4_rpw == 2 : wg16 >= 512;
        const int orows = rows16 ? 28 : 12;  // output rows of a tile: 2 x grid rows - 4
        pl.main = rows16 ? ConvKernel::UP4_16 : ConvKernel::UP4_8;
        pl.grid = {(unsigned)(((2 * W + 59) / 60) * ((2 * H + orows - 1) / orows)), (unsigned)(O / 32), (unsigned)N};
    } else if (up3 && c.y_img && ks == 1 && (s.up3_fused >= 0 ? s.up3_fused != 0 : I <= 64)) {
        // into an image, unsplit, few input channels: the FIR pass and the epilogue inside k_modconv_up3<true> (no intermediate).
        // Measured (tools/conv_layers_time.py, us): 32 -> 256 @128^2 -> 256^2 71 -> 56; 256 -> 128 @256^2 -> 512^2 240 -> 254: with a
        // long K loop the filter's VALU work (76 us chip-wide) and the 1.42 x MFMA work of the overlapping tiles cost more than the
        // intermediate's round trip.
        pl.main = ConvKernel::UP3_FUSED;
        pl.grid = {(unsigned)(((2 * W + 59) / 60) * ((2 * H + 11) / 12)), (unsigned)(O / 32), (unsigned)N};
    } else if (up3) {
        pl.grid = {(unsigned)(((GW + WX_TW - 1) / WX_TW) * ((GH + 7) / 8)), (unsigned)(O / 32), z};
        // k_modconv_up5 (one workgroup per CU, deep prefetch) while the launch leaves the chip under-filled anyway: up to two
        // workgroups per CU in k_modconv_up3's terms, and a K slice of at least eight chunks: the deep ring's prologue requests three
        // patches and two weight chunks before the first MFMA — on the four-chunk slices of the 16^2 -> 32^2 layer it costs more than
        // it hides (23.7 against 19.5 us); 512 -> 512 @32^2 -> 64^2: 41.5 -> 30.5 us, 512 -> 256 @64^2 -> 128^2: 45.2 -> 42.8
        const long long wgs = (long long)pl.grid.x * pl.grid.y * pl.grid.z;
        if (s.up5 != 0 && (s.up5 == 1 || (wgs <= 640 && I / ks >= 128))) {
            pl.main = ConvKernel::UP5;
            pl.grid = {(unsigned)wgs, 1, 1};
        } else pl.main = ConvKernel::UP3;
    } else {
        pl.main = x2 ? ConvKernel::UP_H_X2 : f16 ? ConvKernel::UP_H : ConvKernel::UP;
        pl.grid = {(unsigned)(((GW + CONV_TW - 1) / CONV_TW) * ((GH + CONV_TH - 1) / CONV_TH)), (unsigned)((O + 63) / 64), z};
    }
    const bool one_launch = pl.main == ConvKernel::UP4_16 || pl.main == ConvKernel::UP4_8 || pl.main == ConvKernel::UP3_FUSED;
    // up = 1 with an image output: k_modconv_w3 writes it from its epilogue when it runs unsplit
    pl.main_img = c.y_img && (one_launch || ((pl.main == ConvKernel::W3 || pl.main == ConvKernel::W3_RGB) && ks == 1));

    // Split-K partial sums.  Up-sampling layer with a SHALLOW split (<= 8 slices: the 64^2 .. 256^2 layers at batch 1): the FIR pass
    // sums the slices while it loads its tiles — one launch and one round trip of the (2H+1)x(2W+1) intermediate less, the same
    // slice-ordered sum.  Deep splits (the 4^2 .. 32^2 layers, up to 64 slices) keep the separate, chip-wide reduction: measured
    // (profiles/history/r03_notes.txt) both a per-element slice loop inside the FIR pass (4.8 + 5.8 -> 37 us at 64 slices) and an
    // in-launch last-arriver reduction of the plain convolutions (release / ticket / acquire: +15 .. +50 us per layer) lose to it.
    pl.fir_sums = up == 2 && ks > 1 && ks <= 8;
    const unsigned red_blocks = (unsigned)((pl.out_elems + 255) / 256);
    if (ks > 1 && !pl.fir_sums) {
        // up = 1 into an image: the sums, the epilogue and the next layer's image in one launch
        pl.reduce = up == 1 && c.y_img ? ConvReduce::REDUCE_IMG : ConvReduce::REDUCE;
        pl.reduce_grid = {red_blocks, 1, 1};
    }
    if (up == 1) {
        if (c.y_img && !pl.main_img && pl.reduce != ConvReduce::REDUCE_IMG) {  // (channel counts the pipelined kernel does not take)
            pl.tail = ConvTail::ACT_TO_IMAGE;
            pl.tail_grid = {(unsigned)(((long long)N * (O / 8) * H * W + 255) / 256), 1, 1};
        }
    } else if (!one_launch && !c.y_img) {
        pl.tail = ConvTail::FIR_TILED;
        pl.tail_grid = {(unsigned)(((2 * W + 31) / 32) * ((2 * H + 31) / 32)), (unsigned)(N * O), 1};
    } else if (!one_launch) {
        // the FIR pass into the next layer's image.  Aligned rows (16-byte windows of the intermediate: its regions start 256-byte
        // aligned, so an even W): two channels per stage, 125 VGPRs, four waves per SIMD (four per stage: 195, two; measured 2-5 %
        // slower).  k_fir4x4_img2 where k_fir4x4_img's 32 x 32 tiles are too few workgroups for the chip (512 channels at 32^2: 64 of
        // them, 17.6 us; 8-row tiles: 256, 13.8 us).  On the larger maps the older kernel — which requests its next stage while it
        // filters — stays ahead despite its bank conflicts (64^2: 13.3 against 15.9 us, 128^2: 20.2 against 27.8 - 30.9: measured,
        // profiles/r06_notes.txt).
        const bool aligned = (pl.OW & 3) == 0 && ((pl.out_elems * 4) & 15) == 0;
        const unsigned tiles = (unsigned)(((2 * W + 31) / 32) * ((2 * H + 31) / 32)), groups = (unsigned)((long long)N * O / 8);
        pl.tail = aligned ? ConvTail::FIR_IMG_ALIGNED : ConvTail::FIR_IMG;
        pl.tail_grid = {tiles, groups, 1};
        if (aligned && s.fir_img2 != 0 && (s.fir_img2 == 8 || s.fir_img2 == 32 || (long long)tiles * groups < 128)) {
            const int rows = s.fir_img2 == 32 ? 32 : 8;
            pl.tail = rows == 32 ? ConvTail::FIR_IMG2_32 : ConvTail::FIR_IMG2_8;
            pl.tail_grid = {(unsigned)(((2 * W + 63) / 64) * ((2 * H + rows - 1) / rows)), groups, 1};
        }
    }

    // the workspace: every region starts 256-byte aligned
    pl.dcoef = 0;
    pl.inter = conv_round256((size_t)N * O * 4);
    pl.part = up == 2 ? pl.inter + conv_round256(pl.out_elems * 4) : pl.inter;
    pl.img = pl.part + (ks > 1 ? conv_round256((size_t)ks * pl.out_elems * 4) : 0);
    size_t end = (size_t)N * O * 4;
    if (up == 2 && !(pl.main == ConvKernel::UP4_16 || pl.main == ConvKernel::UP4_8)) end = pl.inter + pl.out_elems * 4;
    if (ks > 1) end = pl.part + (size_t)ks * pl.out_elems * 4;
    if (pl.pre_image) end = pl.img + (size_t)N * I * H * W * 4;
    pl.end = end;
    return pl;
}

// p3d_modconv2d_workspace_bytes: enough for the plan of every call of this shape — any operand mode, input and output kind — with
// 256 bytes of slack per region.  The deepest split any plan may take (the wide tile of the two-term kernel, k_modconv_up3's own
// depth), and the activation image an fp32 input is turned into wherever a pipelined kernel could run.  Callers may cache it.
static inline size_t p3d_conv_workspace_bytes(int N, int I, int O, int H, int W, int up) {
    size_t b = (size_t)N * O * 4 + 256;  // demodulation coefficients
    const size_t out_elems = (up == 2) ? (size_t)N * O * (2 * H + 1) * (2 * W + 4) : (size_t)N * O * H * W;
    if (up == 2) b += out_elems * 4;  // transposed-conv intermediate
    int ks = conv_ksplit(N, I, O, up == 2 ? H + 1 : H, up == 2 ? W + 1 : W, CONV_TW);
    if (up == 1 && conv_w_wide(W)) {
        const int kw = conv_ksplit(N, I, O, H, W, WX_TW);
        ks = kw > ks ? kw : ks;
    }
    if (ks > 1) b += (size_t)ks * out_elems * 4;  // split-K partial sums
    if (up == 1 && conv_w3_applies(I, O, W)) b += (size_t)N * I * H * W * 4 + 256;  // the image of an fp32 input (k_modconv_w3)
    if (up == 2 && conv_up3_applies(I, O, W)) {  // k_modconv_up3: its own split-K depth, and the image of an fp32 input
        const int k3 = conv_ksplit_up3(N, I, O, H, W);
        if (k3 > ks) b += (size_t)(k3 - (ks > 1 ? ks : 0)) * out_elems * 4;
        b += (size_t)N * I * H * W * 4 + 256;
    }
    return b + 256;
}
