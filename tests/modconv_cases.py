"""The designed case list of the FORWARD modulated convolution (ops.modulated_conv2d -> p3d_modconv2d_ex_f32): a covering list, not a
product.  Every case is small (float64 on the CPU in well under a second; the only larger ones need >= 256 workgroups so that the
pipelined plain kernel runs unsplit) and names the cell of the host-side plan (csrc/p3d_conv_plan.hpp) it is there to reach.
tests/test_modconv_cases_cpu.py checks the list against the plan and enforces the coverage conditions;
tests/test_hip_modconv_edges.py runs each case through ops.modulated_conv2d against tests/modconv_ref.py (make_inputs / case_ref).

Coverage conditions: every ConvKernel, ConvReduce and ConvTail value is reached by at least two cases, with N = 1 and N = 3, H < W
and H > W among them; fir_sums, pre_image and main_img are reached true and false on every main kernel where both are possible;
every epilogue option appears in every kernel family; per-sample noise with N = 3 on every pipelined kernel."""
import math
from collections import namedtuple

SQRT2 = math.sqrt(2.0)

Case = namedtuple("Case", "id N I O H W ks up mma layout xin out R noise bias demod act alpha gain clamp sw taps cell why")
# mma: "f32" | "f16" | "x2";  layout: "oik" | "lib" (the one conv_weight_layout asks for);  xin: "f32" | "img" (ActImage);
# out: "y" | "img" (up = 2: instead of y) | "both" (up = 1: y and the image) | "rgb" | "rgb+img" | "rgb-noy" (the ToRGB ride, R channels);
# noise: None | "const" | "per";  demod: True | False | "dcoef" (the caller's coefficients);  sw: the environment switches;
# taps: the 1-D resample filter;  cell: (main kernel, ksplit class "1" | "2-8" | ">8", reduce, tail, fir_sums, pre_image, main_img)

# the epilogue presets: together they hold every option (noise none / shared / per sample, bias absent, demodulate on / off / given,
# linear / lrelu, another alpha, another gain, a clamp that clips)
P0 = dict()
P1 = dict(noise="const", clamp=0.5)
P2 = dict(noise="per", demod="dcoef")
P3 = dict(act="linear", gain=1.0, bias=False, demod=False)
P4 = dict(alpha=2.0, gain=0.7)
P4U = dict(alpha=0.5, gain=0.7)   # (k_modconv_up4 takes 0 <= alpha <= 1 only)
P5 = dict(noise="const", demod="dcoef", clamp=0.5)  # P1 for an image input (its demodulation is the caller's)
ASYM = (1.0, 2.0, 3.0, 5.0)      # a filter that is not its own mirror image: a flip that is left out shows

UP4_8, UP4_16 = {"P3D_UP4": 1, "P3D_UP4_RPW": 0}, {"P3D_UP4": 1, "P3D_UP4_RPW": 2}
UP5 = {"P3D_UP5": 1}

_SPECS = []


def _c(cid, N, I, O, H, W, why, ks=3, up=1, mma="f32", layout="oik", xin="f32", out="y", R=0, sw=None, taps=(1.0, 3.0, 3.0, 1.0), **ep):
    e = dict(noise=None, bias=True, demod=True, act="lrelu", alpha=0.2, gain=SQRT2, clamp=None)
    e.update(ep)
    _SPECS.append(dict(id=cid, N=N, I=I, O=O, H=H, W=W, ks=ks, up=up, mma=mma, layout=layout, xin=xin, out=out, R=R, sw=dict(sw or {}),
                       taps=tuple(taps), why=why, **e))


# ---- k_modconv<0>: fp32 operands, 3x3, 16 x 8 tiles, 8-channel chunks ---------------------------------------------------------------
_c("m3-1x1", 1, 1, 1, 1, 1, "a 1x1 map, one channel in and out", **P3)
_c("m3-1xW", 3, 7, 3, 1, 17, "a 1xW map, a chunk tail, two column tiles, per-sample noise", **P2)
_c("m3-7x15", 1, 9, 63, 7, 15, "one short of a tile both ways, O = 63", **P0)
_c("m3-8x16", 1, 17, 64, 8, 16, "exactly one tile; I = 17 splits in two with a one-channel last chunk", **P1)
_c("m3-9x17", 3, 19, 65, 9, 17, "one past a tile both ways, O = 65, a split with a partial last slice", **P4)
_c("m3-17x7", 1, 19, 3, 17, 7, "H > W, three row tiles", **P1)
_c("m3-toimg", 1, 9, 40, 5, 33, "k_act_to_image as the tail: fp32 kernel, I < 16, unsplit, O % 8 == 0", out="both", **P0)
_c("m3-toimg-n3", 3, 15, 8, 9, 6, "k_act_to_image as the tail with three samples, H > W", out="both", **P2)
_c("m3-deep", 1, 515, 64, 3, 5, "64 slices of 8 channels and a ragged last one: the chip-wide reduction", **P1)
_c("m3-redimg", 1, 40, 16, 4, 4, "a split layer with an image output: k_splitk_reduce_img", out="both", **P3)
_c("m3-redimg-n3", 3, 40, 16, 9, 4, "k_splitk_reduce_img with three samples, H > W", out="both", **P2)
# ---- k_modconv<1>: fp32 operands, 1x1 -----------------------------------------------------------------------------------------------
_c("m1-1x1", 1, 1, 1, 1, 1, "a 1x1 map, 1x1 taps", ks=1, **P3)
_c("m1-9x15", 3, 19, 3, 9, 15, "the ToRGB shape: O = 3, ragged everything, per-sample noise", ks=1, **P2)
_c("m1-17x7", 1, 17, 65, 17, 7, "H > W, O = 65, a split with a partial slice", ks=1, **P1)
_c("m1-split", 1, 128, 64, 8, 16, "eight slices: k_splitk_reduce after a 1x1 layer", ks=1, **P4)
_c("m1-7x33", 3, 7, 63, 7, 33, "one chunk with a tail, three column tiles", ks=1, **P0)
# ---- k_modconv_h: f16 / two-term operands, register-staged, W < 32 (3x3) or any W (1x1) ---------------------------------------------
for m, t in (("f16", "h"), ("x2", "hx")):
    _c(t + "3-1x1", 1, 16, 1, 1, 1, "a 1x1 map; I = 16 split into two 8-channel slices", mma=m, **P3)
    _c(t + "3-9x17", 3, 48, 65, 9, 17, "three chunks under a split, O = 65, one past a tile, per-sample noise", mma=m, **P2)
    _c(t + "3-8x31", 1, 80, 64, 8, 31, "five chunks under a split, W one below the wide rule", mma=m, out="both", **P1)
    _c(t + "3-1x15", 1, 16, 3, 1, 15, "a 1xW map, O = 3", mma=m, **P4)
    _c(t + "3-17x5", 3, 32, 96, 17, 5, "H > W, O = 96", mma=m, **P0)
    _c(t + "1-1x1", 1, 16, 3, 1, 1, "1x1 taps on a 1x1 map", ks=1, mma=m, **P3)
    _c(t + "1-7x33", 3, 48, 63, 7, 33, "1x1 taps take wide maps too: W = 33, O = 63", ks=1, mma=m, **P2)
    _c(t + "1-17x5", 1, 80, 65, 17, 5, "1x1 taps, H > W, five chunks", ks=1, mma=m, **P1)
_c("hx3-deep", 1, 512, 8, 4, 4, "32 slices of one chunk: the chip-wide reduction after the two-term kernel", mma="x2", **P4)
_c("hx3-15x16", 1, 16, 96, 15, 16, "O = 96: a half-empty second channel tile", mma="x2", **P0)
# ---- k_modconv_w2<false>: two-term 3x3, 32-column tiles, fp32 input, O % 64 != 0 ---------------------------------------------------
_c("w2-1x32", 1, 16, 40, 1, 32, "a 1xW map, exactly one 32-column tile, O = 40", mma="x2", **P3)
_c("w2-9x33", 3, 48, 40, 9, 33, "one past a tile both ways, per-sample noise", mma="x2", **P2)
_c("w2-7x63", 1, 80, 65, 7, 63, "O = 65, W one short of two tiles, five chunks in four slices", mma="x2", **P1)
_c("w2-redimg", 1, 32, 40, 8, 65, "split, with an image output: k_splitk_reduce_img", mma="x2", out="both", **P0)
_c("w2-40x33", 1, 16, 40, 40, 33, "H > W: five row tiles", mma="x2", **P4)
_c("w2-toimg", 3, 16, 40, 9, 1350, "unsplit (258 workgroups) with an image output: k_act_to_image as the tail", mma="x2", out="both", **P4)
# ---- k_modconv_w2<true>: the same from an activation image -------------------------------------------------------------------------
_c("w2i-1x32", 1, 16, 40, 1, 32, "image input, a 1xW map", mma="x2", xin="img", **P3)
_c("w2i-9x33", 3, 48, 40, 9, 33, "image input, one past a tile both ways, per-sample noise", mma="x2", xin="img", **P2)
_c("w2i-redimg", 1, 80, 40, 7, 63, "image in, image out, split: k_splitk_reduce_img", mma="x2", xin="img", out="both", **P5)
_c("w2i-35x32", 1, 32, 65, 35, 32, "H > W, O = 65", mma="x2", xin="img", demod="dcoef")
_c("w2i-toimg", 3, 16, 40, 9, 1350, "image in, unsplit, image out: k_act_to_image as the tail", mma="x2", xin="img", out="both", alpha=2.0, gain=0.7, demod="dcoef")
# ---- k_modconv_w3<false>: the pipelined plain 3x3 kernel ---------------------------------------------------------------------------
_c("w3-1x32", 1, 16, 64, 1, 32, "fp32 input turned into an image first; a 1xW map; two 8-channel slices", mma="x2", **P0)
_c("w3-9x33", 3, 48, 128, 9, 33, "image input, the library's weight layout, one past a tile, per-sample noise", mma="x2", xin="img", layout="lib", **P2)
_c("w3-redimg", 1, 80, 64, 7, 63, "image in, image out, split: k_splitk_reduce_img", mma="x2", xin="img", layout="lib", out="both", **P5)
_c("w3-mainimg", 4, 16, 128, 9, 497, "unsplit (256 workgroups): the kernel's epilogue writes the next image itself", mma="x2", xin="img",
   layout="lib", out="both", alpha=2.0, gain=0.7, demod="dcoef")
_c("w3-unsplit", 3, 16, 192, 9, 455, "unsplit from an fp32 input, three channel tiles", mma="x2", layout="lib", **P3)
_c("w3-deep", 1, 512, 64, 8, 32, "32 slices: the chip-wide reduction", mma="x2", **P1)
_c("w3-65x33", 1, 32, 64, 65, 33, "H > W: nine row tiles, the last with one row", mma="x2", xin="img", **P3)
# ---- k_modconv_w3<true>: with the ToRGB layer riding (needs the unsplit launch: >= 256 workgroups) ----------------------------------
_c("rgb-121x33", 4, 16, 128, 121, 33, "H > W, two channel groups, three image channels", mma="x2", xin="img", layout="lib", out="rgb", R=3, **P5)
_c("rgb-n3", 3, 16, 192, 9, 455, "three samples, three groups, four image channels, y and the next image too", mma="x2", xin="img",
   layout="lib", out="rgb+img", R=4, **P2)
_c("rgb-noy", 1, 16, 128, 1, 4065, "a 1xW map, one image channel, y not written", mma="x2", xin="img", out="rgb-noy", R=1, **P3)
# ---- k_modconv_up: fp32 operands, transposed 3x3 + FIR pass -------------------------------------------------------------------------
_c("up-1x1", 1, 1, 1, 1, 1, "a 1x1 map up-sampled to 2x2", up=2, **P3)
_c("up-1x17", 3, 7, 3, 1, 17, "a 1xW map, per-sample noise at 2 x 34", up=2, **P2)
_c("up-7x15", 1, 9, 63, 7, 15, "the (H+1) x (W+1) grid is exactly one tile", up=2, **P1)
_c("up-8x16", 1, 17, 65, 8, 16, "the grid is one past a tile; two slices summed by the FIR pass", up=2, taps=ASYM, **P0)
_c("up-img-odd", 1, 19, 8, 9, 3, "image output at odd W: the unaligned k_fir4x4_img; H > W", up=2, out="img", **P4)
_c("up-img-even", 3, 9, 16, 15, 4, "image output at even W; 2H = 30 rows", up=2, out="img", taps=ASYM, **P2)
_c("up-deep", 1, 515, 8, 3, 5, "64 slices: reduction, then k_fir4x4_tiled", up=2, **P1)
_c("up-deep-img", 1, 256, 8, 2, 2, "16 slices: REDUCE followed by an image FIR", up=2, out="img", **P3)
# ---- k_modconv_up_h: f16 / two-term operands, register-staged transposed 3x3 --------------------------------------------------------
for m, t in (("f16", "uph"), ("x2", "uphx")):
    _c(t + "-1x1", 1, 16, 1, 1, 1, "a 1x1 map", up=2, mma=m, **P3)
    _c(t + "-9x17", 3, 48, 65, 9, 17, "three chunks, O = 65, per-sample noise", up=2, mma=m, **P2)
    _c(t + "-7x15", 1, 80, 72, 7, 15, "the grid is exactly one tile; five chunks under a split, O = 72", up=2, mma=m, **P1)
    _c(t + "-img-odd", 1, 32, 40, 8, 5, "feeding k_fir4x4_img<false,4,2>: image output at odd W; H > W", up=2, mma=m, out="img", **P4)
    _c(t + "-17x4", 3, 16, 3, 17, 4, "O = 3, 2H = 34 rows: one past a 32-row FIR tile", up=2, mma=m, taps=ASYM, **P0)
    _c(t + "-deep-img", 1, 256, 8, 2, 2, "16 slices: REDUCE followed by an image FIR", up=2, mma=m, out="img", **P0)
_c("uphx-w3", 1, 32, 32, 5, 3, "W = 3: below the up3 rule the two-term layer stays register-staged", up=2, mma="x2", **P1)
# ---- k_modconv_up3<false>: image-fed transposed 3x3 + a FIR pass --------------------------------------------------------------------
_c("up3-1x4", 1, 16, 32, 1, 4, "W = 4, the first map the kernel takes; fp32 input; unsplit", up=2, mma="x2", **P3)
_c("up3-9x5", 3, 48, 96, 9, 5, "image in, the library's layout, three chunks in two slices, O = 96, H > W", up=2, mma="x2", xin="img", layout="lib", **P2)
_c("up3-7x31", 1, 80, 32, 7, 31, "five chunks in four slices; image out at odd W", up=2, mma="x2", out="img", **P1)
_c("up3-deep", 1, 512, 32, 2, 4, "16 slices: reduction, then k_fir4x4_tiled", up=2, mma="x2", **P0)
_c("up3-deep-img", 3, 512, 32, 3, 4, "16 slices: REDUCE followed by an image FIR", up=2, mma="x2", xin="img", out="img", alpha=2.0, gain=0.7, demod="dcoef")
_c("up3-firsums-img", 1, 128, 64, 4, 6, "eight slices summed by the image FIR pass", up=2, mma="x2", layout="lib", out="img", **P1)
_c("up3-aligned", 1, 32, 32, 5, 8, "k_fir4x4_img<true,2,3> at a small shape", up=2, mma="x2", out="img", sw={"P3D_FIR_IMG2": 0}, taps=ASYM, **P0)
_c("up3-aligned-n3", 3, 32, 32, 9, 6, "k_fir4x4_img<true,2,3>, three samples, H > W", up=2, mma="x2", out="img", sw={"P3D_FIR_IMG2": 0}, **P2)
_c("up3-img2-32", 3, 32, 32, 17, 30, "k_fir4x4_img2<32>: 34 rows, 60 columns", up=2, mma="x2", out="img", sw={"P3D_FIR_IMG2": 32}, **P2)
_c("up3-img2-32b", 1, 32, 32, 9, 64, "k_fir4x4_img2<32>: 128 columns, two full tiles", up=2, mma="x2", out="img", sw={"P3D_FIR_IMG2": 32}, taps=ASYM, **P4)
_c("up3-img2-32c", 1, 32, 64, 33, 4, "k_fir4x4_img2<32>: H > W, 66 rows", up=2, mma="x2", out="img", sw={"P3D_FIR_IMG2": 32}, **P0)
_c("up3-w63", 1, 32, 32, 3, 63, "image out at W = 63 (126 columns)", up=2, mma="x2", out="img", **P3)
_c("up3-w65", 3, 32, 32, 3, 65, "image out at W = 65 (130 columns)", up=2, mma="x2", out="img", taps=ASYM, **P2)
_c("up3-unfused", 1, 16, 32, 8, 16, "P3D_UP3_FUSED=0: the unsplit kernel feeds an image FIR pass", up=2, mma="x2", out="img", sw={"P3D_UP3_FUSED": 0}, **P4)
_c("up3-refused-up4", 1, 32, 32, 5, 8, "P3D_UP4=1 with alpha = 2: the plan must refuse k_modconv_up4", up=2, mma="x2", sw={"P3D_UP4": 1}, **P4)
# ---- k_modconv_up3<true>: the FIR pass inside (I = 16: unsplit at any map size) ------------------------------------------------------
_c("fused-1x4", 1, 16, 32, 1, 4, "a 1xW map, fp32 input", up=2, mma="x2", out="img", **P3)
_c("fused-7x29", 3, 16, 96, 7, 29, "image in, O = 96, 58 columns: one short of the 60-column tile", up=2, mma="x2", xin="img", layout="lib", out="img", **P2)
_c("fused-14x5", 1, 16, 32, 14, 5, "H > W, 28 rows: one past two 12-row tiles", up=2, mma="x2", out="img", taps=ASYM, **P1)
_c("fused-15x30", 1, 16, 64, 15, 30, "60 columns: exactly one tile; 30 rows", up=2, mma="x2", out="img", **P4)
_c("fused-6x31", 1, 16, 32, 6, 31, "62 columns: one past the tile; 12 rows: exactly one", up=2, mma="x2", xin="img", out="img", **P5)
# ---- k_modconv_up5: the deep-prefetch form of up3<false> ---------------------------------------------------------------------------
_c("up5-7x9", 1, 32, 32, 7, 9, "two chunks in two slices", up=2, mma="x2", sw=UP5, **P0)
_c("up5-9x33", 3, 48, 96, 9, 33, "image in, the grid is one past a tile, O = 96, per-sample noise", up=2, mma="x2", xin="img", layout="lib", sw=UP5, **P2)
_c("up5-1x4", 1, 80, 32, 1, 4, "a 1xW map, five chunks", up=2, mma="x2", sw=UP5, **P3)
_c("up5-deep", 1, 512, 32, 2, 4, "16 slices: the chip-wide reduction", up=2, mma="x2", sw=UP5, **P1)
_c("up5-img", 1, 80, 64, 16, 17, "image out at odd W", up=2, mma="x2", out="img", sw=UP5, **P4)
_c("up5-9x7", 1, 16, 32, 9, 7, "H > W, one chunk, unsplit", up=2, mma="x2", sw=UP5, taps=ASYM, **P1)
# ---- k_modconv_up4: transposed 3x3 + FIR + epilogue in one launch; 60-column tiles of 12 (<4,2,2>) or 28 (<8,2,3>) rows ---------------
for sw, t, h1, h2, h3 in ((UP4_8, "up4s", 6, 7, 5), (UP4_16, "up4l", 14, 15, 13)):
    _c(t + "-1x4", 1, 16, 32, 1, 4, "a 1xW map, fp32 input", up=2, mma="x2", sw=sw, **P3)
    _c(t + "-n3", 3, 48, 96, h1, 29, "rows exactly one tile, 58 columns, image in, O = 96, per-sample noise", up=2, mma="x2", xin="img",
       layout="lib", sw=sw, **P2)
    _c(t + "-img", 1, 80, 32, h2, 30, "rows one past a tile, 60 columns, image out", up=2, mma="x2", out="img", sw=sw, **P1)
    _c(t + "-w31", 1, 32, 64, h3, 31, "rows one short of a tile, 62 columns", up=2, mma="x2", sw=sw, taps=ASYM, **P4U)
    _c(t + "-tall", 3, 32, 64, 31, 5, "H > W, image in and out", up=2, mma="x2", xin="img", out="img", sw=sw, taps=ASYM, **P5)

# the plan cell of every case (csrc/p3d_conv_plan.hpp), by id: checked against the plan by tests/test_modconv_cases_cpu.py
CELLS = {
    'm3-1x1': ('k_modconv<0>', '1', '-', '-', 0, 0, 0),
    'm3-1xW': ('k_modconv<0>', '1', '-', '-', 0, 0, 0),
    'm3-7x15': ('k_modconv<0>', '1', '-', '-', 0, 0, 0),
    'm3-8x16': ('k_modconv<0>', '2-8', 'k_splitk_reduce', '-', 0, 0, 0),
    'm3-9x17': ('k_modconv<0>', '2-8', 'k_splitk_reduce', '-', 0, 0, 0),
    'm3-17x7': ('k_modconv<0>', '2-8', 'k_splitk_reduce', '-', 0, 0, 0),
    'm3-toimg': ('k_modconv<0>', '1', '-', 'k_act_to_image', 0, 0, 0),
    'm3-toimg-n3': ('k_modconv<0>', '1', '-', 'k_act_to_image', 0, 0, 0),
    'm3-deep': ('k_modconv<0>', '>8', 'k_splitk_reduce', '-', 0, 0, 0),
    'm3-redimg': ('k_modconv<0>', '2-8', 'k_splitk_reduce_img', '-', 0, 0, 0),
    'm3-redimg-n3': ('k_modconv<0>', '2-8', 'k_splitk_reduce_img', '-', 0, 0, 0),
    'm1-1x1': ('k_modconv<1>', '1', '-', '-', 0, 0, 0),
    'm1-9x15': ('k_modconv<1>', '2-8', 'k_splitk_reduce', '-', 0, 0, 0),
    'm1-17x7': ('k_modconv<1>', '2-8', 'k_splitk_reduce', '-', 0, 0, 0),
    'm1-split': ('k_modconv<1>', '>8', 'k_splitk_reduce', '-', 0, 0, 0),
    'm1-7x33': ('k_modconv<1>', '1', '-', '-', 0, 0, 0),
    'h3-1x1': ('k_modconv_h<0,false>', '2-8', 'k_splitk_reduce', '-', 0, 0, 0),
    'h3-9x17': ('k_modconv_h<0,false>', '2-8', 'k_splitk_reduce', '-', 0, 0, 0),
    'h3-8x31': ('k_modconv_h<0,false>', '2-8', 'k_splitk_reduce_img', '-', 0, 0, 0),
    'h3-1x15': ('k_modconv_h<0,false>', '2-8', 'k_splitk_reduce', '-', 0, 0, 0),
    'h3-17x5': ('k_modconv_h<0,false>', '2-8', 'k_splitk_reduce', '-', 0, 0, 0),
    'h1-1x1': ('k_modconv_h<1,false>', '2-8', 'k_splitk_reduce', '-', 0, 0, 0),
    'h1-7x33': ('k_modconv_h<1,false>', '2-8', 'k_splitk_reduce', '-', 0, 0, 0),
    'h1-17x5': ('k_modconv_h<1,false>', '2-8', 'k_splitk_reduce', '-', 0, 0, 0),
    'hx3-1x1': ('k_modconv_h<0,true>', '2-8', 'k_splitk_reduce', '-', 0, 0, 0),
    'hx3-9x17': ('k_modconv_h<0,true>', '2-8', 'k_splitk_reduce', '-', 0, 0, 0),
    'hx3-8x31': ('k_modconv_h<0,true>', '2-8', 'k_splitk_reduce_img', '-', 0, 0, 0),
    'hx3-1x15': ('k_modconv_h<0,true>', '2-8', 'k_splitk_reduce', '-', 0, 0, 0),
    'hx3-17x5': ('k_modconv_h<0,true>', '2-8', 'k_splitk_reduce', '-', 0, 0, 0),
    'hx1-1x1': ('k_modconv_h<1,true>', '2-8', 'k_splitk_reduce', '-', 0, 0, 0),
    'hx1-7x33': ('k_modconv_h<1,true>', '2-8', 'k_splitk_reduce', '-', 0, 0, 0),
    'hx1-17x5': ('k_modconv_h<1,true>', '2-8', 'k_splitk_reduce', '-', 0, 0, 0),
    'hx3-deep': ('k_modconv_h<0,true>', '>8', 'k_splitk_reduce', '-', 0, 0, 0),
    'hx3-15x16': ('k_modconv_h<0,true>', '2-8', 'k_splitk_reduce', '-', 0, 0, 0),
    'w2-1x32': ('k_modconv_w2<false>', '2-8', 'k_splitk_reduce', '-', 0, 0, 0),
    'w2-9x33': ('k_modconv_w2<false>', '2-8', 'k_splitk_reduce', '-', 0, 0, 0),
    'w2-7x63': ('k_modconv_w2<false>', '2-8', 'k_splitk_reduce', '-', 0, 0, 0),
    'w2-redimg': ('k_modconv_w2<false>', '2-8', 'k_splitk_reduce_img', '-', 0, 0, 0),
    'w2-40x33': ('k_modconv_w2<false>', '2-8', 'k_splitk_reduce', '-', 0, 0, 0),
    'w2-toimg': ('k_modconv_w2<false>', '1', '-', 'k_act_to_image', 0, 0, 0),
    'w2i-1x32': ('k_modconv_w2<true>', '2-8', 'k_splitk_reduce', '-', 0, 0, 0),
    'w2i-9x33': ('k_modconv_w2<true>', '2-8', 'k_splitk_reduce', '-', 0, 0, 0),
    'w2i-redimg': ('k_modconv_w2<true>', '2-8', 'k_splitk_reduce_img', '-', 0, 0, 0),
    'w2i-35x32': ('k_modconv_w2<true>', '2-8', 'k_splitk_reduce', '-', 0, 0, 0),
    'w2i-toimg': ('k_modconv_w2<true>', '1', '-', 'k_act_to_image', 0, 0, 0),
    'w3-1x32': ('k_modconv_w3<false>', '2-8', 'k_splitk_reduce', '-', 0, 1, 0),
    'w3-9x33': ('k_modconv_w3<false>', '2-8', 'k_splitk_reduce', '-', 0, 0, 0),
    'w3-redimg': ('k_modconv_w3<false>', '2-8', 'k_splitk_reduce_img', '-', 0, 0, 0),
    'w3-mainimg': ('k_modconv_w3<false>', '1', '-', '-', 0, 0, 1),
    'w3-unsplit': ('k_modconv_w3<false>', '1', '-', '-', 0, 1, 0),
    'w3-deep': ('k_modconv_w3<false>', '>8', 'k_splitk_reduce', '-', 0, 1, 0),
    'w3-65x33': ('k_modconv_w3<false>', '2-8', 'k_splitk_reduce', '-', 0, 0, 0),
    'rgb-121x33': ('k_modconv_w3<true>', '1', '-', '-', 0, 0, 0),
    'rgb-n3': ('k_modconv_w3<true>', '1', '-', '-', 0, 0, 1),
    'rgb-noy': ('k_modconv_w3<true>', '1', '-', '-', 0, 0, 0),
    'up-1x1': ('k_modconv_up', '1', '-', 'k_fir4x4_tiled', 0, 0, 0),
    'up-1x17': ('k_modconv_up', '1', '-', 'k_fir4x4_tiled', 0, 0, 0),
    'up-7x15': ('k_modconv_up', '1', '-', 'k_fir4x4_tiled', 0, 0, 0),
    'up-8x16': ('k_modconv_up', '2-8', '-', 'k_fir4x4_tiled', 1, 0, 0),
    'up-img-odd': ('k_modconv_up', '2-8', '-', 'k_fir4x4_img<false,4,2>', 1, 0, 0),
    'up-img-even': ('k_modconv_up', '1', '-', 'k_fir4x4_img2<8>', 0, 0, 0),
    'up-deep': ('k_modconv_up', '>8', 'k_splitk_reduce', 'k_fir4x4_tiled', 0, 0, 0),
    'up-deep-img': ('k_modconv_up', '>8', 'k_splitk_reduce', 'k_fir4x4_img2<8>', 0, 0, 0),
    'uph-1x1': ('k_modconv_up_h<false>', '2-8', '-', 'k_fir4x4_tiled', 1, 0, 0),
    'uph-9x17': ('k_modconv_up_h<false>', '2-8', '-', 'k_fir4x4_tiled', 1, 0, 0),
    'uph-7x15': ('k_modconv_up_h<false>', '2-8', '-', 'k_fir4x4_tiled', 1, 0, 0),
    'uph-img-odd': ('k_modconv_up_h<false>', '2-8', '-', 'k_fir4x4_img<false,4,2>', 1, 0, 0),
    'uph-17x4': ('k_modconv_up_h<false>', '2-8', '-', 'k_fir4x4_tiled', 1, 0, 0),
    'uph-deep-img': ('k_modconv_up_h<false>', '>8', 'k_splitk_reduce', 'k_fir4x4_img2<8>', 0, 0, 0),
    'uphx-1x1': ('k_modconv_up_h<true>', '2-8', '-', 'k_fir4x4_tiled', 1, 0, 0),
    'uphx-9x17': ('k_modconv_up_h<true>', '2-8', '-', 'k_fir4x4_tiled', 1, 0, 0),
    'uphx-7x15': ('k_modconv_up_h<true>', '2-8', '-', 'k_fir4x4_tiled', 1, 0, 0),
    'uphx-img-odd': ('k_modconv_up_h<true>', '2-8', '-', 'k_fir4x4_img<false,4,2>', 1, 0, 0),
    'uphx-17x4': ('k_modconv_up_h<true>', '2-8', '-', 'k_fir4x4_tiled', 1, 0, 0),
    'uphx-deep-img': ('k_modconv_up_h<true>', '>8', 'k_splitk_reduce', 'k_fir4x4_img2<8>', 0, 0, 0),
    'uphx-w3': ('k_modconv_up_h<true>', '2-8', '-', 'k_fir4x4_tiled', 1, 0, 0),
    'up3-1x4': ('k_modconv_up3<false>', '1', '-', 'k_fir4x4_tiled', 0, 1, 0),
    'up3-9x5': ('k_modconv_up3<false>', '2-8', '-', 'k_fir4x4_tiled', 1, 0, 0),
    'up3-7x31': ('k_modconv_up3<false>', '2-8', '-', 'k_fir4x4_img<false,4,2>', 1, 1, 0),
    'up3-deep': ('k_modconv_up3<false>', '>8', 'k_splitk_reduce', 'k_fir4x4_tiled', 0, 1, 0),
    'up3-deep-img': ('k_modconv_up3<false>', '>8', 'k_splitk_reduce', 'k_fir4x4_img2<8>', 0, 0, 0),
    'up3-firsums-img': ('k_modconv_up3<false>', '2-8', '-', 'k_fir4x4_img2<8>', 1, 1, 0),
    'up3-aligned': ('k_modconv_up3<false>', '2-8', '-', 'k_fir4x4_img<true,2,3>', 1, 1, 0),
    'up3-aligned-n3': ('k_modconv_up3<false>', '2-8', '-', 'k_fir4x4_img<true,2,3>', 1, 1, 0),
    'up3-img2-32': ('k_modconv_up3<false>', '2-8', '-', 'k_fir4x4_img2<32>', 1, 1, 0),
    'up3-img2-32b': ('k_modconv_up3<false>', '2-8', '-', 'k_fir4x4_img2<32>', 1, 1, 0),
    'up3-img2-32c': ('k_modconv_up3<false>', '2-8', '-', 'k_fir4x4_img2<32>', 1, 1, 0),
    'up3-w63': ('k_modconv_up3<false>', '2-8', '-', 'k_fir4x4_img<false,4,2>', 1, 1, 0),
    'up3-w65': ('k_modconv_up3<false>', '2-8', '-', 'k_fir4x4_img<false,4,2>', 1, 1, 0),
    'up3-unfused': ('k_modconv_up3<false>', '1', '-', 'k_fir4x4_img2<8>', 0, 1, 0),
    'up3-refused-up4': ('k_modconv_up3<false>', '2-8', '-', 'k_fir4x4_tiled', 1, 1, 0),
    'fused-1x4': ('k_modconv_up3<true>', '1', '-', '-', 0, 1, 1),
    'fused-7x29': ('k_modconv_up3<true>', '1', '-', '-', 0, 0, 1),
    'fused-14x5': ('k_modconv_up3<true>', '1', '-', '-', 0, 1, 1),
    'fused-15x30': ('k_modconv_up3<true>', '1', '-', '-', 0, 1, 1),
    'fused-6x31': ('k_modconv_up3<true>', '1', '-', '-', 0, 0, 1),
    'up5-7x9': ('k_modconv_up5', '2-8', '-', 'k_fir4x4_tiled', 1, 1, 0),
    'up5-9x33': ('k_modconv_up5', '2-8', '-', 'k_fir4x4_tiled', 1, 0, 0),
    'up5-1x4': ('k_modconv_up5', '2-8', '-', 'k_fir4x4_tiled', 1, 1, 0),
    'up5-deep': ('k_modconv_up5', '>8', 'k_splitk_reduce', 'k_fir4x4_tiled', 0, 1, 0),
    'up5-img': ('k_modconv_up5', '2-8', '-', 'k_fir4x4_img<false,4,2>', 1, 1, 0),
    'up5-9x7': ('k_modconv_up5', '1', '-', 'k_fir4x4_tiled', 0, 1, 0),
    'up4s-1x4': ('k_modconv_up4<4,2,2>', '1', '-', '-', 0, 1, 0),
    'up4s-n3': ('k_modconv_up4<4,2,2>', '1', '-', '-', 0, 0, 0),
    'up4s-img': ('k_modconv_up4<4,2,2>', '1', '-', '-', 0, 1, 1),
    'up4s-w31': ('k_modconv_up4<4,2,2>', '1', '-', '-', 0, 1, 0),
    'up4s-tall': ('k_modconv_up4<4,2,2>', '1', '-', '-', 0, 0, 1),
    'up4l-1x4': ('k_modconv_up4<8,2,3>', '1', '-', '-', 0, 1, 0),
    'up4l-n3': ('k_modconv_up4<8,2,3>', '1', '-', '-', 0, 0, 0),
    'up4l-img': ('k_modconv_up4<8,2,3>', '1', '-', '-', 0, 1, 1),
    'up4l-w31': ('k_modconv_up4<8,2,3>', '1', '-', '-', 0, 1, 0),
    'up4l-tall': ('k_modconv_up4<8,2,3>', '1', '-', '-', 0, 0, 1),
}

CASES = [Case(cell=CELLS.get(s["id"]), **s) for s in _SPECS]
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)

# Calls the validation refuses (argument checks: the documented error, nothing launched)
REFUSALS = [
    ("img-narrow", dict(N=1, I=16, O=64, H=8, W=31, up=1, xin="img"), "an ActImage with W < 32 at up = 1"),
    ("img-o-not-32", dict(N=1, I=16, O=40, H=8, W=8, up=2, xin="img"), "an ActImage with O % 32 != 0 at up = 2"),
    ("rgb-split", dict(N=1, I=16, O=64, H=8, W=32, up=1, xin="img", R=3), "a ToRGB ride where conv_fuses_torgb says no"),
    ("wrong-layout", dict(N=1, I=16, O=64, H=8, W=32, up=1, xin="f32", layout=2), "a weight layout that conv_weight_layout does not name"),
]


def refusal_case(rid):
    """The refused call `rid` as a Case: a two-term 3x3 layer with the default epilogue (an image input brings its own dcoef)."""
    spec = dict({r[0]: r[1] for r in REFUSALS}[rid])
    e = dict(id=rid, ks=3, mma="x2", layout="oik", out="rgb" if spec.get("R") else "y", R=0, noise=None, bias=True,
             demod="dcoef" if spec["xin"] == "img" else True, act="lrelu", alpha=0.2, gain=SQRT2, clamp=None, sw={}, taps=(1.0, 3.0, 3.0, 1.0),
             cell=None, why={r[0]: r[2] for r in REFUSALS}[rid])
    e.update(spec)
    return Case(**e)
