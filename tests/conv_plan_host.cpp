// Host program of tests/test_conv_plan.py: the convolution plan (csrc/p3d_conv_plan.hpp) compiled without any device code.
// stdin, one line per request:
//   s N I O H W up                                  sweep every operand mode, input / output kind, act and forcing switch of
//                                                   this shape and check that each plan's carve-up fits the workspace query
//   p N I O H W ks up mma x_img y_img rgb act alpha  print the default-environment plan of one call: main ksplit reduce tail
//   q N I O H W ks up mma x_img y_img rgb act alpha up4 up4_rpw up3_fused up5 fir_img2
//                                                   print the plan of one call under those five switches (-1: not set):
//                                                   main ksplit reduce tail fir_sums pre_image main_img (tests/test_modconv_cases_cpu.py)
// Exit status 1 and a line on stderr for every plan that does not fit.
#include <stdio.h>
#include <string.h>

#include "p3d_conv_plan.hpp"

static const char* kernel_name(ConvKernel k) {
    static const char* const names[] = {"k_modconv<0>", "k_modconv<1>", "k_modconv_h<0,false>", "k_modconv_h<0,true>", "k_modconv_h<1,false>",
                                        "k_modconv_h<1,true>", "k_modconv_w2<false>", "k_modconv_w2<true>", "k_modconv_w3<false>",
                                        "k_modconv_w3<true>", "k_modconv_up", "k_modconv_up_h<false>", "k_modconv_up_h<true>",
                                        "k_modconv_up3<false>", "k_modconv_up3<true>", "k_modconv_up5", "k_modconv_up4<8,2,3>",
                                        "k_modconv_up4<4,2,2>"};
    return names[(int)k];
}
static const char* reduce_name(ConvReduce r) {
    static const char* const names[] = {"-", "k_splitk_reduce", "k_splitk_reduce_img"};
    return names[(int)r];
}
static const char* tail_name(ConvTail t) {
    static const char* const names[] = {"-", "k_act_to_image", "k_fir4x4_tiled", "k_fir4x4_img<false,4,2>", "k_fir4x4_img<true,2,3>",
                                        "k_fir4x4_img2<8>", "k_fir4x4_img2<32>"};
    return names[(int)t];
}

static const ConvSwitches kDefault = {-1, -1, -1, -1, -1};
static const ConvSwitches kForced[] = {
    kDefault, {0, -1, -1, -1, -1}, {1, -1, -1, -1, -1}, {1, 0, -1, -1, -1}, {1, 2, -1, -1, -1}, {0, -1, 0, -1, -1}, {0, -1, 1, -1, -1},
    {0, -1, 0, 0, -1}, {0, -1, 0, 1, -1}, {0, -1, 0, -1, 0}, {0, -1, 0, -1, 8}, {0, -1, 0, -1, 32}, {-1, -1, -1, 1, 32}};

static int sweep(int N, int I, int O, int H, int W, int up) {
    const size_t budget = p3d_conv_workspace_bytes(N, I, O, H, W, up);
    int bad = 0, plans = 0;
    for (int ks = 1; ks <= 3; ks += 2) {
        if (ks == 1 && up != 1) continue;
        for (int mma = 0; mma < 3; ++mma) {
            if (mma != P3D_CONV_MMA_F32 && I % 16 != 0) continue;  // (refused by p3d_modconv2d_ex_f32)
            for (int x_img = 0; x_img < 2; ++x_img) {
                if (x_img && (mma != P3D_CONV_MMA_F16X2 || ks != 3 || !conv_takes_image(I, O, W, up))) continue;
                for (int out = 0; out < 4; ++out) {  // y, y_img, both (up = 1), the ToRGB ride
                    const bool y_img = out == 1 || out == 2, rgb = out == 3;
                    if ((y_img && O % 8 != 0) || (out == 2 && up != 1)) continue;
                    if (rgb && !(up == 1 && x_img && conv_rgb_fusable(N, I, O, H, W, 3))) continue;
                    for (int a = 0; a < 3; ++a) {
                        const ConvCall c = {N, I, O, H, W, ks, up, mma, x_img != 0, y_img, rgb, a ? 1 : 0, a == 2 ? 2.0f : 0.2f};
                        for (const ConvSwitches& s : kForced) {
                            const ConvPlan pl = p3d_conv_plan(c, s);
                            ++plans;
                            const bool ok = pl.end <= budget && pl.ksplit >= 1 && pl.ksplit <= 64 && pl.grid.x && pl.grid.y && pl.grid.z &&
                                            (pl.tail == ConvTail::NONE || (pl.tail_grid.x && pl.tail_grid.y)) && !(pl.pre_image && c.x_img) &&
                                            (!rgb || pl.main == ConvKernel::W3_RGB);
                            if (!ok) {
                                fprintf(stderr, "bad plan: N %d I %d O %d H %d W %d ks %d up %d mma %d x_img %d out %d act %d: %s end %zu budget %zu\n",
                                        N, I, O, H, W, ks, up, mma, x_img, out, a, kernel_name(pl.main), pl.end, budget);
                                bad = 1;
                            }
                        }
                    }
                }
            }
        }
    }
    printf("s %d\n", plans);
    return bad;
}

int main() {
    char kind[4];
    int bad = 0;
    while (scanf("%3s", kind) == 1) {
        if (!strcmp(kind, "s")) {
            int N, I, O, H, W, up;
            if (scanf("%d %d %d %d %d %d", &N, &I, &O, &H, &W, &up) != 6) return 2;
            bad |= sweep(N, I, O, H, W, up);
        } else if (!strcmp(kind, "q")) {
            ConvCall c;
            ConvSwitches s;
            int x_img, y_img, rgb;
            if (scanf("%d %d %d %d %d %d %d %d %d %d %d %d %f %d %d %d %d %d", &c.N, &c.I, &c.O, &c.H, &c.W, &c.ks, &c.up, &c.mma, &x_img, &y_img,
                      &rgb, &c.act, &c.alpha, &s.up4, &s.up4_rpw, &s.up3_fused, &s.up5, &s.fir_img2) != 18)
                return 2;
            c.x_img = x_img; c.y_img = y_img; c.rgb = rgb;
            const ConvPlan pl = p3d_conv_plan(c, s);
            printf("q %s %d %s %s %d %d %d\n", kernel_name(pl.main), pl.ksplit, reduce_name(pl.reduce), tail_name(pl.tail), (int)pl.fir_sums,
                   (int)pl.pre_image, (int)pl.main_img);
        } else {
            ConvCall c;
            int x_img, y_img, rgb;
            if (scanf("%d %d %d %d %d %d %d %d %d %d %d %d %f", &c.N, &c.I, &c.O, &c.H, &c.W, &c.ks, &c.up, &c.mma, &x_img, &y_img, &rgb,
                      &c.act, &c.alpha) != 13)
                return 2;
            c.x_img = x_img; c.y_img = y_img; c.rgb = rgb;
            const ConvPlan pl = p3d_conv_plan(c, kDefault);
            printf("p %s %d %s %s%s\n", kernel_name(pl.main), pl.ksplit, reduce_name(pl.reduce), tail_name(pl.tail),
                   pl.pre_image ? " (input image first)" : "");
        }
    }
    return bad;
}
