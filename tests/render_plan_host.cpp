// Host program of tests/test_render_plan.py: the render plan (csrc/p3d_render_plan.hpp) compiled without any device code.
// stdin, one line per request:
//   p N R ray_tile_w Sc Sf flags dumps limits   print the plan of one launch: the instantiation, grid, block, dynamic LDS bytes,
//                                               tile_w, tiles_x, tiles_per_img, ntiles, lds_rows, swz, blocked; or "err CODE"
//   v                                           check the invariants over the sweep below; prints "v <plans checked>"
// Exit status 1 and a line on stderr for every plan that breaks an invariant.
#include <stdio.h>
#include <string.h>

#include "p3d_render_plan.hpp"

static void kernel_name(const RenderPlan& p, char* buf, size_t n) {
    const int F = p.fast ? 1 : 0;
    switch (p.kernel) {
    case RenderKernel::DUMP: snprintf(buf, n, "k_render<%d,1,%d,0,0>", p.nf, F); break;
    case RenderKernel::PLAIN: snprintf(buf, n, "k_render<%d,0,%d,0,0>", p.nf, F); break;
    case RenderKernel::EARLY: snprintf(buf, n, "k_render<%d,0,%d,1,0>", p.nf, F); break;
    case RenderKernel::EARLY_TCG: snprintf(buf, n, "k_render<%d,0,%d,1,1>", p.nf, F); break;
    case RenderKernel::SLOTS2: snprintf(buf, n, "k_render_slots<2,%d,%d,0>", p.nf, F); break;
    case RenderKernel::SLOTS4: snprintf(buf, n, "k_render_slots<4,%d,%d,0>", p.nf, F); break;
    case RenderKernel::SLOTS4_WO: snprintf(buf, n, "k_render_slots<4,%d,1,1>", p.nf); break;
    }
}

static RenderPlan plan(int N, long long R, int rtw, int Sc, int Sf, int flags, int dumps, int limits) {
    p3d_opts o;
    memset(&o, 0, sizeof(o));
    o.Sc = Sc;
    o.Sf = Sf;
    o.flags = flags;
    return p3d_render_plan(N, R, rtw, o, dumps != 0, limits != 0);
}

static int check(const RenderPlan& p, int N, long long R, int rtw, int Sc, int Sf, int flags, int dumps, int limits) {
    if (p.err) return 0;
    const char* bad = nullptr;
    const bool tiled = p.tile_w > 0;
    const long long tiles_y = tiled ? p.tiles_per_img / p.tiles_x : 0;
    const size_t fixed = (size_t)((p.fast ? P3D_LDS_FAST_FLOATS : P3D_LDS_MLP_FLOATS) + 4) * 4;
    if (p.lds_bytes != fixed + (size_t)p.nwaves * p.lds_rows * p.rays_per_wave * 4) bad = "dynamic LDS is not the image + the waves' rows";
    else if (p.lds_bytes * (p.slots == 4 ? 2 : 1) > P3D_RENDER_LDS_CU) bad = "LDS of the workgroups packed per CU exceeds 160 KiB";
    else if (p.block != 64u * p.nwaves || (p.nwaves != 1 && p.nwaves != 2 && p.nwaves != 4)) bad = "block";
    else if ((long long)p.grid * p.nwaves < p.ntiles || (long long)(p.grid - 1) * p.nwaves >= p.ntiles) bad = "grid x waves does not cover ntiles tightly";
    else if (p.ntiles * p.rays_per_wave < (long long)N * R) bad = "tiles do not cover N * R rays";
    else if (p.rays_per_wave * p.slots != 32) bad = "rays per wave";
    else if (tiled && p.tiles_per_img * p.rays_per_wave != R) bad = "screen tiles do not cover the image exactly";
    else if (p.ntiles != p.tiles_per_img * N) bad = "ntiles";
    else if (p.blocked && !(p.slots == 1 && tiled && p.tiles_x % 16 == 0 && tiles_y % 16 == 0 && (p.ntiles / 256) % 8 == 0 &&
                            p.swz * p.nwaves == 256)) bad = "blocked order without whole super-tiles per XCD run";
    else if (p.slots > 1 && (dumps || (flags & P3D_FLAG_NO_PAIR))) bad = "small-launch kernel where it is not allowed";
    else if (p.kernel == RenderKernel::EARLY_TCG && (p.nf != 96 || limits || (flags & P3D_FLAG_DISPARITY))) bad = "TCG where the coarse depths are not the plain spacing";
    if (!bad) return 0;
    fprintf(stderr, "N=%d R=%lld w=%d Sc=%d Sf=%d flags=%d dumps=%d limits=%d: %s\n", N, R, rtw, Sc, Sf, flags, dumps, limits, bad);
    return 1;
}

static long long sweep(int* nbad) {
    static const long long Rs[][3] = {{1, 0, 8}, {31, 0, 8}, {32, 8, 16}, {1000, 0, 40}, {4096, 64, 48}, {8192, 64, 128},
                                      {8200, 40, 100}, {16384, 128, 96}, {36864, 192, 100}, {65536, 256, 250}, {147456, 384, 200},
                                      {262144, 512, 1000}, {1048576, 1024, 1000}};
    static const int Ss[] = {4, 47, 48, 64, 65, 96, 128, 192, 0};
    static const int Fl[] = {P3D_FLAG_FAST_COLOR, P3D_FLAG_NO_PAIR, P3D_FLAG_PAIR16, P3D_FLAG_QUAD8, P3D_FLAG_WEIGHTS_ONLY,
                             P3D_FLAG_NO_EARLY_OUT, P3D_FLAG_DISPARITY};
    long long n = 0;
    for (int N = 1; N <= 4; N *= 2)
        for (const auto& r : Rs)
            for (int w = 0; w < 3; ++w)
                for (int sc = 0; sc < 8; ++sc)
                    for (int sf = 0; sf < 9; ++sf)
                        for (int fm = 0; fm < 128; ++fm)
                            for (int dl = 0; dl < 4; ++dl) {
                                int flags = 0;
                                for (int i = 0; i < 7; ++i) flags |= (fm >> i & 1) ? Fl[i] : 0;
                                const int rtw = (int)r[w], d = dl & 1, l = dl >> 1;
                                const RenderPlan p = plan(N, r[0], rtw, Ss[sc], Ss[sf], flags, d, l);
                                *nbad += check(p, N, r[0], rtw, Ss[sc], Ss[sf], flags, d, l);
                                n += p.err == 0;
                            }
    return n;
}

int main() {
    char line[256];
    int nbad = 0;
    while (fgets(line, sizeof line, stdin)) {
        int N, rtw, Sc, Sf, flags, d, l;
        long long R;
        if (line[0] == 'v') {
            printf("v %lld\n", sweep(&nbad));
        } else if (sscanf(line, "p %d %lld %d %d %d %d %d %d", &N, &R, &rtw, &Sc, &Sf, &flags, &d, &l) == 8) {
            const RenderPlan p = plan(N, R, rtw, Sc, Sf, flags, d, l);
            if (p.err) {
                printf("err %d\n", p.err);
                continue;
            }
            nbad += check(p, N, R, rtw, Sc, Sf, flags, d, l);
            char name[64];
            kernel_name(p, name, sizeof name);
            printf("%s %u %u %zu %d %d %lld %lld %d %d %d\n", name, p.grid, p.block, p.lds_bytes, p.tile_w, p.tiles_x, p.tiles_per_img,
                   p.ntiles, p.lds_rows, p.swz, p.blocked);
        }
    }
    return nbad ? 1 : 0;
}
