// Host program of tests/test_tile_order_cpu.py and tools/xcd_load_model.py: k_render's tile order (p3d_tile_of_block and
// p3d_tile_screen of csrc/p3d_render_plan.hpp, the very functions the kernel calls) evaluated without any device code.
// stdin, one line per request:
//   m N R ray_tile_w Sc Sf flags nw parent pw ph xa xs
//       nw      0: the plan's workgroup size; 1 / 2 / 4: that many waves per workgroup instead (the grid and the run length follow)
//       parent  1: the round-5 order (what -DP3D_TILE_ORDER_PARENT builds launch)
//       pw, ph, xa, xs  pw > 0: pieces of pw x ph tiles dealt by the rule (xa, xs) instead of the plan's choice, if the shape can
//               take them (p3d_piece_order)
// stdout: "order <swz> <blocked> <pieces> <pw> <ph> <xa> <xs> <nwaves> <grid> <tiles_x> <tiles_per_img> <ntiles>" (or "err CODE"), then one line
// per wave of the grid, "<block> <wave> <tile> <view> <tx> <ty>" (view, tx, ty = -1 for the padding tiles >= ntiles and for an
// untiled launch).
#include <stdio.h>
#include <string.h>

#include "p3d_render_plan.hpp"

int main() {
    char line[256];
    while (fgets(line, sizeof line, stdin)) {
        int N, rtw, Sc, Sf, flags, nw, parent, pw, ph, xa, xs;
        long long R;
        if (sscanf(line, "m %d %lld %d %d %d %d %d %d %d %d %d %d", &N, &R, &rtw, &Sc, &Sf, &flags, &nw, &parent, &pw, &ph, &xa, &xs) != 12)
            continue;
        p3d_opts o;
        memset(&o, 0, sizeof(o));
        o.Sc = Sc;
        o.Sf = Sf;
        o.flags = flags;
        const RenderPlan pl = p3d_render_plan(N, R, rtw, o, false, false);
        if (pl.err || pl.slots != 1) {
            printf("err %d\n", pl.err ? pl.err : -100);
            continue;
        }
        const int nwaves = nw ? nw : pl.nwaves;
        P3dTileOrder t = pl.order;
        if (parent || pw > 0) {
            memset(&t, 0, sizeof(t));
            t.swz = pl.swz;
            t.blocked = pl.blocked;
        }
        t.swz = t.swz * pl.nwaves / nwaves;  // a run keeps its tiles: a piece, a super-tile, or 16 of the plan's workgroups
        if (!parent && pw > 0 && pl.tile_w > 0) p3d_piece_order(t, pl.tiles_x, pl.tiles_per_img / pl.tiles_x, nwaves, pw, ph, xa, xs);
        const long long grid = (pl.ntiles + nwaves - 1) / nwaves;
        printf("order %d %d %d %d %d %d %d %d %lld %d %lld %lld\n", t.swz, t.blocked, t.pieces, t.pw, t.ph, t.xa, t.xs, nwaves, grid,
               pl.tiles_x, pl.tiles_per_img, pl.ntiles);
        for (long long b = 0; b < grid; ++b)
            for (int w = 0; w < nwaves; ++w) {
                const long long tile = p3d_tile_of_block(t, grid, b, nwaves, w, pl.tiles_x, pl.tiles_per_img);
                P3dTileXY s = {-1, -1, -1};
                if (pl.tile_w > 0 && tile < pl.ntiles) s = p3d_tile_screen(t, tile, pl.tiles_x, pl.tiles_per_img);
                printf("%lld %d %lld %lld %lld %lld\n", b, w, tile, s.n, s.tx, s.ty);
            }
    }
    return 0;
}
