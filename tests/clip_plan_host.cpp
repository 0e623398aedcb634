// Host program of tests/test_clip_cpu.py: the host side of the CLIP unit (csrc/p3d_clip_plan.hpp) compiled without any device code.
//   gemm M K NOUT FORCE      prints "plan TILE SPLIT CPS WGS GRID WORKSPACE", or "error CODE"
//   attn N T HEADS           prints "attn WGS QBLOCKS ROWS LDS", or "error CODE"
//   resize H W S             prints "resize h w offy offx ksy ksx row_lo row_hi", or "error CODE"
//   table IN OUT FIRST COUNT prints one line per output: "xmin n k0 k1 ...", or "error CODE"
// Exit status 1 and a line on stderr when a plan breaks what the kernels (csrc/p3d_clip.hip) rely on: the splits tile the chunks in
// order without an empty one, at most 255 of them; the XCD deal reaches every (column tile, split) slab exactly once; the query blocks
// tile the rows without an empty one; a table row stays inside the source and inside ksize.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "p3d_clip_plan.hpp"

static int fail(const char* what, long long a, long long b) {
    fprintf(stderr, "plan: %s (%lld, %lld)\n", what, a, b);
    return 1;
}

int main(int argc, char** argv) {
    if (argc < 2) return fail("usage", argc, 0);
    if (!strcmp(argv[1], "gemm") && argc == 6) {
        const int M = atoi(argv[2]), K = atoi(argv[3]), Nout = atoi(argv[4]), force = atoi(argv[5]);
        ClipPlan p;
        const int rc = clip_gemm_plan(M, K, Nout, force, &p);
        if (rc) {
            printf("error %d\n", rc);
            return 0;
        }
        const int chunks = (K + P3D_CLIP_KC - 1) / P3D_CLIP_KC;
        if (p.split < 1 || p.split > P3D_CLIP_MAX_SPLIT || p.cps < 1) return fail("a bad split", p.split, p.cps);
        if ((int64_t)(p.split - 1) * p.cps >= chunks || (int64_t)p.split * p.cps < chunks) return fail("the splits do not tile the chunks", p.split, p.cps);
        if (p.tm != (p.tile == P3D_CLIP_TILE_64 ? 64 : 32)) return fail("tile", p.tile, p.tm);
        if ((int64_t)(p.mt - 1) * p.tm >= M || (int64_t)p.mt * p.tm < M) return fail("row tiles", p.mt, M);
        if ((int64_t)(p.nt - 1) * 64 >= Nout || (int64_t)p.nt * 64 < Nout) return fail("column tiles", p.nt, Nout);
        // the deal of k_clip_gemm: id -> (row tile, slab); every pair exactly once
        const int groups = p.nt * p.split;
        std::vector<int> seen((size_t)groups * p.mt, 0);
        for (int64_t id = 0; id < p.grid; ++id) {
            const int64_t place = id >> 3;
            const int mi = (int)(place % p.mt);
            const int64_t g = (place / p.mt) * P3D_CLIP_XCDS + (id & 7);
            if (g >= groups) continue;
            if (seen[(size_t)g * p.mt + mi]++) return fail("a workgroup twice", g, mi);
        }
        for (size_t i = 0; i < seen.size(); ++i)
            if (!seen[i]) return fail("a tile without a workgroup", (long long)i, 0);
        printf("plan %d %d %d %lld %lld %zu\n", p.tile, p.split, p.cps, (long long)p.wgs, (long long)p.grid, clip_gemm_workspace(p, M, Nout));
        return 0;
    }
    if (!strcmp(argv[1], "attn") && argc == 5) {
        const int N = atoi(argv[2]), T = atoi(argv[3]), heads = atoi(argv[4]);
        ClipAttnPlan p;
        const int rc = clip_attn_plan(N, T, heads, &p);
        if (rc) {
            printf("error %d\n", rc);
            return 0;
        }
        if (p.rows < 1 || (p.qblocks - 1) * p.rows >= T || p.qblocks * p.rows < T) return fail("the query blocks do not tile the rows", p.qblocks, p.rows);
        if (p.lds_bytes > 64 * 1024) return fail("LDS", p.lds_bytes, 0);
        printf("attn %lld %d %d %d\n", (long long)p.wgs, p.qblocks, p.rows, p.lds_bytes);
        return 0;
    }
    if (!strcmp(argv[1], "resize") && argc == 5) {
        ClipResize r;
        const int rc = clip_resize_plan(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), &r);
        if (rc) {
            printf("error %d\n", rc);
            return 0;
        }
        if (r.row_lo < 0 || r.row_hi > atoi(argv[2]) || r.offy < 0 || r.offx < 0 || r.offy + atoi(argv[4]) > r.h || r.offx + atoi(argv[4]) > r.w)
            return fail("the crop or the row range leaves the image", r.row_lo, r.row_hi);
        printf("resize %d %d %d %d %d %d %d %d\n", r.h, r.w, r.offy, r.offx, r.ksy, r.ksx, r.row_lo, r.row_hi);
        return 0;
    }
    if (!strcmp(argv[1], "table") && argc == 6) {
        const int in = atoi(argv[2]), out = atoi(argv[3]), first = atoi(argv[4]), count = atoi(argv[5]);
        const int ks = in > 0 && out > 0 ? clip_ksize(in, out) : 1;
        std::vector<int32_t> tab((size_t)(count > 0 ? count : 1) * (2 + ks));
        const int rc = clip_resize_table(in, out, first, count, ks, tab.data());
        if (rc) {
            printf("error %d\n", rc);
            return 0;
        }
        for (int i = 0; i < count; ++i) {
            const int32_t* rec = tab.data() + (size_t)i * (2 + ks);
            if (rec[0] < 0 || rec[1] < 1 || rec[1] > ks || rec[0] + rec[1] > in) return fail("a table row leaves the source", rec[0], rec[1]);
            for (int x = 0; x < 2 + rec[1]; ++x) printf(x ? " %d" : "%d", rec[x]);
            for (int x = rec[1]; x < ks; ++x)
                if (rec[2 + x]) return fail("a coefficient beyond the row's end", i, x);
            printf("\n");
        }
        return 0;
    }
    return fail("usage", argc, 1);
}
