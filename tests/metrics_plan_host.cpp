// Host program of tests/test_metrics_cpu.py: the launch plan of the point-to-mesh distance (csrc/p3d_metrics_plan.hpp) compiled without
// any device code.  argv: Q F FLAGS.  Prints "plan QBLOCKS NTILES SLICES TILES_PER_SLICE" and "workspace BOXES PD2 PFACE BYTES", or
// "error CODE".  Exit status 1 and a line on stderr when the plan breaks what k_pm_pairs (csrc/p3d_metrics.hip) relies on: every face in
// exactly one slice and every query in exactly one block, no empty slice, at most P3D_PM_MAX_SLICES slices, the workspace's parts in
// order, 16-byte aligned where float4 is read, and large enough for every slice.
#include <stdio.h>
#include <stdlib.h>

#include "p3d_metrics_plan.hpp"

static int fail(const char* what, long long a, long long b) {
    fprintf(stderr, "plan: %s (%lld, %lld)\n", what, a, b);
    return 1;
}

int main(int argc, char** argv) {
    if (argc != 4) return fail("usage: Q F FLAGS", argc, 0);
    const int64_t Q = atoll(argv[1]), F = atoll(argv[2]);
    const int flags = atoi(argv[3]);
    pm_plan p;
    const int rc = pm_make_plan(Q, F, flags, &p);
    if (rc) {
        printf("error %d\n", rc);
        return 0;
    }
    if (p.slices < 1 || p.slices > P3D_PM_MAX_SLICES) return fail("a bad slice count", p.slices, 0);
    // faces: walk the slices' tile ranges; they must tile [0, ntiles) in order without a gap, and the tiles must tile [0, F)
    int64_t next_tile = 0;
    for (int64_t s = 0; s < p.slices; ++s) {
        const int64_t lo = s * p.tiles_per_slice;
        const int64_t hi = lo + p.tiles_per_slice < p.ntiles ? lo + p.tiles_per_slice : p.ntiles;
        if (lo != next_tile) return fail("a gap or an overlap between slices", s, lo);
        if (hi <= lo) return fail("an empty slice", s, lo);
        next_tile = hi;
    }
    if (next_tile != p.ntiles) return fail("face tiles not covered", next_tile, p.ntiles);
    if ((p.ntiles - 1) * P3D_PM_FACE_TILE >= F || p.ntiles * P3D_PM_FACE_TILE < F) return fail("the tiles do not cover the faces exactly", p.ntiles, F);
    if (Q > 0 && ((p.qblocks - 1) * P3D_PM_QUERY_BLOCK >= Q || p.qblocks * P3D_PM_QUERY_BLOCK < Q)) return fail("the blocks do not cover the queries exactly", p.qblocks, Q);
    if (Q == 0 && p.qblocks != 0) return fail("blocks for no query", p.qblocks, 0);
    const int64_t forced = (flags & P3D_PM_SLICES_MASK) >> P3D_PM_SLICES_SHIFT;
    if (forced && p.slices > forced) return fail("more slices than were forced", p.slices, forced);
    const size_t boxes = pm_ws_boxes(F), samples = pm_ws_samples(F), seed = pm_ws_seed(F), pd2 = pm_ws_pd2(Q, F), pface = pm_ws_pface(Q, F),
                 bytes = pm_ws_bytes(Q, F);
    if (boxes != (size_t)F * 64 || boxes % 16) return fail("records", (long long)boxes, 0);
    if (samples - boxes != (size_t)p.ntiles * PM_BOX_FLOATS * 4 || samples % 16) return fail("boxes", (long long)samples, (long long)boxes);
    if (seed - samples != (size_t)p.ntiles * 64) return fail("sample records", (long long)seed, (long long)samples);
    pm_plan sp;  // the seeding run: the sample records as a mesh
    if (pm_make_plan(Q, p.ntiles, 0, &sp) || sp.slices > P3D_PM_MAX_SLICES) return fail("the seeding run's plan", p.ntiles, 0);
    if (pd2 - seed != (size_t)Q * 4) return fail("seeds", (long long)pd2, (long long)seed);
    if (pface - pd2 < (size_t)sp.slices * (size_t)Q * 4) return fail("the seeding run's partials", (long long)pface, (long long)pd2);
    if (pface - pd2 < (size_t)p.slices * (size_t)Q * 4 || bytes - pface < (size_t)p.slices * (size_t)Q * 4) return fail("partials", (long long)pface, (long long)bytes);
    printf("plan %lld %lld %lld %lld\n", (long long)p.qblocks, (long long)p.ntiles, (long long)p.slices, (long long)p.tiles_per_slice);
    printf("workspace %zu %zu %zu %zu %zu %zu\n", boxes, samples, seed, pd2, pface, bytes);
    return 0;
}
