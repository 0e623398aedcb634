// p3d_metrics_plan.hpp — how the (query, face) pair loop of the point-to-mesh distance (k_pm_pairs, p3d_metrics.hip) is cut into
// workgroups, decided in ONE place: query blocks x face slices, and the workspace's layout.  Host code only (no HIP headers):
// tests/test_metrics_cpu.py compiles it into a plain host program.
//   pm_make_plan        the launch shape (or a negative P3D_E_*)
//   pm_workspace_*      byte offsets of the workspace's four parts
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/p3d_metrics.h"

#define PM_RECORD_FLOATS 16     // a, b, c, n, n.n, ab.ab, bc.bc, ca.ca
#define PM_BOX_FLOATS 8         // lo, hi, the longest squared edge, one pad
// 10^4 queries are 79 waves: the face loop is sliced until the grid holds about 80 one-wave workgroups per CU on 256 CUs.  Measured at
// 10^4 x 9.7e5 (tools/bench_metrics.py's mesh): 26 slices 39.0 ms, 64 29.8, 128 23.0, 256 22.0 without culling; 14.3, 8.9, 5.7, 4.4 ms
// with it, where short workgroups also even out the waves that skip much and the ones that skip little
#define PM_TARGET_BLOCKS 20480
#define PM_KNOWN_FLAGS (P3D_PM_NO_CULL | P3D_PM_SLICES_MASK)

struct pm_plan {
    int64_t qblocks;          // workgroups along the queries: query q belongs to block q / P3D_PM_QUERY_BLOCK
    int64_t ntiles;           // face tiles: face f belongs to tile f / P3D_PM_FACE_TILE
    int64_t slices;           // workgroups along the faces
    int64_t tiles_per_slice;  // slice s takes tiles [s * tiles_per_slice, min((s + 1) * tiles_per_slice, ntiles))
};

static inline int pm_make_plan(int64_t Q, int64_t F, int flags, pm_plan* p) {
    if (!p || (flags & ~PM_KNOWN_FLAGS) || Q < 0) return P3D_E_ARG;
    if (F < 1 || F > P3D_PM_MAX_F || Q > P3D_PM_MAX_Q) return P3D_E_RANGE;
    const int64_t forced = (flags & P3D_PM_SLICES_MASK) >> P3D_PM_SLICES_SHIFT;
    if (forced > P3D_PM_MAX_SLICES) return P3D_E_RANGE;
    p->qblocks = (Q + P3D_PM_QUERY_BLOCK - 1) / P3D_PM_QUERY_BLOCK;
    p->ntiles = (F + P3D_PM_FACE_TILE - 1) / P3D_PM_FACE_TILE;
    int64_t want = forced;
    if (!want) {
        const int64_t qb = p->qblocks > 0 ? p->qblocks : 1;
        want = (PM_TARGET_BLOCKS + qb - 1) / qb;
        if (want > P3D_PM_MAX_SLICES) want = P3D_PM_MAX_SLICES;
    }
    if (want > p->ntiles) want = p->ntiles;
    p->tiles_per_slice = (p->ntiles + want - 1) / want;
    p->slices = (p->ntiles + p->tiles_per_slice - 1) / p->tiles_per_slice;  // <= want, and no slice is empty
    return 0;
}

// records | boxes | sample records (the first face of every tile) | seed dist2 [Q] | partial dist2 [P3D_PM_MAX_SLICES][Q] |
// partial face [P3D_PM_MAX_SLICES][Q]; the first three are 16-byte multiples
static inline int64_t pm_tiles(int64_t F) { return (F + P3D_PM_FACE_TILE - 1) / P3D_PM_FACE_TILE; }
static inline size_t pm_ws_boxes(int64_t F) { return sizeof(float) * PM_RECORD_FLOATS * (size_t)F; }
static inline size_t pm_ws_samples(int64_t F) { return pm_ws_boxes(F) + sizeof(float) * PM_BOX_FLOATS * (size_t)pm_tiles(F); }
static inline size_t pm_ws_seed(int64_t F) { return pm_ws_samples(F) + sizeof(float) * PM_RECORD_FLOATS * (size_t)pm_tiles(F); }
static inline size_t pm_ws_pd2(int64_t Q, int64_t F) { return pm_ws_seed(F) + sizeof(float) * (size_t)Q; }
static inline size_t pm_ws_pface(int64_t Q, int64_t F) { return pm_ws_pd2(Q, F) + sizeof(float) * P3D_PM_MAX_SLICES * (size_t)Q; }
static inline size_t pm_ws_bytes(int64_t Q, int64_t F) {
    if (Q < 0 || Q > P3D_PM_MAX_Q || F < 1 || F > P3D_PM_MAX_F) return 0;
    return pm_ws_pface(Q, F) + sizeof(int32_t) * P3D_PM_MAX_SLICES * (size_t)Q;
}
