// p3d_rmline_plan.hpp — the host-side plan of one generator layer (include/p3d_rmline.h): which pixel tile a workgroup takes, from the
// LDS its input patch and weights need.  Pure host code: no HIP, compiled into the library and into tests/rmline_plan_host.cpp.
#ifndef P3D_RMLINE_PLAN_HPP
#define P3D_RMLINE_PLAN_HPP
#include <stddef.h>

#include "../../include/p3d_rmline.h"

#define RM_TW 32                    // a tile's columns: two 16-pixel MFMA blocks
#define RM_PW (RM_TW + 2)           // the patch's columns
#define RM_LDS_LIMIT (160 * 1024)   // one workgroup may take the whole CU's LDS

struct RmPlan {
    int plan;     // P3D_RMLINE_TILE_*
    int rows;     // the tile's rows: 8 (two per wave) or 4 (one per wave)
    int ci4;      // Ci rounded up to a multiple of 4: the k-steps of a tap
    int cip;      // LDS pitch of a pixel's / a filter's channels in floats: ci4 + 2 (== 2 mod 4: conflict-free ds_read_b32 of 16 rows)
    int cot;      // output channels per workgroup: 16 or 32
    int cblocks;  // workgroups along Co
    size_t lds;   // bytes
};

static inline size_t rm_lds_bytes(int rows, int cip, int cot) { return sizeof(float) * (size_t)cip * ((size_t)(rows + 2) * RM_PW + 9 * (size_t)cot); }

static inline int rm_conv_plan(int Ci, int Co, int force_plan, RmPlan* p) {
    if (Ci <= 0 || Co <= 0) return P3D_E_ARG;
    if (Ci > P3D_RMLINE_MAX_C || Co > P3D_RMLINE_MAX_C) return P3D_E_RANGE;
    if (force_plan != 0 && force_plan != P3D_RMLINE_TILE_8 && force_plan != P3D_RMLINE_TILE_4) return P3D_E_RANGE;
    p->ci4 = (Ci + 3) / 4 * 4;
    p->cip = p->ci4 + 2;
    p->cot = Co <= 16 ? 16 : 32;
    p->cblocks = (Co + p->cot - 1) / p->cot;
    const bool fits8 = rm_lds_bytes(8, p->cip, p->cot) <= RM_LDS_LIMIT;
    if (force_plan == P3D_RMLINE_TILE_8 && !fits8) return P3D_E_RANGE;
    p->plan = force_plan ? force_plan : (fits8 ? P3D_RMLINE_TILE_8 : P3D_RMLINE_TILE_4);
    p->rows = p->plan == P3D_RMLINE_TILE_8 ? 8 : 4;
    p->lds = rm_lds_bytes(p->rows, p->cip, p->cot);
    return 0;
}
#endif
