// p3d_rmline_grad_plan.hpp — the host-side plan of a weight gradient of the illustration-to-render module
// (include/p3d_rmline_grad.h): into how many slices the patches are split, which patches a slice takes, and what the kernel needs in LDS
// and workspace.  Pure host code: no HIP, compiled into the library and into tests/rmline_grad_plan_host.cpp.
#ifndef P3D_RMLINE_GRAD_PLAN_HPP
#define P3D_RMLINE_GRAD_PLAN_HPP
#include <stddef.h>
#include <stdint.h>

#include "../../include/p3d_rmline_grad.h"
#include "p3d_rmline_plan.hpp"

#define RM_WG_ROWS 8  // a weight-gradient tile: 8 x RM_TW output pixels, its input patch 10 x RM_PW

struct RmWgradPlan {
    int slices;    // workgroups of the first launch
    int ci16, co16;  // Ci, Co rounded up to 16: the LDS pitch of a pixel's channels
    int nci, nco;  // 16-channel blocks: a wave owns (ci block, co block) pairs, nine taps (and the bias) each
    int sets;      // pairs a wave holds accumulators for: 1 (at most 4 pairs) or 4
    size_t lds;    // bytes
    int64_t ws_floats;  // slices (9 Ci Co + 2 Co): the bias partial is a (sum, correction) pair
};

static inline int rm_wgrad_plan(int N, int Ci, int Co, int force_slices, RmWgradPlan* p) {
    if (N <= 0 || Ci <= 0 || Co <= 0) return P3D_E_ARG;
    if (Ci > P3D_RMLINE_MAX_C || Co > P3D_RMLINE_MAX_C || N > 65535) return P3D_E_RANGE;
    const int most = N < P3D_RMLINE_WG_MAX_SLICES ? N : P3D_RMLINE_WG_MAX_SLICES;
    if (force_slices < 0 || force_slices > most) return P3D_E_RANGE;
    p->slices = force_slices ? force_slices : most;
    p->ci16 = (Ci + 15) / 16 * 16, p->co16 = (Co + 15) / 16 * 16;
    p->nci = p->ci16 / 16, p->nco = p->co16 / 16;
    p->sets = p->nci * p->nco <= 4 ? 1 : 4;
    p->lds = sizeof(float) * ((size_t)(RM_WG_ROWS + 2) * RM_PW * p->ci16 + (size_t)RM_WG_ROWS * RM_TW * p->co16);
    if (p->lds > RM_LDS_LIMIT) return P3D_E_RANGE;  // (not reached for Ci, Co <= 64: 152 576 bytes)
    p->ws_floats = (int64_t)p->slices * (9 * (int64_t)Ci * Co + 2 * Co);
    return 0;
}

#ifdef __HIPCC__
#define RM_HOST_DEVICE __host__ __device__
#else
#define RM_HOST_DEVICE
#endif
// the patches [lo, hi) of slice s: consecutive, every patch in exactly one slice, none empty for slices <= N (the kernel calls this too)
RM_HOST_DEVICE static inline void rm_wgrad_slice(int s, int slices, int N, int* lo, int* hi) {
    *lo = (int)((int64_t)s * N / slices);
    *hi = (int)((int64_t)(s + 1) * N / slices);
}
#endif
