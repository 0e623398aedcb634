// p3d_torgb_plan.hpp — which instantiation of k_torgb (p3d_torgb.hip) runs one p3d_torgb_f32 call and in what shape, decided in ONE
// place: the instantiation, the grid and the dynamic LDS.  Host code only (no HIP headers): tests/test_torgb_cases_cpu.py compiles it
// into a plain host program (tests/torgb_plan_host.cpp).
//   p3d_torgb_plan   the plan of one launch: a pure function of (N, I, O, H, W)
#pragma once
#include <stddef.h>

#include "../../include/panic3d_hip.h"

#define TG_KC 64  // input channels per chunk of the A operand (k_torgb)

enum class TorgbKernel {
    PX1,     // k_torgb<1, false>: O <= 32, a wave = 32 pixels x all K, a workgroup = 128 pixels
    KS1,     // k_torgb<1, true>: O <= 32, a workgroup = 32 pixels, its four waves split K
    PX3,     // k_torgb<3, false>: O > 32, the PX shape
    KS3,     // k_torgb<3, true>: O > 32, the KS shape
    MS,      // k_torgb<1, true, true>: O > 32, KS, one workgroup per 32-channel tile (blockIdx.z)
    MS_PRE,  // k_torgb<1, true, true, true>: ... everything requested up front (I <= 8 chunks)
};

struct TorgbPlan {
    int err;             // P3D_OK, or the P3D_E_* code p3d_torgb_f32 returns for this shape (the other fields then mean nothing)
    TorgbKernel kernel;
    unsigned gx, gy, gz; // the grid; 256 threads per workgroup
    size_t lds_bytes;    // dynamic LDS per workgroup: the two A buffers + the styles of this image
};

static inline TorgbPlan p3d_torgb_plan(int N, int I, int O, int H, int W) {
    TorgbPlan pl = {};
    if (N <= 0 || I <= 0 || O <= 0 || H <= 0 || W <= 0) pl.err = P3D_E_ARG;
    else if (O > 96 || I > 1024 || (long long)I * H * W * 4 >= (1ll << 31)) pl.err = P3D_E_RANGE;  // (x of one image behind a 32-bit byte offset)
    if (pl.err) return pl;
    const int HW = H * W, MT = O <= 32 ? 1 : 3;
    // PX shape (a wave = 32 pixels x all K) once the map alone gives >= 512 workgroups of 128 pixels; KS (a workgroup = 32 pixels,
    // waves split K) below that
    const bool ks = (long long)N * ((HW + 127) / 128) < 512;
    // small maps of a 96-channel layer: one workgroup per 32-channel tile while that still leaves the chip underfilled
    const bool ms = ks && MT == 3 && (long long)N * ((HW + 31) / 32) * 3 <= 1024;
    const bool pre = ms && I <= 8 * TG_KC;  // everything requested up front (k_torgb<..., PRE>)
    pl.lds_bytes = (size_t)(2 * TG_KC * 32 * (ms ? 1 : MT) + (pre ? 8 * TG_KC : ((I + 63) / 64) * 64)) * 4;
    pl.gx = (unsigned)(ks ? (HW + 31) / 32 : (HW + 127) / 128);
    pl.gy = (unsigned)N;
    pl.gz = ms ? 3u : 1u;
    // (53 KB at I = 1024, O = 96: inside the default dynamic-LDS limit, no per-device attribute to set)
    if (pl.lds_bytes > 64 * 1024) { pl.err = P3D_E_RANGE; return pl; }
    pl.kernel = MT == 1 ? (ks ? TorgbKernel::KS1 : TorgbKernel::PX1)
              : pre ? TorgbKernel::MS_PRE : ms ? TorgbKernel::MS : ks ? TorgbKernel::KS3 : TorgbKernel::PX3;
    return pl;
}
