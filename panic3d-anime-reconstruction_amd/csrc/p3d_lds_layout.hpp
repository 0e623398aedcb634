// p3d_lds_layout.hpp — the decoder parameters' LDS image (p3d_decode.hpp loads it, every decoding kernel reads it) as offsets in
// floats.  Host code only (no HIP headers): the launch plans size their dynamic LDS from it (p3d_render_plan.hpp).
#pragma once

// LDS image of the decoder parameters (per workgroup), in MFMA operand order:
//   W0A [2][4][64][4] : tile t, s4, lane l, e  -> w0[32t + (l&31)][16(l>>5) + 4*s4 + e]
//   W1A [2][4][64][4] : tile t, s4, lane l, e  -> w1[1 + (l&31)][nlo(t, 4*s4+e) + 4(l>>5)]
//   B0P [2][2][16]    : half h, tile t, reg r  -> b0[32t + rowof(r) + 4h]
//   B1P [2][16]       : half h, reg r          -> b1[1 + rowof(r) + 4h]
//   W1S [2][32]       : half h, (t,s)          -> w1[0][nlo(t,s) + 4h]
//   B1S [4]           : b1[0], 0, 0, 0
// with rowof(r) = (r&3) + 8(r>>2) and nlo(t,s) = 32t + rowof(s).
#define P3D_LDS_W0A 0
#define P3D_LDS_W1A 2048
#define P3D_LDS_B0P 4096
#define P3D_LDS_B1P 4160
#define P3D_LDS_W1S 4192
#define P3D_LDS_B1S 4256
#define P3D_LDS_MLP_FLOATS 4260

// tolerance mode of the final pass (P3D_FLAG_FAST_COLOR; p3d_decode.hpp):
// Extra LDS image (only in the FAST kernels), in MFMA operand order, 16 B per lane:
//   W0H [2 t][2 q][2 hi/lo][64 lanes][8 f16] : w0[32t + (l&31)][16(l>>5) + 8q + i]
//   W1H [2 t][2 pp][2 hi/lo][64 lanes][8 f16]: w1[1 + (l&31)][32t + rowof(8pp + i) + 4(l>>5)]   (overlays W1A: the f32
//                                               colour weights are never used by a FAST kernel)
#define P3D_LDS_W0H P3D_LDS_MLP_FLOATS
#define P3D_LDS_W1H P3D_LDS_W1A
#define P3D_LDS_FAST_FLOATS (P3D_LDS_MLP_FLOATS + 2048)
