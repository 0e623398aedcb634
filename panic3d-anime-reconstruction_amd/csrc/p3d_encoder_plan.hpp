// p3d_encoder_plan.hpp — the host-side plan of the encoder's convolution (include/p3d_encoder.h states the rule): tile shape and
// split-K factor from the layer's sizes alone.  Pure host code: no HIP type, callable without a GPU.
#pragma once
#include <stdint.h>

#include "../../include/p3d_encoder.h"

struct EncPlan {
    int tile;         // P3D_ENC_TILE_64 / P3D_ENC_TILE_32
    int tm;           // output channels per workgroup: 64 / 32
    int split;        // K ranges (launch grid z); 1: the convolution finishes its values itself
    int cps;          // chunks of P3D_ENC_KC per split
    int64_t ptiles;   // ceil(N Ho Wo / 64)
    int ctiles;       // ceil(Co / tm)
    int64_t wgs;      // ptiles * ctiles * split
};

static const int64_t ENC_MAX_ELEMS = (int64_t)1 << 40;

// the sizes p3d_enc_conv_f32 accepts (Ho, Wo are the OUTPUT sizes); 0 or P3D_E_*
static inline int enc_conv_sizes(int N, int Ci, int Co, int Ho, int Wo, int k, int stride) {
    if (N <= 0 || Ci <= 0 || Co <= 0 || Ho <= 0 || Wo <= 0) return P3D_E_ARG;
    if ((k != 1 && k != 3 && k != 7) || (stride != 1 && stride != 2)) return P3D_E_RANGE;
    if ((int64_t)k * k * Ci > 0x7fffffff / 2 || (int64_t)k * k * Ci * Co > 0x7fffffff) return P3D_E_RANGE;
    if ((int64_t)N * Co * Ho >= ENC_MAX_ELEMS / Wo || (int64_t)N * Ho * Wo > 0x7fffffff - 64) return P3D_E_RANGE;
    if ((Co + 31) / 32 > 65535) return P3D_E_RANGE;
    return 0;
}

static inline void enc_split(int chunks, int want, EncPlan* p) {
    if (want > chunks) want = chunks;
    if (want < 1) want = 1;
    int cps = chunks / want;
    if (cps < 1) cps = 1;
    while ((chunks + cps - 1) / cps > P3D_ENC_MAX_SPLIT) ++cps;
    p->cps = cps;
    p->split = (chunks + cps - 1) / cps;
}

static inline int enc_conv_plan(int N, int Ci, int Co, int Ho, int Wo, int k, int stride, int force_plan, EncPlan* p) {
    const int rc = enc_conv_sizes(N, Ci, Co, Ho, Wo, k, stride);
    if (rc) return rc;
    const int64_t P = (int64_t)N * Ho * Wo, pt = (P + 63) / 64;
    const int64_t K = (int64_t)k * k * Ci;
    const int chunks = (int)((K + P3D_ENC_KC - 1) / P3D_ENC_KC);
    const int64_t t64 = (int64_t)((Co + 63) / 64) * pt, t32 = (int64_t)((Co + 31) / 32) * pt;
    int tile, want;
    if (force_plan) {
        tile = force_plan >> 8, want = force_plan & 255;
        if ((tile != P3D_ENC_TILE_64 && tile != P3D_ENC_TILE_32) || want < 1) return P3D_E_RANGE;  // (a negative code has tile < 0)
    } else if (t64 >= P3D_ENC_CUS) {
        tile = P3D_ENC_TILE_64, want = 1;
    } else if (t32 >= P3D_ENC_CUS) {
        tile = P3D_ENC_TILE_32, want = 1;
    } else if (t64 * chunks >= P3D_ENC_CUS) {
        tile = P3D_ENC_TILE_64, want = (int)((P3D_ENC_CUS + t64 - 1) / t64);
    } else {
        tile = P3D_ENC_TILE_32, want = (int)((P3D_ENC_CUS + t32 - 1) / t32);
    }
    p->tile = tile;
    p->tm = tile == P3D_ENC_TILE_64 ? 64 : 32;
    enc_split(chunks, want, p);
    p->ptiles = pt;
    p->ctiles = (Co + p->tm - 1) / p->tm;
    p->wgs = p->ptiles * p->ctiles * p->split;
    return 0;
}

static inline size_t enc_conv_workspace(const EncPlan& p, int N, int Co, int Ho, int Wo) {
    return p.split > 1 ? (size_t)p.split * (size_t)N * Co * Ho * Wo * sizeof(float) : 0;
}
