// p3d_clip_plan.hpp — the host side of the CLIP unit (include/p3d_clip.h states the rules): the GEMM's tile and split-K factor, the
// attention's query blocks, and the coefficient tables of PIL's 8-bit bicubic resize.  Pure host code: no HIP type, callable without
// a GPU.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/p3d_clip.h"

struct ClipPlan {
    int tile;      // P3D_CLIP_TILE_64 / P3D_CLIP_TILE_32
    int tm;        // rows per workgroup: 64 / 32
    int split;     // K ranges; 1: the GEMM finishes its values itself
    int cps;       // chunks of P3D_CLIP_KC per split
    int mt, nt;    // ceil(M / tm), ceil(Nout / 64)
    int64_t wgs;   // mt * nt * split: the workgroups that work
    int64_t grid;  // the launch: mt * 8 * ceil(nt * split / 8) (the XCD deal rounds the slab count up to a multiple of 8)
};

static inline int clip_gemm_sizes(int M, int K, int Nout) {
    if (M <= 0 || K <= 0 || Nout <= 0) return P3D_E_ARG;
    const int64_t lim = 0x7fffffff;
    if ((int64_t)M * K >= lim || (int64_t)M * Nout >= lim || (int64_t)K * Nout >= lim) return P3D_E_RANGE;
    return 0;
}

static inline int clip_gemm_plan(int M, int K, int Nout, int force_plan, ClipPlan* p) {
    const int rc = clip_gemm_sizes(M, K, Nout);
    if (rc) return rc;
    const int chunks = (K + P3D_CLIP_KC - 1) / P3D_CLIP_KC;
    const int64_t nt = (Nout + 63) / 64;
    const int64_t t64 = (int64_t)((M + 63) / 64) * nt, t32 = (int64_t)((M + 31) / 32) * nt;
    int tile, want;
    if (force_plan) {
        tile = force_plan >> 8, want = force_plan & 255;
        if ((tile != P3D_CLIP_TILE_64 && tile != P3D_CLIP_TILE_32) || want < 1) return P3D_E_RANGE;  // (a negative code has tile < 0)
    } else if (t64 >= P3D_CLIP_CUS) {
        tile = P3D_CLIP_TILE_64, want = 1;
    } else if (t32 >= P3D_CLIP_CUS) {
        tile = P3D_CLIP_TILE_32, want = 1;
    } else if (t64 * chunks >= P3D_CLIP_CUS) {
        tile = P3D_CLIP_TILE_64, want = (int)((P3D_CLIP_CUS + t64 - 1) / t64);
    } else {
        tile = P3D_CLIP_TILE_32, want = (int)((P3D_CLIP_CUS + t32 - 1) / t32);
    }
    if (want > chunks) want = chunks;
    int cps = chunks / want;
    if (cps < 1) cps = 1;
    while ((chunks + cps - 1) / cps > P3D_CLIP_MAX_SPLIT) ++cps;
    p->tile = tile;
    p->tm = tile == P3D_CLIP_TILE_64 ? 64 : 32;
    p->cps = cps;
    p->split = (chunks + cps - 1) / cps;
    p->mt = (M + p->tm - 1) / p->tm;
    p->nt = (int)nt;
    p->wgs = (int64_t)p->mt * nt * p->split;
    p->grid = (int64_t)p->mt * P3D_CLIP_XCDS * ((nt * p->split + P3D_CLIP_XCDS - 1) / P3D_CLIP_XCDS);
    if (p->grid > 0x7fffffff) return P3D_E_RANGE;
    return 0;
}

static inline size_t clip_gemm_workspace(const ClipPlan& p, int M, int Nout) {
    return p.split > 1 ? (size_t)p.split * (size_t)M * Nout * sizeof(float) : 0;
}

// ---- attention ----------------------------------------------------------------------------------------------------------------------
struct ClipAttnPlan {
    int qblocks, rows;
    int64_t wgs;
    int lds_bytes;
};

static inline int clip_attn_plan(int N, int T, int heads, ClipAttnPlan* p) {
    if (N <= 0 || T <= 0 || heads <= 0) return P3D_E_ARG;
    if (T > P3D_CLIP_MAX_T || heads > 1024 || (int64_t)N * heads > 0x7fffffff / 64 || (int64_t)N * T * heads * 64 * 3 >= 0x7fffffff) return P3D_E_RANGE;
    const int64_t heads_all = (int64_t)N * heads;
    int64_t qb = (P3D_CLIP_CUS + heads_all - 1) / heads_all;
    if (qb > (T + 3) / 4) qb = (T + 3) / 4;
    p->rows = (int)(T / qb) > 0 ? (int)(T / qb) : 1;
    p->qblocks = (T + p->rows - 1) / p->rows;  // (>= qb, and no empty block)
    p->wgs = heads_all * p->qblocks;
    // what k_clip_attention reserves (statically, for T = 64): Q, K at a pitch of 65, V, and one row of probabilities per wave
    p->lds_bytes = (int)sizeof(float) * (P3D_CLIP_MAX_T * (64 + 65 + 64) + 4 * 64);
    return 0;
}

// ---- PIL's bicubic resize -----------------------------------------------------------------------------------------------------------
struct ClipResize {
    int h, w, offy, offx, ksy, ksx, row_lo, row_hi;
};

static inline double clip_cubic(double t) {
    const double a = -0.5;
    if (t < 0.0) t = -t;
    if (t < 1.0) return ((a + 2.0) * t - (a + 3.0)) * t * t + 1.0;
    if (t < 2.0) return (((t - 5.0) * t + 8.0) * t - 4.0) * a;
    return 0.0;
}

static inline int clip_ksize(int in, int out) {
    double fs = (double)in / (double)out;
    if (fs < 1.0) fs = 1.0;
    return (int)ceil(2.0 * fs) * 2 + 1;
}

// the source range of output xx: [*xmin, *xmin + *n)
static inline void clip_bounds(int in, int out, int xx, int* xmin, int* n, double* center, double* fs_out) {
    const double scale = (double)in / (double)out;
    const double fs = scale < 1.0 ? 1.0 : scale, support = 2.0 * fs;
    const double c = (xx + 0.5) * scale;
    int lo = (int)(c - support + 0.5), hi = (int)(c + support + 0.5);
    if (lo < 0) lo = 0;
    if (hi > in) hi = in;
    *xmin = lo, *n = hi - lo, *center = c, *fs_out = fs;
}

static inline int clip_resize_table(int in, int out, int first, int count, int ksize, int32_t* tab) {
    if (!tab || in <= 0 || out <= 0 || count <= 0) return P3D_E_ARG;
    if (in > P3D_CLIP_MAX_SIDE || out > 4 * P3D_CLIP_MAX_SIDE || first < 0 || first > out - count || ksize != clip_ksize(in, out)) return P3D_E_RANGE;
    for (int i = 0; i < count; ++i) {
        int32_t* rec = tab + (size_t)i * (2 + ksize);
        int xmin, n;
        double center, fs;
        clip_bounds(in, out, first + i, &xmin, &n, &center, &fs);
        if (n > ksize) return P3D_E_RANGE;  // (cannot happen: ksize covers 2 support + 1)
        double w[64 * 1024 / 8];            // (ksize <= 2 ceil(2 * 16384) + 1 would not fit: refused below)
        if (ksize > (int)(sizeof(w) / sizeof(w[0]))) return P3D_E_RANGE;
        double ww = 0.0;
        for (int x = 0; x < n; ++x) {
            w[x] = clip_cubic((x + xmin - center + 0.5) * (1.0 / fs));
            ww += w[x];
        }
        rec[0] = xmin, rec[1] = n;
        for (int x = 0; x < ksize; ++x) {
            double v = x < n ? w[x] : 0.0;
            if (x < n && ww != 0.0) v /= ww;
            rec[2 + x] = v < 0.0 ? (int32_t)(-0.5 + v * (double)(1 << 22)) : (int32_t)(0.5 + v * (double)(1 << 22));
        }
    }
    return 0;
}

// int(round(d / 2.0)) for d >= 0 with Python's round (half to even)
static inline int clip_half_even(int d) {
    const int half = d / 2;
    return (d & 1) ? half + (half & 1) : half;
}

static inline int clip_resize_plan(int H, int W, int S, ClipResize* r) {
    if (H <= 0 || W <= 0 || S <= 0) return P3D_E_ARG;
    if (H > P3D_CLIP_MAX_SIDE || W > P3D_CLIP_MAX_SIDE || S > P3D_CLIP_MAX_S) return P3D_E_RANGE;
    if (W <= H) r->w = S, r->h = (int)((double)((int64_t)S * H) / (double)W);
    else r->h = S, r->w = (int)((double)((int64_t)S * W) / (double)H);
    if (r->h > 4 * P3D_CLIP_MAX_SIDE || r->w > 4 * P3D_CLIP_MAX_SIDE) return P3D_E_RANGE;
    r->offy = clip_half_even(r->h - S), r->offx = clip_half_even(r->w - S);
    r->ksy = clip_ksize(H, r->h), r->ksx = clip_ksize(W, r->w);
    if (r->ksy > 8192 || r->ksx > 8192) return P3D_E_RANGE;
    int lo = H, hi = 0;
    for (int i = 0; i < S; ++i) {
        int ymin, n;
        double c, fs;
        clip_bounds(H, r->h, r->offy + i, &ymin, &n, &c, &fs);
        if (ymin < lo) lo = ymin;
        if (ymin + n > hi) hi = ymin + n;
    }
    r->row_lo = lo, r->row_hi = hi;
    return hi > lo ? 0 : P3D_E_RANGE;
}

static inline size_t clip_prepare_workspace(int N, const ClipResize& r, int S) {
    return (size_t)N * 3 * (size_t)(r.row_hi - r.row_lo) * S;
}

// ---- PSNR ---------------------------------------------------------------------------------------------------------------------------
static inline int clip_psnr_blocks(int64_t count) {
    const int64_t b = (count + 4095) / 4096;
    return (int)(b > 1024 ? 1024 : (b < 1 ? 1 : b));
}
