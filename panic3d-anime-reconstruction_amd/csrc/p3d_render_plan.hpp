// p3d_render_plan.hpp — which kernel runs one render launch (render_impl, p3d_kernels.hip) and in what shape, decided in ONE place:
// the instantiation, the ray tiles, the per-wave LDS rows, the workgroup size, the grid, the dynamic LDS and k_render's XCD tile
// order.  Host code only (no HIP headers): tests/test_render_plan.py compiles it into a plain host program.
//   p3d_render_tcg / p3d_render_occ / p3d_render_slots_occ   per-instantiation rules, shared with the kernels' template defaults
//                                                            and __launch_bounds__
//   p3d_tile_of_block / p3d_tile_screen   k_render's tile order itself, compiled for the host AND the device (the kernel calls them)
//   p3d_render_plan              the plan of one launch: a pure function of its shape and options
//   p3d_render_plan_workspace_bytes   what p3d_render_workspace_bytes answers
//   p3d_render_wide_rows         which of the launch's two draw rows k_render may load as 16-byte pieces (needs the pointers)
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/panic3d_hip.h"
#include "p3d_lds_layout.hpp"

#define P3D_RENDER_WAVES 4           // the widest render workgroup
#define P3D_RENDER_LDS_CU (160 * 1024)  // LDS bytes of a CU

// TCG ("coarse depths from global", see k_render): the default of k_render's TCG parameter — on wherever it can be
constexpr bool p3d_render_tcg(int NF, bool DUMP, bool EARLY) { return NF == 96 && EARLY && !DUMP; }
// waves per SIMD that k_render<NF, ..., TCG>'s registers are held to (__launch_bounds__) and the plan packs its LDS for: one for the
// LDS-resident 96-key instantiations, two for every other
constexpr int p3d_render_occ(int NF, bool TCG) { return (NF >= 96 && !TCG) ? 1 : 2; }
// ... and k_render_slots<SLOTS, NF, FAST>'s: two for the four-slot tolerance-mode ones, one for the others (see that kernel)
constexpr int p3d_render_slots_occ(int SLOTS, bool FAST) { return (SLOTS == 4 && FAST) ? 2 : 1; }

// ---- k_render's tile order: ONE definition for the kernel (p3d_ray_phases.hpp), the plan below, tests/test_tile_order_cpu.py and
// tools/xcd_load_model.py (both through tests/tile_order_host.cpp).  Hardware places block b on XCD b % 8 and nothing moves work
// between XCDs afterwards: the order decides which screen area an XCD's L2 serves and how evenly the uneven tiles (early-outs)
// add up per XCD.  A pure permutation of which wave renders which tile: results are bit-identical under every order.
#if defined(__HIPCC__)
#define P3D_HD __host__ __device__ __forceinline__
#else
#define P3D_HD static inline
#endif

struct P3dTileOrder {
    int swz;      // blocks of one XCD run
    int blocked;  // round 5: a run is one 16 x 16-tile super-tile, XCD x takes element (x + g) % 8 of group g of eight runs
    int pieces;   // round 12: a run is one pw x ph-tile piece; the piece of column c, row r belongs to XCD (xa * c + r + xs * (r / 8)) % 8
    int pw, ph, xa, xs;
};

// The pieces and the rule the plan takes: 2 x 8 tiles (16 x 32 pixels, 4 workgroups of 4 waves), piece (c, r) to XCD (c + r) % 8.
// Of the rules the model (tools/xcd_load_model.py, profiles/r12_xcd_model.txt) finds no worse than the round-5 order on any view of
// its sweep, the one that measured fastest: with a = 1 an XCD's pieces of neighbouring columns are
// diagonal neighbours, so what it holds at a time is a diagonal band of the screen, not scattered pieces.
#ifndef P3D_PIECE_W
#define P3D_PIECE_W 2
#define P3D_PIECE_H 8
#define P3D_XCD_RULE_A 1
#define P3D_XCD_RULE_S 0
#endif

// Turns `t` into the piece order of pw x ph-tile pieces under the rule (xa, xs) if a view of tiles_x x tiles_y tiles, rendered by
// workgroups of nw waves, can take it: whole pieces, a whole number of workgroups per piece, a multiple of 8 piece rows (every
// column then gives every XCD the same number of pieces, and an XCD visits every column), and of the rows an XCD gets as many in
// the inner half of the view as in the outer half (the subject sits in the middle).  Otherwise leaves t alone; returns whether.
static inline bool p3d_piece_order(P3dTileOrder& t, long long tiles_x, long long tiles_y, int nw, int pw, int ph, int xa, int xs) {
    if (pw <= 0 || ph <= 0 || tiles_x <= 0 || tiles_x % pw || tiles_y % ph || (pw * ph) % nw || (tiles_y / ph) % 8) return false;
    const long long PC = tiles_x / pw, PR = tiles_y / ph;
    long long inner[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (long long r = PR / 4; r < PR - PR / 4; ++r)
        for (long long c = 0; c < PC; ++c) ++inner[(xa * c + r + xs * (r / 8)) & 7];
    for (int x = 0; x < 8; ++x)
        if (2 * inner[x] != PC * PR / 8) return false;
    t.pieces = 1;
    t.swz = pw * ph / nw;
    t.pw = pw; t.ph = ph; t.xa = xa; t.xs = xs;
    return true;
}

// the tile of wave `wave` of block b of a grid of nblk blocks of nwaves waves (tiles >= ntiles: the padding of the last block)
P3D_HD long long p3d_tile_of_block(const P3dTileOrder& t, long long nblk, long long b, int nwaves, int wave, int tiles_x,
                                   long long tiles_per_img) {
    const long long swz = t.swz;
    long long bs = b;
    if (t.pieces) {
        // XCD x = b % 8 walks ITS pieces view by view and, inside a view, column by column: in a column it owns one row of every
        // 8 (rows r, r + 8, ...).  The 256 waves an XCD holds at a time cover as many tiles as a super-tile did, in as many tile
        // columns (x-extent) and as many tile rows per column (y-extent in total).  The plan takes this order only where the
        // views divide into whole pieces and every XCD owns the same number of them, so there is no remainder.
        const int x = (int)(b & 7), PC = tiles_x / t.pw, per_img = (int)(tiles_per_img / (t.pw * t.ph)), per_xcd = per_img >> 3;
        const int per_col = per_xcd / PC;  // = piece rows / 8
        const long long slot = b >> 3, k = slot / swz;
        const int n = (int)(k / per_xcd), kk = (int)(k - (long long)n * per_xcd), c = kk / per_col, j = kk - c * per_col;
        const int r = ((x - t.xa * c - t.xs * j) & 7) + 8 * j;
        bs = ((long long)n * per_img + (long long)r * PC + c) * swz + (slot - k * swz);
    } else {
        const long long full = (nblk / (8 * swz)) * (8 * swz);
        if (b < full) {
            const long long slot = b >> 3, x = b & 7;  // slot-th block of XCD x
            // blocked: over its runs an XCD visits every column of super-tiles (the subject sits in the middle columns: a fixed
            // column per XCD would leave the XCDs of the outer columns idle early)
            const long long g = slot / swz, xr = t.blocked ? ((x + g) & 7) : x;
            bs = g * (8 * swz) + xr * swz + (slot % swz);
        }
    }
    return bs * nwaves + wave;
}

struct P3dTileXY { long long n, tx, ty; };  // view, tile column and row on its screen

// where tile `tile` of a tiled launch (tiles_x tiles per screen row) lies
P3D_HD P3dTileXY p3d_tile_screen(const P3dTileOrder& t, long long tile, int tiles_x, long long tiles_per_img) {
    P3dTileXY o;
    o.n = tile / tiles_per_img;
    const long long tl = tile - o.n * tiles_per_img;
    o.ty = tl / tiles_x;
    o.tx = tl - o.ty * tiles_x;
    if (t.pieces) {
        // consecutive tiles fill one piece, row by row, before the next piece starts; the pieces of a view in row-major order
        const long long pc = tl / (t.pw * t.ph);
        const int q = (int)(tl - pc * (t.pw * t.ph)), PC = tiles_x / t.pw;
        o.tx = (pc % PC) * t.pw + (q % t.pw);
        o.ty = (pc / PC) * t.ph + (q / t.pw);
    } else if (t.blocked) {
        // Blocked tile order (round 5): consecutive tiles fill a SUPER-TILE of 16 x 16 tiles (128 x 64 pixels)
        // before the next one starts, and the XCD swizzle above hands an XCD whole super-tiles — so the ~256 waves resident on an
        // XCD march through a compact screen block whose footprint in the three planes (x-extent 1/4, y-extent 1/8 of the image:
        // ~0.3 + 2.1 + 1.0 MB) fits that XCD's 4 MB L2.  Row-major order gave an XCD four full-width tile rows: the whole xz plane
        // (8.4 MB) streamed through every L2 (measured round 4: the 25 MB of planes fetched ~5 x per XCD).
        const long long st = tl >> 8;
        const int q = (int)(tl & 255), SX = tiles_x >> 4;
        o.tx = (st % SX) * 16 + (q & 15);
        o.ty = (st / SX) * 16 + (q >> 4);
    }
    return o;
}

enum class RenderKernel {
    DUMP,       // k_render<NF, true, FAST, false>: every sample decoded, the stages dumped
    PLAIN,      // k_render<NF, false, FAST, false>: every sample decoded (P3D_FLAG_NO_EARLY_OUT)
    EARLY,      // k_render<NF, false, FAST, true, false>: the exact early-outs, coarse depths in LDS
    EARLY_TCG,  // k_render<96, false, FAST, true, true>: the production 96-key kernel (coarse depths recomputed)
    SLOTS2,     // k_render_slots<2, NF, FAST>: small launches, 16 rays x 2 samples per wave
    SLOTS4,     // k_render_slots<4, NF, FAST>: small launches, 8 rays x 4 samples per wave
    SLOTS4_WO,  // k_render_slots<4, NF, true, true>: ... weights only (NF = 48 / 96)
};

struct RenderPlan {
    int err;              // P3D_OK, or the P3D_E_* code the render entry points return for these arguments (nothing else is set)
    RenderKernel kernel;
    int nf;               // the instantiation's fine-depth capacity: 48, 64, 96, or 0 (the generic path)
    bool fast;            // FAST: the final pass in tolerance mode
    int slots;            // samples per wave-step: 1 (k_render), 2 or 4 (k_render_slots)
    int rays_per_wave;    // 32 / slots: the rays of one tile
    int tile_w, tiles_x;  // tile_w > 0: screen tiles over a tile_w-wide image, tiles_x of them per row; 0: runs of rays_per_wave rays
    long long tiles_per_img, ntiles;
    int lds_rows;         // per-wave LDS rows of rays_per_wave floats
    int nwaves;           // waves per workgroup
    unsigned grid, block;
    size_t lds_bytes;     // dynamic LDS per workgroup
    int swz, blocked;     // k_render's XCD tile order as of round 5 (runs of blocks / whole super-tiles); 0 for k_render_slots
    P3dTileOrder order;   // ... and the order the launch runs in: that one, or the balanced pieces where the shape divides into them
    long long decode_steps_full;  // wave-level decode steps with every sample decoded
};

// ---- wide draw rows (k_render; k_render_slots keeps its scalar loads)
// A ray's jitter row is Sc contiguous floats and its u row Sf; each lane half of k_render takes half of a row.  Where every such
// share is whole 16-byte pieces the kernel loads it as pieces, the jitter row in front of the weight copy (p3d_kernels.hip).  The
// launch decides per row, once, and hands the kernel the bits (RenderParams::wide_rows, wave-uniform):
//   no in-kernel draws; the row's base pointer 16-byte aligned; the row's length a multiple of 8 floats (so that the row of every
//   ray, and the second half's share of it, start on a piece); the jitter row also at most 2 * 4 * P3D_WIDE_MAX_PIECES floats, what
//   the kernel holds in registers across the weight copy.
// Otherwise the kernels run the scalar loads.  -DP3D_WIDE_ROWS=0 rebuilds the kernels without the pieces (the A/B of DESIGN.md section 6).
#ifndef P3D_WIDE_ROWS
#define P3D_WIDE_ROWS 1
#endif
#define P3D_WIDE_JITTER 1
#define P3D_WIDE_U 2
#define P3D_WIDE_MAX_PIECES 12  // per half: Sc <= 96
static inline int p3d_render_wide_rows(int rng, const void* jitter, const void* u, int Sc, int Sf) {
#if P3D_WIDE_ROWS
    if (rng) return 0;
    int bits = 0;
    if (jitter && ((uintptr_t)jitter & 15u) == 0 && Sc % 8 == 0 && Sc / 8 <= P3D_WIDE_MAX_PIECES) bits |= P3D_WIDE_JITTER;
    if (u && ((uintptr_t)u & 15u) == 0 && Sf > 0 && Sf % 8 == 0) bits |= P3D_WIDE_U;
    return bits;
#else
    (void)rng; (void)jitter; (void)u; (void)Sc; (void)Sf;
    return 0;
#endif
}

// ---- interior taps (k_render with the early-outs; every other kernel keeps the generic gather set-up)
// triplane_crop masks by position, and k_render's early-outs decode a lane only when its sample is not cropped: a decoded sample
// has |p.x| <= crop_limit and |p.z| <= crop_limit.  Where that keeps all four bilinear taps of the x and of the z axis inside the
// plane, the gather set-up (p3d_decode.hpp, INTERIOR) needs no range test on those axes and one address serves a texel's
// neighbours; only the y axis, which nothing crops, keeps its tests.  The launch decides once, here, from the kernel's own chain
//     q = p * coord_scale;  ix = (q + 1) * half - 0.5          (binary32, no contraction: p3d_tap_offsets)
// evaluated at p = -crop_limit and p = +crop_limit: the nw tap floor(ix) must be >= 0 at the one and the se tap floor(ix) + 1 <= W - 1
// at the other.  With coord_scale > 0 and half > 0 every operation of the chain (a product with a positive constant, a sum with a
// constant, floor) is monotone non-decreasing in p under round-to-nearest, so the two ends bound every |p| <= crop_limit.  That
// is an argument about the operations; tests/test_interior_taps_cpu.py adds a sweep of the chain around both ends and across the
// interval (a sweep, not a proof).  W == H lets the three planes share one chain per axis.
// -DP3D_INTERIOR_TAPS=0 rebuilds the library without the interior form; P3D_FLAG_GENERIC_TAPS switches it off per launch (tests, A/B).
#ifndef P3D_INTERIOR_TAPS
#define P3D_INTERIOR_TAPS 1
#endif
static inline float p3d_tap_coord(float p, float coord_scale, float half) {
    const float q = p * coord_scale;
    const float s = q + 1.0f;
    const float m = s * half;
    return m - 0.5f;
}
static inline bool p3d_render_interior_taps(int H, int W, const p3d_opts& o) {
#if P3D_INTERIOR_TAPS
    if (!(o.flags & P3D_FLAG_CROP) || (o.flags & P3D_FLAG_GENERIC_TAPS)) return false;
    if (!(o.coord_scale > 0.0f) || !(o.crop_limit >= 0.0f) || W != H || W < 2) return false;
    const float half = 0.5f * (float)W;
    const float lo = __builtin_floorf(p3d_tap_coord(-o.crop_limit, o.coord_scale, half));
    const float hi = __builtin_floorf(p3d_tap_coord(o.crop_limit, o.coord_scale, half));
    return lo >= 0.0f && hi + 1.0f <= (float)(W - 1);  // (false for a NaN anywhere)
#else
    (void)H; (void)W; (void)o;
    return false;
#endif
}
// ... and of the kernels the plan can choose, the ones that have the interior form: k_render with the early-outs, except the
// LDS-resident 96-key instantiation (per-ray limits, disparity spacing), whose registers the interior set-up would push from two
// waves per SIMD's worth to one's (227 + 32 accumulation registers; tools/resource_usage.py)
constexpr bool p3d_render_nf_has_interior(int NF, bool TCG) { return NF != 96 || TCG; }
static inline bool p3d_render_plan_has_interior(const RenderPlan& pl) {
    return (pl.kernel == RenderKernel::EARLY && p3d_render_nf_has_interior(pl.nf, false)) || pl.kernel == RenderKernel::EARLY_TCG;
}

static inline size_t p3d_render_plan_workspace_bytes(int N) {
    return 256 + (size_t)(N > 0 ? N : 0) * 8;  // global min / max + decode-step count, then one min / max pair per view
}

static inline RenderPlan p3d_render_plan(int N, int64_t R, int ray_tile_w, const p3d_opts& o, bool has_dumps, bool has_ray_limits) {
    RenderPlan pl = {};
    const int Sc = o.Sc, Sf = o.Sf, flags = o.flags;
    const bool disparity = (flags & P3D_FLAG_DISPARITY) != 0;
    if (N <= 0 || R <= 0) pl.err = P3D_E_ARG;
    else if (Sc < 4 || Sc > P3D_MAX_S || Sf < 0 || Sf > P3D_MAX_S) pl.err = P3D_E_RANGE;
    else if (disparity && has_ray_limits) pl.err = P3D_E_RANGE;  // not with per-ray limits
    if (pl.err) return pl;

    // register-resident fine depths: 48 / 96 exactly (the trainer's and the eval-faithful rates), any other Sf <= 64 padded to 64;
    // the rest sorts in LDS
    pl.nf = (Sf == 48) ? 48 : (Sf == 96 && Sc <= 96) ? 96 : (Sf <= 64 ? 64 : 0);
    pl.fast = (flags & P3D_FLAG_FAST_COLOR) != 0 && Sf > 0;
    const bool tiled = ray_tile_w > 0 && R % ray_tile_w == 0 && ray_tile_w % 8 == 0 && (R / ray_tile_w) % 4 == 0;
    const auto tile = [&](int rpw) {  // k_render: 8 x 4-ray screen tiles; k_render_slots: 4 x (rpw / 4)
        const int tw = rpw == 32 ? 8 : 4;
        pl.rays_per_wave = rpw;
        pl.tile_w = tiled ? ray_tile_w : 0;
        pl.tiles_x = tiled ? ray_tile_w / tw : 0;
        pl.tiles_per_img = tiled ? (long long)pl.tiles_x * (R / ray_tile_w / (rpw / tw)) : (R + rpw - 1) / rpw;
        pl.ntiles = pl.tiles_per_img * N;
    };
    tile(32);

    // small launches: 16 rays x 2 samples per wave (k_render_slots<2, ...>) while its waves still fit in ONE round on the 1024 SIMDs
    // (measured at 48+48: 128^2 rays 0.74 -> 0.49 ms, but 192^2 = 1152 tiles 0.99 -> 1.28 ms: its steps are ~30 % dearer)
    // ... and of those, 8 rays x 4 samples per wave (k_render_slots<4, ...>) where it measured faster (profiles/r04_notes.txt): launches of at
    // most 8192 rays — fewer 16-ray waves than SIMDs: 64^2 x (96+96) 0.80 -> 0.60 ms exact, 0.60 -> 0.45 tolerance — and the
    // tolerance mode at 96+96 (128^2: 0.63 -> 0.57 ms).  NOT the 128^2 exact launches (0.80 -> 0.88 at 96+96, 0.44 -> 0.49 at 48+48):
    // a decode step is ~4k MFMA clocks + ~1.5k VALU instructions of ISSUE, which ONE wave per SIMD already saturates; a second wave
    // per SIMD has nothing to hide and the per-ray work (draws, sort, marcher) is then done by twice as many waves.
    // P3D_FLAG_QUAD8 / P3D_FLAG_PAIR16 force one of the two (tests, A/B timing).  No dumps on this path.
    // Round 5 (profiles/r05_notes.txt): the tolerance-mode quad kernels spill 30 VGPRs instead of 109 (the fold no longer copies its
    // partial sums) and win at every sample count of a 128^2 view (48+48: 0.42 -> 0.325 ms vs 0.354 for the pair kernel; 96+96: 0.559 vs
    // 0.618): the tolerance mode takes the quad kernel for every small launch.  The exact quad kernels are compiled for one wave per
    // SIMD (no spills: 64^2 x (96+96) 0.60 -> 0.50 ms) and stay the choice for <= 8192 rays only.
    // (Decided on the 32-ray tile count, before the small-launch kernels re-tile.)
    const bool small = !has_dumps && !(flags & P3D_FLAG_NO_PAIR) && pl.ntiles <= 512;
    const bool quad = small && !(flags & P3D_FLAG_PAIR16) &&
                      ((flags & P3D_FLAG_QUAD8) || (long long)N * R <= 8192 || (pl.fast && (pl.nf == 96 || pl.nf == 48)));
    // the production 96-key kernel keeps no coarse-depth rows (TCG) and runs two waves per SIMD like the others
    // (for the plain stratified spacing: per-ray limits and disparity spacing keep the LDS-resident 96-key kernel)
    const bool tcg = pl.nf == 96 && !has_dumps && !small && !(flags & P3D_FLAG_NO_EARLY_OUT) && !has_ray_limits && !disparity;

    // per-wave LDS rows: tc (Sc) + wc/cdf/sorted-fine (max(Sc,Sf)) [+ tf (Sf) on the generic path]
    // + two bit rows over the merged list (is-coarse / known-masked) + the known-masked bits of the coarse samples
    pl.lds_rows = Sc + (Sc > Sf ? Sc : Sf) + (pl.nf == 0 ? Sf : 0) + 2 * ((Sc + Sf + 31) >> 5) + ((Sc + 31) >> 5);
    if (tcg) pl.lds_rows = (Sc > Sf ? Sc : Sf) + 2 * ((Sc + Sf + 31) >> 5);
    const size_t lds_fixed = (size_t)((pl.fast ? P3D_LDS_FAST_FLOATS : P3D_LDS_MLP_FLOATS) + 4) * 4;
    const auto lds = [&](int nwaves) { return lds_fixed + (size_t)nwaves * pl.lds_rows * pl.rays_per_wave * 4; };

    int nw = P3D_RENDER_WAVES;
    if (small) {
        pl.slots = quad ? 4 : 2;
        tile(32 / pl.slots);
        // P3D_FLAG_WEIGHTS_ONLY: honoured by the tolerance-mode four-slot kernels at 48 / 96 fine samples (what paste_front's occlusion pass runs)
        const bool wo = quad && pl.fast && (flags & P3D_FLAG_WEIGHTS_ONLY) != 0 && (pl.nf == 48 || pl.nf == 96);
        pl.kernel = wo ? RenderKernel::SLOTS4_WO : quad ? RenderKernel::SLOTS4 : RenderKernel::SLOTS2;
        // workgroups per CU the LDS is packed for: two for the four-slot form, the exact one included (whose registers hold it to one
        // wave per SIMD: p3d_render_slots_occ)
        const size_t wgs = quad ? 2 : 1;
        while (nw > 1 && wgs * lds(nw) > P3D_RENDER_LDS_CU) nw >>= 1;
    } else {
        pl.slots = 1;
        pl.kernel = has_dumps ? RenderKernel::DUMP : (flags & P3D_FLAG_NO_EARLY_OUT) ? RenderKernel::PLAIN
                                                   : tcg ? RenderKernel::EARLY_TCG : RenderKernel::EARLY;
        // small ray counts: shrink the workgroup so that every CU gets work
        while (nw > 1 && pl.ntiles / nw < 2 * 256) nw >>= 1;
        if (nw == P3D_RENDER_WAVES) {
            // large launch: the workgroup shape (4, 2 or 1 waves, as many workgroups as fit) that puts most waves on a CU, at
            // most 4 x occ; ties go to the LARGER workgroup.  48+48: 2 x 4 waves; 64+64: 3 x 2 instead of 1 x 4 (measured
            // 6.85 -> 6.53 ms at 512^2); 96+96: 2 x 4 with the production kernel (TCG), 1 x 4 with the LDS-resident instantiations
            // (measured there: 2 x 2 waves 13.3 ms, 1 x 5 12.6, 1 x 4 11.2)
            const int occ = p3d_render_occ(pl.nf, tcg);
            int best = 0, best_waves = 0;
            for (int w = P3D_RENDER_WAVES; w >= 1; w >>= 1) {
                if (lds(w) > P3D_RENDER_LDS_CU) continue;
                const int fit = (int)(P3D_RENDER_LDS_CU / lds(w)) * w;
                const int waves = fit > 4 * occ ? 4 * occ / w * w : fit;
                if (waves > best_waves) { best_waves = waves; best = w; }
            }
            if (best == 0) { pl.err = P3D_E_RANGE; return pl; }
            nw = best;
        }
        while (nw > 1 && lds(nw) > P3D_RENDER_LDS_CU) nw >>= 1;
        // XCD tile order: runs of swz blocks per XCD (measured: 8..64 within 0.5 %, 1..4 and >= 256 about 1-3 % slower) ...
        pl.swz = 16;
        // ... or whole 16 x 16-tile super-tiles per XCD run when the tile grid divides into them, and into a multiple of 8 of them:
        // 384^2 (18 super-tiles on 8 XCDs) loses 2-3 % to the imbalance, every shape with whole super-tiles per XCD is equal or up
        // to 3 % better (profiles/r05_tile_order_shapes.json)
        const long long tiles_y = tiled ? pl.tiles_per_img / pl.tiles_x : 0;
        if (tiled && pl.tiles_x % 16 == 0 && tiles_y % 16 == 0 && 256 % nw == 0 && (pl.ntiles / 256) % 8 == 0) {
            pl.blocked = 1;
            pl.swz = 256 / nw;
        }
        pl.order.swz = pl.swz;
        pl.order.blocked = pl.blocked;
#ifndef P3D_TILE_ORDER_PARENT  // (the switch rebuilds the round-5 order everywhere: the A/B of DESIGN.md section 6)
        // ... or, round 12, small pieces dealt to the XCDs by a rule of the piece's column and row (p3d_piece_order), where the
        // shape allows: the early-outs make the tiles uneven, nothing moves work between XCDs, and the sums of many small pieces
        // per XCD differ less than the sums of 4 super-tiles (modelled: profiles/r12_xcd_model.txt; measured, the time each XCD's last
        // wave ends: profiles/r12_xcd_finish_*.txt).  Shapes it cannot take (384^2: 96 tile rows are 12 piece rows) keep the above.
        if (pl.blocked) p3d_piece_order(pl.order, pl.tiles_x, tiles_y, nw, P3D_PIECE_W, P3D_PIECE_H, P3D_XCD_RULE_A, P3D_XCD_RULE_S);
#endif
    }
    if (lds(nw) > P3D_RENDER_LDS_CU) { pl.err = P3D_E_RANGE; return pl; }
    pl.nwaves = nw;
    pl.lds_bytes = lds(nw);
    pl.grid = (unsigned)((pl.ntiles + nw - 1) / nw);
    pl.block = 64 * nw;
    const auto steps = [&](int S) { return (long long)((S + pl.slots - 1) / pl.slots); };
    pl.decode_steps_full = pl.ntiles * (Sf > 0 ? steps(Sc) + steps(Sc + Sf) : steps(Sc));
    return pl;
}
