// p3d_kernels.hip — HIP kernels + the C ABI (include/panic3d_hip.h) of libpanic3d_hip.so.  gfx950 only.
//
// Kernels:
//   k_planes_to_nhwc   LDS-tiled transpose of the reference's NCHW planes to channels-last.
//   k_decode_points    run_model on a point cloud (32 points per wavefront, see p3d_decode.hpp).
//   k_render           ImportanceRenderer.forward fused per wavefront: 32 rays per wave (lane pair = ray x channel half);
//                      coarse density pass -> weights -> importance resampling -> merge -> final decode + compositing,
//                      all per-ray state in registers / LDS; no intermediate tensor ever reaches HBM.
//   k_render_slots     the same algorithm for small launches: 32 / SLOTS rays x SLOTS samples per wave, SLOTS = 2 or 4
//                      (bit-identical results).
//   k_render_finish    the one cross-ray dependency: depth clamp to the global [min t, max t] (ray_marcher.py:49-50).
//   k_sigma2density    get_eg3d_volume's activation + crop / cull masks in one pass.
//   k_stratified / k_composite / k_importance / k_unify_perm   operator-level stand-alone stages (one thread per ray).
// The per-ray phases are defined once in p3d_ray_phases.hpp (what the two lane halves share out: p3d_importance.hpp); the render
// kernels here are the order in which a wave goes through them.
// Compile: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (see panic3d-anime-reconstruction_amd/_build.py).
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <type_traits>

#include "p3d_ray_phases.hpp"
#include "p3d_render_plan.hpp"
#include "p3d_cull_band.hpp"
#include "p3d_phase_timing.hpp"

#define P3D_WAVES_PER_WG 4
// Quad-cooperative gathers (p3d_decode.hpp) in every decode of k_render and k_render_slots (measured with the 76-instruction transpose,
// 512^2 x (48+48), canonical / surface ms: tolerance kernel 1.99 / 2.62 -> 1.61 / 2.13 with them in the final AND the coarse pass
// (final only: 1.78 / 2.22); exact kernel 2.32 / 3.33 -> 1.93 / 3.09 (final only 2.09 / 3.16); every sample decoded 3.39 / 5.16).
// Not in the exact point / grid query (density-only decoder: 12.75 vs 12.65 ms at 512^3); yes in the tolerance one (10.2 -> 7.7).
#define P3D_WG (64 * P3D_WAVES_PER_WG)

// =====================================================================================================================
// planes NCHW -> NHWC
// =====================================================================================================================
// grid: (ceil(H*W/64), n3); block 256.  Each block moves a [32 ch][64 px] tile through LDS.
__global__ __launch_bounds__(256) void k_planes_to_nhwc(const float* __restrict__ src, float* __restrict__ dst, int HW) {
    __shared__ float tile[32][65];
    const int p0 = blockIdx.x * 64;
    const size_t img = (size_t)blockIdx.y * 32 * HW;
    {
        int px = threadIdx.x & 63, c0 = threadIdx.x >> 6;  // 4 channels per pass
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            int c = c0 + 4 * k;
            tile[c][px] = (p0 + px < HW) ? src[img + (size_t)c * HW + p0 + px] : 0.0f;
        }
    }
    __syncthreads();
    {
        int c = threadIdx.x & 31, q0 = threadIdx.x >> 5;  // 8 pixels per pass
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            int px = q0 + 8 * k;
            if (p0 + px < HW) dst[img + (size_t)(p0 + px) * 32 + c] = tile[c][px];
        }
    }
}

// =====================================================================================================================
// run_model on a point cloud
// =====================================================================================================================
struct DecodeParams {
    const float* planes;  // [N][3][H][W][32]
    const float* coords;  // [N][M][3]
    const float *w0, *b0, *w1, *b1;
    float* out_sigma;  // [N][M]
    float* out_rgb;    // [N][M][32] or null
    unsigned char* out_cropmask;  // grid mode only: [M] 1 where |x| or |z| > mask_limit (triplane_crop_mask), or null
    float mask_limit;
    long long M;
    long long tiles_per_img;  // ceil(M/32)
    long long ntiles;
    int H, W;
    // coords == nullptr: points of the reference's regular grid (create_samples, _util/eg3d_metrics3d.py:70-92), flat index
    // grid_lo + m: column 2 = idx % n, column 1 = fmod(float(idx) / n, n), column 0 = fmod(float(idx) / n / n, n), each * vsize + goff
    int grid_n;
    long long grid_lo;
    float vsize, goff0, goff1, goff2;
    P3dDecodeCfg cfg;
};

// fmodf(a, b) for finite a >= 0, b > 0 with a / b < 2^24 — exactly C's fmodf there, without its generic exponent loop:
// q = trunc(RN(a/b)) is floor(a/b) or one more (rounding is monotonic and integers are representable); a - q*b is then exactly
// representable (a multiple of ulp(b), magnitude < b), so the fma returns it without rounding and one conditional add fixes q+1.
P3D_DEV float p3d_fmod_pos(float a, float b) {
    const float q = __builtin_truncf(a / b);
    const float r = __builtin_fmaf(-q, b, a);
    return r < 0.0f ? r + b : r;
}

// STAGED (grid mode, density only): every wave-step first tries to park the texel boxes its 32 points touch in LDS and gathers
// the taps from there (p3d_gather_features_staged); tiles whose taps do not fit (a tile that straddles two grid rows) take the
// direct path.  Dynamic LDS: the MLP image + P3D_BOX_FLOATS_PER_WAVE floats per wave.
// FASTD (P3D_FLAG_FAST_COLOR on the grid query): the tolerance-mode decoder (f16 two-term MFMA + hardware transcendentals).
template <bool WANT_RGB, bool STAGED, bool FASTD>
__global__ __launch_bounds__(P3D_WG, 2) void k_decode_points(DecodeParams p) {
    static_assert(!(FASTD && WANT_RGB), "the tolerance-mode point decoder is density-only");
    extern __shared__ __attribute__((aligned(16))) float lds_alloc[];
    // FASTD (density only) needs neither of the fp32 weight images nor the f16 colour weights: the LDS image starts at the biases
    // (P3D_LDS_B0P) and `lds` points that many floats before the allocation, so that every P3D_LDS_* offset still applies
    float* lds = FASTD ? lds_alloc - P3D_LDS_B0P : lds_alloc;
    p3d_load_mlp_to_lds(lds, p.w0, p.b0, p.w1, p.b1, !FASTD, !FASTD);
    if constexpr (FASTD) p3d_load_mlp_f16_to_lds(lds, p.w0, p.w1, false);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 31, h = lane >> 5;
    float* box = lds + (FASTD ? P3D_LDS_FAST_FLOATS : P3D_LDS_MLP_FLOATS) + 4 + (STAGED ? wave * P3D_BOX_FLOATS_PER_WAVE : 0);
    (void)box;
    P3dPlaneGeom g;
    g.halfW = 0.5f * (float)p.W; g.halfH = 0.5f * (float)p.H; g.fW = (float)p.W; g.fH = (float)p.H; g.W = p.W;
    g.plane_bytes = (uint32_t)p.H * (uint32_t)p.W * 128u;
    const long long stride = (long long)gridDim.x * P3D_WAVES_PER_WG;

    // everything a tile needs before its decode: sample position, flags, plane resource
    struct Tile {
        long long n, m;
        bool active, skip, any;
        float px, py, pz;
    };
    auto setup = [&](long long tile, Tile& t) {
        long long n = 0, tl = tile;
        if (p.tiles_per_img != p.ntiles) { n = tile / p.tiles_per_img; tl = tile - n * p.tiles_per_img; }  // uniform; 1 image: no 64-bit division
        t.n = n;
        t.m = tl * 32 + j;
        t.active = t.m < p.M;
        const long long mc = t.active ? t.m : p.M - 1;
        t.skip = false;
        if (p.coords) {
            const float* c = p.coords + ((size_t)n * p.M + mc) * 3;
            t.px = c[0]; t.py = c[1]; t.pz = c[2];
        } else {  // the same float arithmetic as the reference's create_samples (float division: fractional carries are kept)
            // idx < grid_n^3 <= 2^31 (the host checks grid_n <= 1290): 32-bit index arithmetic; (float)idx rounds like torch's
            const unsigned idx = (unsigned)(p.grid_lo + mc);
            const float fn = (float)p.grid_n, f = (float)idx;
            const float s2 = (float)(idx % (unsigned)p.grid_n);
            const float q1 = f / fn;
            const float s1 = p3d_fmod_pos(q1, fn);
            const float s0 = p3d_fmod_pos(q1 / fn, fn);
            t.px = s0 * p.vsize + p.goff0; t.py = s1 * p.vsize + p.goff1; t.pz = s2 * p.vsize + p.goff2;
            if (p.out_cropmask) {
                const bool cropped = __builtin_fabsf(t.px) > p.mask_limit || __builtin_fabsf(t.pz) > p.mask_limit;
                if (t.active && h == 0) p.out_cropmask[t.m] = cropped ? 1 : 0;
                if (p.cfg.flags & P3D_FLAG_SKIP_CROPPED) t.skip = cropped;
            }
        }
        // P3D_FLAG_SKIP_CROPPED (grid mode): a cropped point's density is -1000 whatever the network says
        // (eg3d_metrics3d.py:155-159), so it is not decoded: whole wavefronts are skipped, single lanes fetch nothing
        t.any = __builtin_amdgcn_ballot_w64(t.active && !t.skip) != 0;
    };
    auto resource = [&](long long n) {
        const unsigned nlo = __builtin_amdgcn_readfirstlane((unsigned)n);
        const float* base = p.planes + ((p.cfg.flags & P3D_FLAG_SHARED_PLANES) ? (size_t)0 : (size_t)nlo * 3 * (g.plane_bytes / 4));
        return __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, 3 * g.plane_bytes, 0x00020000);
    };
    auto finish = [&](const Tile& t, float sigma, const f32x16& rgb) {
        if (t.skip) sigma = -1000.0f;
        if (t.active) {
            const size_t o = (size_t)t.n * p.M + t.m;
            if (h == 0) p.out_sigma[o] = sigma;
            if (WANT_RGB) {
                float* dst = p.out_rgb + o * 32 + 4 * h;
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    *(f32x4*)(dst + 8 * q) = (f32x4){rgb[4 * q], rgb[4 * q + 1], rgb[4 * q + 2], rgb[4 * q + 3]};
            }
        }
    };

    // grid-stride over tiles of 32 points; a tile never straddles two images
    long long tile = (long long)blockIdx.x * P3D_WAVES_PER_WG + wave;
    if constexpr (!STAGED) {
        for (; tile < p.ntiles; tile += stride) {
            Tile t;
            setup(tile, t);
            float sigma = -1000.0f;
            f32x16 rgb;
            if (t.any) {
                if constexpr (FASTD) p3d_decode_wave_fast<WANT_RGB, true>(lds, resource(t.n), g, p.cfg, t.px, t.py, t.pz, sigma, rgb, !t.skip);
                else p3d_decode_wave<WANT_RGB>(lds, resource(t.n), g, p.cfg, t.px, t.py, t.pz, sigma, rgb, !t.skip);
            }
            finish(t, sigma, rgb);
        }
    } else {
        // software pipeline: the NEXT tile's texel boxes are being loaded (into registers) while this tile is decoded
        if (tile >= p.ntiles) return;
        Tile cur, nxt;
        P3dStage st;
        setup(tile, cur);
        bool cur_staged = cur.any && p3d_stage_plan(resource(cur.n), g, p.cfg, cur.px, cur.py, cur.pz, st);
        for (;;) {
            P3dBox cb[3] = {st.b[0], st.b[1], st.b[2]};
            if (cur_staged) p3d_stage_commit(box, st);  // waits for the loads issued one iteration ago
            const long long next = tile + stride;
            bool nxt_staged = false;
            if (next < p.ntiles) {
                setup(next, nxt);
                nxt_staged = nxt.any && p3d_stage_plan(resource(nxt.n), g, p.cfg, nxt.px, nxt.py, nxt.pz, st);
            }
            float sigma = -1000.0f;
            f32x16 rgb;
            if (cur.any) {
                if (cur_staged) {
                    const f32x16 X = p3d_gather_features_boxed(box, cb, g, p.cfg, cur.px, cur.py, cur.pz, !cur.skip);
                    if constexpr (FASTD) p3d_decode_features_fast<WANT_RGB>(lds, p.cfg, X, cur.px, cur.pz, sigma, rgb);
                    else p3d_decode_features<WANT_RGB>(lds, p.cfg, X, cur.px, cur.pz, sigma, rgb);
                } else if constexpr (FASTD) {
                    p3d_decode_wave_fast<WANT_RGB>(lds, resource(cur.n), g, p.cfg, cur.px, cur.py, cur.pz, sigma, rgb, !cur.skip);
                } else {
                    p3d_decode_wave<WANT_RGB>(lds, resource(cur.n), g, p.cfg, cur.px, cur.py, cur.pz, sigma, rgb, !cur.skip);
                }
            }
            finish(cur, sigma, rgb);
            if (next >= p.ntiles) break;
            tile = next;
            cur = nxt;
            cur_staged = nxt_staged;
        }
    }
}

// OSGDecoder.forward (training/triplane.py:528-544) on ALREADY SAMPLED features — the module's own call surface, for callers that
// hold `sampled_features` [N][3][M][32] (the reference's renderer hands the decoder exactly that, renderer.py:271-273).  The plane
// mean in the contract's order ((f0 + f1) + f2) * (1/3), then the same MFMA decoder as every other kernel here.  No masks: the
// decoder knows no positions.  HBM-bound: 384 B in, 132 B out per sample.
struct DecodeFeatParams {
    const float* feats;  // [N][3][M][32]
    const float *w0, *b0, *w1, *b1;
    float* out_sigma;    // [N][M]
    float* out_rgb;      // [N][M][32]
    long long M, tiles_per_img, ntiles;
    P3dDecodeCfg cfg;    // flags: P3D_FLAG_FORCE_SIGMOID only
};
__global__ __launch_bounds__(P3D_WG, 2) void k_decode_features(DecodeFeatParams p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    p3d_load_mlp_to_lds(lds, p.w0, p.b0, p.w1, p.b1);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 31, h = lane >> 5;
    const long long stride = (long long)gridDim.x * P3D_WAVES_PER_WG;
    for (long long tile = (long long)blockIdx.x * P3D_WAVES_PER_WG + wave; tile < p.ntiles; tile += stride) {
        const long long n = tile / p.tiles_per_img, m = (tile - n * p.tiles_per_img) * 32 + j;
        const bool active = m < p.M;
        const long long mc = active ? m : p.M - 1;
        f32x16 f[3];
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) {
            const f32x4* src = (const f32x4*)(p.feats + (((size_t)n * 3 + pl) * p.M + mc) * 32 + 16 * h);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const f32x4 v = src[q];
                f[pl][4 * q] = v.x; f[pl][4 * q + 1] = v.y; f[pl][4 * q + 2] = v.z; f[pl][4 * q + 3] = v.w;
            }
        }
        f32x16 X, rgb;
#pragma unroll
        for (int c = 0; c < 16; ++c) X[c] = ((f[0][c] + f[1][c]) + f[2][c]) * P3D_THIRD;  // triplane.py:530 mean(1)
        float sigma;
        p3d_decode_features<true>(lds, p.cfg, X, 0.0f, 0.0f, sigma, rgb);
        if (active) {
            const size_t o = (size_t)n * p.M + m;
            if (h == 0) p.out_sigma[o] = sigma;
            float* dst = p.out_rgb + o * 32 + 4 * h;  // register r holds channel rowof(r) + 4h (p3d_decode.hpp)
#pragma unroll
            for (int q = 0; q < 4; ++q) *(f32x4*)(dst + 8 * q) = (f32x4){rgb[4 * q], rgb[4 * q + 1], rgb[4 * q + 2], rgb[4 * q + 3]};
        }
    }
}

// =====================================================================================================================
// fused ImportanceRenderer.forward
// =====================================================================================================================
// NF: register capacity for the fine depths (sorted by a network); NF == 0: generic path, fine depths sorted in LDS.
//   NF = 48 / 96: Sf == NF exactly (the trainer's 48+48 and the eval-faithful 96+96 of eg3dc_v0.py:30-31): no padding keys, no
//   `i < Sf` predicates (64 uniform predicates held in SGPR pairs were the 102-107 SGPR spills of round 2's NF = 64 kernels);
//   NF = 64: any Sf <= 64, padded with +inf.  Sf in (64, 128] other than 96 takes the LDS path.
//   NF >= 96 is compiled for ONE wave per SIMD (512 registers): its LDS rows (Sc + Sf + bit rows, 26 KB per wave at 96+96) cap a
//   CU at 4-5 waves anyway, and round 2's 128-key variant under the 256-register cap spilled 31-39 VGPRs to scratch.
// DUMP: per-stage dumps (parity tests; disables the early-outs so that every dumped density is a real decode).
//
// Exact early-outs (EARLY = !DUMP && !(flags & P3D_FLAG_NO_EARLY_OUT)), both decided per wavefront:
//   * dead rays: once the binary64 transmittance of a ray is below 1e-60 every later weight alpha * (float)Td is exactly 0
//     (alpha <= 1; Td can grow by at most (1 + 1e-10) per step), so its remaining samples cannot change any output;
//   * cropped samples: triplane_crop masks by POSITION (renderer.py:138-149), so sigma = -1000 is known without a decode.
//   A step whose 32 rays are all dead or cropped skips gather + MLP; in a mixed step the dead / cropped LANES get
//   out-of-bounds gather offsets, i.e. they issue no L1 lookups.
//   In the final pass a skipped sample's colour is needed only if one of its two interval weights is non-zero (sigma of
//   the neighbour >= ~794); that is checked on the exact weights and, if it ever happens, the sample is decoded after
//   all — results are bit-identical by construction.
// the plan (p3d_render_plan.hpp) picks the workgroup size (1, 2 or 4 waves) that fills the CU's 160 KB of LDS best
// FAST (P3D_FLAG_FAST_COLOR): the FINAL pass decodes in tolerance mode (p3d_decode_wave_fast); the coarse pass, and with it
// the importance resampling (inverse-CDF indices, fine depths, merged depth order), stays on the exact contract.
// EARLY: the exact early-outs (compile-time, so that the measurement / dump variant is the plain uniform loop).
// TCG ("coarse depths from global"): the production (EARLY) 96-key kernel keeps NO coarse-depth rows in LDS — Sc + Sf = 192 depth
// rows are 24.5 KB per wave, which capped a CU at 4 waves = ONE per SIMD (round 3: 512^2 x (96+96) every sample decoded took 1.39x
// twice the 48+48 time).  A coarse depth is a pure function of (index, jitter value): t_i = lin_i + jitter[ray][i] * delta, so it is
// recomputed wherever it is needed — streamed in index order in the coarse pass and the merge pre-pass (the jitter row is read
// like the stratified phase reads it), fetched per lane (one 4-byte load from the L2-resident jitter tensor, or the in-kernel
// generator) in the inverse-CDF lerp and in the final walk, where the NEXT coarse depth of every lane is prefetched under the
// current decode.  Rows per wave: max(Sc, Sf) + 12 bit rows = 108 -> 13.8 KB -> 8 waves per CU, two per SIMD, also with the
// tolerance-mode LDS image; the known-masked bits of the coarse samples live in three registers.  With jitter in [0, 1), as
// torch.rand_like produces it, the stratified depths can be out of order only between NEIGHBOURS (rounding), which the sorted
// accessor resolves with two more reads; any other disorder takes an exact O(Sc^2) selection (p3d_coarse_rank, p3d_importance.hpp).
// The draw rows: a ray's jitter row (Sc floats) and u row (Sf) are contiguous, and where the launch says so (RenderParams::wide_rows,
// p3d_render_wide_rows: tensors passed in, aligned, rows of whole pieces) they are read as 16-byte pieces under ONE wave-uniform
// branch per row.  The jitter pieces are requested in front of the weight copy, so their round trip runs under it; half h makes
// the stratified depths [h * Sc/2, (h + 1) * Sc/2) and one exchange joins the halves' flags and extrema (p3d_stratified_combine);
// TCG reads the row one batch of eight ahead of the decodes that use it.  The same operations on the same operands: no result bit
// changes.  Any other launch (in-kernel draws, an unaligned view, Sc % 8 != 0) runs the scalar loads, both halves all depths.
// The final pass merges on the fly (ties: coarse first = stable), decodes and composites [rgb | xyz]: renderer.py:243-259.
// Every lane walks ITS OWN merged list.  With the early-outs on, a lane first consumes — without a decode — every sample
// whose sigma = -1000 is already known (cropped by position, or a coarse sample the coarse pass really decoded and found
// masked) while the previous sample's sigma is <= 602: the interval's softplus argument is then <= -200, rho = alpha = w = 0
// and Td * (double)(1.0f + 1e-10f) = Td, i.e. the marcher update is exactly the identity (include/p3d_numerics.h); only
// prev_t / prev_sigma move.  A dead ray (Td < 1e-60: every later weight is exactly 0) drops all its remaining samples.
// The merge itself runs ONCE, ahead of the walk, as a uniform loop that leaves two bit rows per lane in LDS (merged sample q
// is coarse / is known); the walk then jumps over a whole run of known samples with a count-trailing-ones — consuming them
// one at a time was a chain of two LDS round trips per sample and a quarter of the kernel (profiles/history/r02_notes.txt).
// What is left — the samples that can matter — is decoded one per wave-step until every lane has finished, so a tile of
// rays that miss the subject runs ~Sf/2 steps instead of Sc + Sf.  A consumed sample's colour is fetched after all if one
// of its interval weights turns out non-zero (sigma of a neighbour >= ~794): results are bit-identical by construction.
#define P3D_NF_EXACT(NF) ((NF) == 48 || (NF) == 96)
// TCG is a template parameter of its own (default: on wherever it can be): the plan turns it OFF for the launches whose coarse
// depths are not the plain stratified spacing — per-ray limits (ray_start = 'auto') and disparity spacing — which p3d_stratified_fixed()
// does not know (with TCG derived from (NF, DUMP, EARLY) alone those launches silently rendered the fixed spacing).
// INTERIOR (EARLY only; the launch decides: p3d_render_interior_taps, p3d_render_plan.hpp): the crop keeps every tap of the x and z
// axes inside the planes, and with the early-outs a lane is decoded only when its sample is not cropped — the coarse loops' `live`
// and the walk's `live = have && !known` both exclude a cropped sample — so those decodes set their gathers up in the interior form
// (p3d_decode.hpp).  The guard decodes fetch the colours of consumed samples, cropped ones included: they keep the generic form, as
// does every instantiation without the early-outs.  A template parameter and not a wave-uniform branch: the two set-ups feed the
// fold through different loads, a branch would have to duplicate the fold and the transpose in every decode of the kernel, and the
// instantiation a launch does not take costs it nothing.
template <int NF, bool DUMP, bool FAST, bool EARLY, bool TCG = p3d_render_tcg(NF, DUMP, EARLY), bool INTERIOR = false>
__global__ __launch_bounds__(64 * P3D_RENDER_WAVES, p3d_render_occ(NF, TCG)) void k_render(RenderParams p) {
    static_assert(!(DUMP && EARLY), "dumps need every sample decoded");
    static_assert(!INTERIOR || EARLY, "without the early-outs cropped samples are decoded: the generic gather set-up");
    static_assert(!TCG || p3d_render_tcg(NF, DUMP, EARLY), "TCG exists only for the production 96-key kernel");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    P3D_PHASE_START();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 31, h = lane >> 5;
    const int Sc = p.Sc, Sf = P3D_NF_EXACT(NF) ? NF : p.Sf, S = Sc + Sf;
    constexpr int JP = TCG ? 2 : P3D_WIDE_MAX_PIECES;  // 16-byte pieces of the jitter row a lane holds
#if P3D_WIDE_ROWS
    // ---- tile -> ray, wave set-up, and the jitter row requested: all of it in front of the weight copy, whose barrier every wave
    // waits at with nothing else in flight.  Half h takes the pieces of ITS Sc/2 stratified depths (TCG: both halves the first batch
    // of eight, the coarse loop needs every depth in both).  A wave without a tile sets up the last tile's rays, requests no row and
    // leaves behind the barrier.
    const long long tile = p3d_render_wave_tile(p, wave);
    const bool has_tile = tile < p.ntiles;
    const P3dRayCtx cx = p3d_ray_setup(p, p3d_render_tile_ray(p, has_tile ? tile : p.ntiles - 1, j), Sc, Sf);
    const bool wide_j = has_tile && (p.wide_rows & P3D_WIDE_JITTER) != 0;  // wave-uniform
    const bool wide_u = (p.wide_rows & P3D_WIDE_U) != 0;
    f32x4 jw[JP];
    if (wide_j) p3d_load_row_pieces<JP>(cx.jit + (TCG ? 0 : h * (Sc >> 1)), TCG ? 2 : (Sc >> 3), jw);
    p3d_load_mlp_to_lds(lds, p.w0, p.b0, p.w1, p.b1, !FAST);
    if constexpr (FAST) p3d_load_mlp_f16_to_lds(lds, p.w0, p.w1);
    __syncthreads();
    if (!has_tile) return;  // no workgroup barrier below this line
    P3D_PHASE(P3D_PH_WEIGHTS);
#else
    p3d_load_mlp_to_lds(lds, p.w0, p.b0, p.w1, p.b1, !FAST);
    if constexpr (FAST) p3d_load_mlp_f16_to_lds(lds, p.w0, p.w1);
    __syncthreads();
    // ---- tile -> ray, wave set-up
    const long long tile = p3d_render_wave_tile(p, wave);
    if (tile >= p.ntiles) return;  // no workgroup barrier below this line
    P3D_PHASE(P3D_PH_WEIGHTS);
    const P3dRayCtx cx = p3d_ray_setup(p, p3d_render_tile_ray(p, tile, j), Sc, Sf);
    constexpr bool wide_j = false, wide_u = false;
    f32x4 jw[JP];
#endif
    float* wl = lds + (FAST ? P3D_LDS_FAST_FLOATS : P3D_LDS_MLP_FLOATS) + 4 + (size_t)wave * p.lds_rows * 32;  // per-wave rows, 16-B aligned
    const bool active = cx.active;
    const size_t ray = cx.ray;
    const float ox = cx.ox, oy = cx.oy, oz = cx.oz, dx = cx.dx, dy = cx.dy, dz = cx.dz;
    constexpr bool early = EARLY;
    int ndec = 0;  // decode steps this wave executed (statistics)

    // LDS rows of this wave: row(i)[j]
    float* tcA = wl;             // [Sc]            coarse depths (TCG: no such rows)
    float* wcA = TCG ? wl : tcA + Sc * 32;  // [max(Sc,Sf)]    coarse weights -> pdf/cdf (row 0 = cdf[0]) -> (NF path) sorted fine depths
    float* tfA = (NF > 0) ? wcA : wcA + Sc * 32;  // [Sf] sorted fine depths
    uint32_t* mkA = (uint32_t*)(wl + (size_t)(p.lds_rows - ((Sc + 31) >> 5)) * 32);  // [ceil(Sc/32)] known-masked bits of the coarse samples
    const int nmw = (S + 31) >> 5;                         // words of a bit row over the merged list
    uint32_t* knA = TCG ? (uint32_t*)(wl + (size_t)(Sc > Sf ? Sc : Sf) * 32) : mkA - (size_t)2 * nmw * 32;  // [ceil(S/32)] merged sample q: sigma = -1000 known without a decode
    uint32_t* slA = knA + (size_t)nmw * 32;                // [ceil(S/32)] merged sample q comes from the coarse list
    // TCG knows the fixed spacing only (the host launches a TCG instantiation only for it: fixed ray_start / ray_end, no disparity)
    const P3dSpacing sp = TCG ? p3d_spacing_fixed(p.ray_start, p.ray_end, p.depth_delta, Sc) : p3d_spacing_of(p, ray, Sc);
    auto tc_raw = [&](int i) -> float { return p3d_stratified_fixed(i, Sc, cx.jitter(i), sp); };  // TCG: coarse depth i in DRAW order (bins of the pdf)
    auto tc_of = [&](int i) -> float { if constexpr (TCG) return tc_raw(i); else return tcA[i * 32 + j]; };
    bool wave_unsorted = false;  // TCG: some ray of this wave has two neighbouring stratified depths out of order
    bool bad_order = false;      // TCG: disorder beyond neighbours somewhere in this RAY (jitter outside [0, 1))
    bool wave_bad = false;       //      ... somewhere in this wave
    auto tc_sorted = [&](int i) -> float { return p3d_coarse_rank(tc_raw, i, Sc, wave_unsorted, wave_bad); };
    uint32_t mw0 = 0u, mw1 = 0u, mw2 = 0u;  // TCG: known-masked bits of coarse samples 0-31 / 32-63 / 64-95 (registers, not LDS rows)
    uint32_t fw[3] = {0u, 0u, 0u};  // TCG, RANKS: sorted fine sample k is cropped (sigma = -1000 by position)
    // RANKS: the 48-key kernel with the early-outs runs its merge pre-pass by rank search (p3d_importance.hpp) where the merged list
    // is at most 96 samples (the launch decides: Sc <= 48)
    constexpr bool RANKS = P3D_MERGE_RANKS && EARLY && !TCG && NF == 48;
    const bool dump = DUMP && active && h == 0;

    // ---- stratified depths (TCG: made in the coarse pass, never stored)
    bool unsorted = false;
    float tcmin = __builtin_inff(), tcmax = -__builtin_inff();  // extrema of the coarse depths
    if constexpr (!TCG) {
        float prev = -__builtin_inff();
        if (wide_j) {
            // the pieces requested in front of the weight copy: half h makes the depths [h * Sc/2, (h + 1) * Sc/2) and writes their
            // rows (and dump entries); one exchange then gives both halves the ray's flag and extrema (p3d_importance.hpp)
            const int c0 = h * (Sc >> 1);
            float first = 0.0f;
#pragma unroll
            for (int q = 0; q < JP; ++q) {
                if (8 * q < Sc) {  // wave-uniform
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int i = c0 + 4 * q + e;
                        const float t = p3d_stratified_depth(i, Sc, jw[q][e], sp);
                        tcA[i * 32 + j] = t;
                        unsorted |= (t < prev);
                        prev = t;
                        if (q == 0 && e == 0) first = t;
                        tcmin = __builtin_fminf(tcmin, t);
                        tcmax = __builtin_fmaxf(tcmax, t);
                        if constexpr (DUMP) if (active && p.dumps.depths_coarse) p.dumps.depths_coarse[ray * Sc + i] = t;
                    }
                }
            }
            p3d_stratified_combine(h, first, prev, unsorted, tcmin, tcmax);
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // the coarse loop reads the rows the other half wrote
        } else
        for (int i0 = 0; i0 < Sc; i0 += 8) {  // eight loads of the jitter row in flight (one at a time exposed a global-load latency per sample)
            float jv[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) jv[q] = cx.jitter(i0 + q < Sc ? i0 + q : Sc - 1);
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int i = i0 + q;
                if (i < Sc) {  // wave-uniform
                    const float t = p3d_stratified_depth(i, Sc, jv[q], sp);
                    tcA[i * 32 + j] = t;
                    unsorted |= (t < prev);
                    prev = t;
                    tcmin = __builtin_fminf(tcmin, t);
                    tcmax = __builtin_fmaxf(tcmax, t);
                    if constexpr (DUMP) if (dump && p.dumps.depths_coarse) p.dumps.depths_coarse[ray * Sc + i] = t;
                }
            }
        }
    }
    P3D_PHASE(P3D_PH_STRAT);
    float tmin = __builtin_inff(), tmax = -__builtin_inff();
    if (Sf > 0) {
        // ---- coarse pass, densities only -> ray-marcher weights: renderer.py:179-211
        MarchState st = p3d_march_start();
        uint32_t mword = 0;  // bit i & 31: coarse sample i is KNOWN to carry sigma = -1000 (cropped, or really decoded and masked)
        if constexpr (TCG) {
            // stratified depths and coarse pass in one loop: the jitter row is read eight values at a time, the depths never reach LDS
            float prev = -__builtin_inff(), pmax = -__builtin_inff();  // previous depth; maximum of all depths before it
            for (int i0 = 0; i0 < Sc; i0 += 8) {
                float jv[8];
                if (wide_j) {
                    // the batch is here (the first one requested in front of the weight copy); the next batch's two pieces are
                    // requested in front of this batch's eight decodes
#pragma unroll
                    for (int q = 0; q < 8; ++q) jv[q] = jw[q >> 2][q & 3];
                    if (i0 + 8 < Sc) p3d_load_row_pieces<JP>(cx.jit + i0 + 8, 2, jw);  // wave-uniform
                } else {
#pragma unroll
                    for (int q = 0; q < 8; ++q) jv[q] = cx.jitter(i0 + q < Sc ? i0 + q : Sc - 1);
                }
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const int i = i0 + q;
                    if (i >= Sc) break;  // wave-uniform
                    const float t = p3d_stratified_fixed(i, Sc, jv[q], sp);
                    unsorted |= (t < prev);
                    bad_order |= (t < pmax);
                    pmax = __builtin_fmaxf(pmax, prev);
                    prev = t;
                    tcmin = __builtin_fminf(tcmin, t);
                    tcmax = __builtin_fmaxf(tcmax, t);
                    const float px = ox + t * dx, py = oy + t * dy, pz = oz + t * dz;  // renderer.py:179
                    float sigma = P3D_SIGMA_MASKED;
                    const bool cropped = cx.cropped(px, pz);
                    const bool live = !(cropped || st.Td < 1e-60);
                    const bool skip = __builtin_amdgcn_ballot_w64(live) == 0;
                    if (!skip) {
                        f32x16 dummy;
                        p3d_decode_wave<false, true, false, INTERIOR>(lds, cx.rs, cx.g, cx.cfg, px, py, pz, sigma, dummy, live);
                    }
                    mword |= (cropped || (live && sigma == P3D_SIGMA_MASKED)) ? (1u << (i & 31)) : 0u;
                    if ((i & 31) == 31 || i == Sc - 1) {  // wave-uniform
                        if ((i >> 5) == 0) mw0 = mword; else if ((i >> 5) == 1) mw1 = mword; else mw2 = mword;
                        mword = 0;
                    }
                    if (i > 0) wcA[(i - 1) * 32 + j] = p3d_march_interval(st, t, sigma).w;
                    st.prev_t = t; st.prev_sigma = sigma;
                    ndec += skip ? 0 : 1;
                }
            }
        } else
        for (int i = 0; i < Sc; ++i) {
            float t = tcA[i * 32 + j];
            float px = ox + t * dx, py = oy + t * dy, pz = oz + t * dz;  // renderer.py:179
            float sigma = P3D_SIGMA_MASKED;
            bool skip = false, live = true, cropped = false;
            if (early) {
                cropped = cx.cropped(px, pz);
                live = !(cropped || st.Td < 1e-60);  // a cropped sample is -1000 by position; a dead ray's weights are 0
                skip = __builtin_amdgcn_ballot_w64(live) == 0;
            }
            if (!skip) {
                f32x16 dummy;
                p3d_decode_wave<false, true, false, INTERIOR>(lds, cx.rs, cx.g, cx.cfg, px, py, pz, sigma, dummy, live);
            }
            if (early) {  // a lane whose gathers were suppressed (dead ray) decoded garbage: its sample is NOT known to be masked
                mword |= (cropped || (live && sigma == P3D_SIGMA_MASKED)) ? (1u << (i & 31)) : 0u;
                if ((i & 31) == 31 || i == Sc - 1) { mkA[(i >> 5) * 32 + j] = mword; mword = 0; }
            }
            if constexpr (DUMP) if (dump && p.dumps.sigma_coarse) p.dumps.sigma_coarse[ray * Sc + i] = sigma;
            if (i > 0) {
                float w = p3d_march_interval(st, t, sigma).w;
                wcA[(i - 1) * 32 + j] = w;
                if constexpr (DUMP) if (dump && p.dumps.weights_coarse) p.dumps.weights_coarse[ray * (Sc - 1) + i - 1] = w;
            }
            st.prev_t = t; st.prev_sigma = sigma;
            if constexpr (!DUMP) ndec += skip ? 0 : 1;
        }
        P3D_PHASE(P3D_PH_COARSE);
        // ---- pdf -> cdf (per ray; by both halves — the draws and the sort are shared out: p3d_importance.hpp)
        const int Ns = Sc - 3;
        p3d_pdf_to_cdf<32>(wcA, Ns, j);
        P3D_PHASE(P3D_PH_CDF);
        // ---- draws, sort
        constexpr int DB = P3D_DRAW_BATCH;
        auto dump_draw = [&](bool mine, int i, float v, int k) {
            if constexpr (DUMP) {
                if (mine && p.dumps.depths_fine) p.dumps.depths_fine[ray * Sf + i] = v;
                if (mine && p.dumps.inds) p.dumps.inds[ray * Sf + i] = k;
            }
        };
        if constexpr (P3D_NF_EXACT(NF)) {
            // Half h makes the draws [h * H, (h + 1) * H), sorts them, and after one cross-half exchange and a local merge holds
            // H of the sorted ranks (p3d_importance.hpp): half 1 rank H + i in register i, half 0 MINUS rank H - 1 - i.
            constexpr int H = NF / 2;
            static_assert(H % DB == 0, "whole batches of draws per half");
            const int d0 = h * H;
            float tf[H];
            if (wide_u) {  // wave-uniform: the half row as H / 4 16-byte loads
                p3d_load_row_wide<H>(cx.uu + d0, tf);
            } else {
#pragma unroll
                for (int i = 0; i < H; ++i) tf[i] = cx.u(d0 + i);  // every load of the half row issued before the first search
            }
#pragma unroll
            for (int i0 = 0; i0 < H; i0 += DB) {
                float ub[DB], vb[DB];
                int kb[DB];
#pragma unroll
                for (int q = 0; q < DB; ++q) ub[q] = tf[i0 + q];
                p3d_inverse_cdf<DB, 32>(wcA, tc_of, Ns, j, ub, vb, kb);
#pragma unroll
                for (int q = 0; q < DB; ++q) {
                    tf[i0 + q] = vb[q];
                    dump_draw(active, d0 + i0 + q, vb[q], kb[q]);  // each half writes the entries of its own draws
                }
            }
            P3D_PHASE(P3D_PH_DRAWS);
            p3d_sort_halves<H>(tf, h);
            // over the cdf rows: every search of BOTH halves is done, and the other half's rows are read below — same wave, so
            // ordering the wave's own LDS operations is all it takes
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            const int row0 = p3d_half_rank(H, h, 0), rstep = h ? 1 : -1;
            const uint32_t neg0 = h ? 0u : 0x80000000u;  // half 0 holds its keys negated
            uint64_t crop = 0ull;  // TCG: bit i = the key of register i is cropped
            uint32_t crop24 = 0u;  // RANKS: the same (H <= 32 keys)
#pragma unroll
            for (int i = 0; i < H; ++i) {
                const float v = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, tf[i]) ^ neg0);
                tfA[(row0 + rstep * i) * 32 + j] = v;
                if constexpr (TCG) crop |= cx.cropped_at(v) ? (1ull << i) : 0ull;
                else if constexpr (RANKS) crop24 |= cx.cropped_at(v) ? (1u << i) : 0u;
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            if constexpr (TCG) {  // register i -> rank: half 1 shifts by H, half 0 mirrors; then each half takes the other's bits
                static_assert(H >= 32 && H < 64, "the 96 rank bits as 64 + 32");
                const uint64_t g0 = h ? (crop << H) : (__builtin_bitreverse64(crop) >> (64 - H));
                fw[0] = (uint32_t)g0; fw[1] = (uint32_t)(g0 >> 32); fw[2] = h ? (uint32_t)(crop >> (64 - H)) : 0u;
                fw[0] |= __shfl_xor(fw[0], 32); fw[1] |= __shfl_xor(fw[1], 32); fw[2] |= __shfl_xor(fw[2], 32);
            } else if constexpr (RANKS) {  // the same with 2 * H <= 64 rank bits
                static_assert(H <= 32, "a half's bits in one word, the rank bits in two");
                const uint64_t g0 = h ? ((uint64_t)crop24 << H) : (uint64_t)(__builtin_bitreverse32(crop24) >> (32 - H));
                fw[0] = (uint32_t)g0; fw[1] = (uint32_t)(g0 >> 32);
                fw[0] |= __shfl_xor(fw[0], 32); fw[1] |= __shfl_xor(fw[1], 32);
            }
        } else if constexpr (NF > 0) {  // the padded capacity (NF = 64): both halves do all of it
            // (the same text as k_render_slots' below, on purpose: behind one shared helper every LDS read of the searches got one
            // more VALU operation in front of it, +260-370 instructions per kernel, profiles/r08_resource_*.txt)
            float tf[NF];
            if (wide_u) {  // wave-uniform: Sf is whole pieces
#pragma unroll
                for (int q = 0; q < NF / 4; ++q) {
                    f32x4 v = 0.0f;
                    if (4 * q < Sf) v = *(const f32x4*)(cx.uu + 4 * q);
                    tf[4 * q] = v.x; tf[4 * q + 1] = v.y; tf[4 * q + 2] = v.z; tf[4 * q + 3] = v.w;
                }
            } else {
#pragma unroll
                for (int i = 0; i < NF; ++i) tf[i] = (i < Sf) ? cx.u(i) : 0.0f;  // every load of the row issued before the first search
            }
#pragma unroll
            for (int i0 = 0; i0 < NF; i0 += DB) {
                if (i0 < Sf) {  // wave-uniform
                    float ub[DB], vb[DB];
                    int kb[DB];
#pragma unroll
                    for (int q = 0; q < DB; ++q) ub[q] = tf[i0 + q];
                    p3d_inverse_cdf<DB, 32>(wcA, tc_of, Ns, j, ub, vb, kb);
#pragma unroll
                    for (int q = 0; q < DB; ++q) {
                        tf[i0 + q] = (i0 + q < Sf) ? vb[q] : __builtin_inff();
                        if (i0 + q < Sf) dump_draw(dump, i0 + q, vb[q], kb[q]);
                    }
                } else {
#pragma unroll
                    for (int q = 0; q < DB; ++q) tf[i0 + q] = __builtin_inff();
                }
            }
            P3D_PHASE(P3D_PH_DRAWS);
            p3d_sort_network<NF>(tf);
#pragma unroll
            for (int i = 0; i < NF; ++i)
                if (i < Sf) {
                    tfA[i * 32 + j] = tf[i];  // over the cdf rows: every search is done
                    if constexpr (TCG) {
                        const uint32_t b = cx.cropped_at(tf[i]) ? (1u << (i & 31)) : 0u;
                        if (i < 32) fw[0] |= b; else if (i < 64) fw[1] |= b; else fw[2] |= b;
                    }
                }
        } else {
            for (int i0 = 0; i0 < Sf; i0 += DB) {
                float ub[DB], vb[DB];
                int kb[DB];
                if (wide_u) {  // wave-uniform: Sf is whole batches
                    static_assert(DB == 8, "a batch of draws is two pieces");
                    p3d_load_row_wide<DB>(cx.uu + i0, ub);
                } else {
#pragma unroll
                    for (int q = 0; q < DB; ++q) ub[q] = cx.u(i0 + q < Sf ? i0 + q : Sf - 1);
                }
                p3d_inverse_cdf<DB, 32>(wcA, tc_of, Ns, j, ub, vb, kb);
#pragma unroll
                for (int q = 0; q < DB; ++q) {
                    if (i0 + q < Sf) {
                        tfA[(i0 + q) * 32 + j] = vb[q];
                        dump_draw(dump, i0 + q, vb[q], kb[q]);
                    }
                }
            }
            P3D_PHASE(P3D_PH_DRAWS);
            p3d_lds_insertion_sort(tfA, Sf, j);
        }
        P3D_PHASE(P3D_PH_SORT);
        // unify_samples (renderer.py:289-301) merges two sorted lists; the stratified list is sorted unless rounding
        // reversed two neighbours (practically never) — then sort it too.
        if constexpr (TCG) {
            wave_unsorted = __builtin_amdgcn_ballot_w64(unsorted) != 0;  // from here on tc_sorted() looks at the neighbours
            wave_bad = __builtin_amdgcn_ballot_w64(bad_order) != 0;
            if (wave_unsorted) { mw0 = 0u; mw1 = 0u; mw2 = 0u; }         // (bits indexed by draw order: forget them, as below)
        } else
        if (__builtin_amdgcn_ballot_w64(unsorted) != 0) {
            p3d_lds_insertion_sort(tcA, Sc, j);
            if (early) {  // the known-masked bits are indexed by ORIGINAL coarse index: forget them (practically never taken)
                for (int i = 0; i < ((Sc + 31) >> 5); ++i) mkA[i * 32 + j] = 0u;
            }
        }
    }
    // ---- final pass: merge pre-pass, then the walk (see the comment above the kernel)
    MarchState st = p3d_march_start();
    P3dAccum acc;
    f32x16 prev_rgb = 0.0f;
    {
        int ci = 0, fi = 0;
        float ta = TCG ? 0.0f : tcA[j], tb = (Sf > 0) ? tfA[j] : __builtin_inff();
        // the extrema of all depths of the ray (the global clamp range, ray_marcher.py:50); the fine list is sorted
        tmin = __builtin_fminf(tcmin, tb);
        tmax = __builtin_fmaxf(tcmax, (Sf > 0) ? tfA[(Sf - 1) * 32 + j] : -__builtin_inff());
        bool prev_skipped = false, first = true, done = false;
        int m = 0;  // samples of this lane consumed so far (position in the merged list)
        auto advance = [&](bool take_c) {  // pop the head of the coarse or of the fine list
            ci += take_c ? 1 : 0;
            fi += take_c ? 0 : 1;
            // (one LDS read at a selected address and two selects: `if (take_c) ta = ...; else tb = ...;` is turned into a store
            // through a selected POINTER, which parks ta / tb in scratch memory — 1.5-3 k clocks per merged sample)
            const int cq = ci < Sc ? ci : Sc - 1, fq = fi < Sf ? fi : (Sf > 0 ? Sf - 1 : 0);
            const float nv = (take_c ? tcA : tfA)[(take_c ? cq : fq) * 32 + j];
            ta = take_c ? nv : ta;
            tb = take_c ? tb : nv;
        };
        float tcn = 0.0f;  // TCG: the head of the coarse list, tc_sorted(min(ci, Sc - 1)), fetched ahead of its use
        if constexpr (TCG) {
            p3d_merge_bits_ranks<96, 6>(
                tc_sorted, [&](int k) { return tfA[k * 32 + j]; },
                [&](int i, float t) {
                    const uint32_t mwv = (i < 32) ? mw0 : (i < 64 ? mw1 : mw2);
                    return cx.cropped_at(t) || ((mwv >> (i & 31)) & 1u);
                },
                [&](int w, uint32_t kw, uint32_t sw) { knA[w * 32 + j] = kw; slA[w * 32 + j] = sw; }, fw, Sc, Sf, h);
            tcn = tc_sorted(0);
        } else
        if constexpr (EARLY) {
            // the merge, once: bit q of slA = merged sample q is the head of the coarse list, bit q of knA = its sigma is known
            bool by_ranks = false;
            if constexpr (RANKS) {
                // By rank search (p3d_importance.hpp): the coarse column is sorted by now, the coarse pass's known-masked bits are
                // read per rank from their rows, the fine samples' crop bits come from the sort's store, and both halves store
                // every word of the two rows once, the same value: nothing to zero, no OR in LDS, and each lane reads back only
                // what it stored itself.
                by_ranks = S <= 96 && !p.serial_merge;  // launch-uniform: three words per row; the flag is a test switch
                if (by_ranks) {
                    const uint32_t fwr[2] = {fw[0], fw[1]};
                    p3d_merge_bits_ranks<48, 3>(
                        [&](int i) { return tcA[i * 32 + j]; }, [&](int k) { return tfA[k * 32 + j]; },
                        [&](int i, float t) {
                            const int ic = i < Sc ? i : Sc - 1;
                            return cx.cropped_at(t) || ((mkA[(ic >> 5) * 32 + j] >> (ic & 31)) & 1u);
                        },
                        [&](int w, uint32_t kw, uint32_t sw) { knA[w * 32 + j] = kw; slA[w * 32 + j] = sw; }, fwr, Sc, Sf, h);
                }
            }
            if (!by_ranks) {
                // Serially: half 0 walks the merged positions [0, S/2), half 1 [S/2, S), starting behind the samples that lie in
                // front of the cut (p3d_importance.hpp).  The word that holds the cut gets bits from both halves, so the rows start
                // at zero and take their words by LDS OR.
                for (int w = 0; w < nmw; ++w) { knA[w * 32 + j] = 0u; slA[w * 32 + j] = 0u; }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                p3d_merge_bits_half(
                    [&](bool c, int i) { return (c ? tcA : tfA)[i * 32 + j]; },
                    [&](bool c, int i, float t) {
                        bool known = cx.cropped_at(t);
                        if (c && Sf > 0) known = known || ((mkA[(i >> 5) * 32 + j] >> (i & 31)) & 1u);  // Sf == 0: no coarse pass ran
                        return known;
                    },
                    [&](int w, uint32_t kw, uint32_t sw) { atomicOr(&knA[w * 32 + j], kw); atomicOr(&slA[w * 32 + j], sw); },
                    Sc, Sf, h);
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            }
            ci = 0;  // from here on: coarse samples among the first m merged ones (the fine index is m - ci)
        }
        P3D_PHASE(P3D_PH_MERGE);
        // EARLY: the walk keeps the current word of each bit row in a register, shifted so that bit 0 is sample m, and goes back to
        // LDS only when m enters the next word (four LDS round trips per step before, two of them behind the jump loop's exit);
        // and it carries the previous sample's position from step to step (recomputed only behind a jump, which moves prev_t).
        // Not the LDS-resident 96-key kernel (per-ray limits, disparity spacing): its exact instantiation sits at 224 + 32 registers,
        // and the register walk, with or without the carried position, costs it its second wave per SIMD (226 + 32).  It keeps the
        // walk that reads the words where it uses them.
        constexpr bool WALK_REGS = EARLY && (NF != 96 || TCG);
        constexpr bool CARRY_POS = WALK_REGS;
        uint32_t kw = 0u, sw = 0u;
        if constexpr (WALK_REGS) { kw = knA[j]; sw = slA[j]; }
        float ppx = ox + st.prev_t * dx, ppy = oy + st.prev_t * dy, ppz = oz + st.prev_t * dz;
        for (int it = 0;; ++it) {
            bool take_c, known = false;  // known: sigma = -1000 without a decode (reached here only behind a sigma > 602)
            float t;
            if constexpr (!EARLY) {
                if (it >= S) break;  // every lane takes exactly one sample per step: the plain uniform loop
                take_c = (ci < Sc) && (fi >= Sf || ta <= tb);
                t = take_c ? ta : tb;
                advance(take_c);
            } else {
                // exact mode: below 1e-60 every later weight alpha * (float)Td is exactly 0.  Tolerance mode: the transmittance
                // bounds everything the rest of the ray can still add (sum of the remaining weights <= Td): stop at P3D_FAST_TD_CUT,
                // (what that leaves out of each output: p3d_decode.hpp) — early ray termination, inside the stated bound
                // ... and a ray that has taken its last sample is done whatever that sample was: the jump below, which also notices
                // the end of the list, is not reached behind a sigma > 602 (binarize's solid value as the LAST sample)
                if (!done && (m >= S || st.Td < (FAST ? P3D_FAST_TD_CUT : 1e-60))) done = true;
                if constexpr (WALK_REGS) {
                    if (!done && (kw & 1u) != 0u && (first || st.prev_sigma <= 602.0f)) {
                        // jump over the run of known samples that starts at m (one iteration per 32-bit word the run touches).  The
                        // words are shifted in from above with zeros, so a run of ones ends at the word's last bit at the latest.
                        bool last_c = false;
                        for (;;) {
                            const int left = S - m;
                            int run = (~kw != 0u) ? __builtin_ctz(~kw) : 32;
                            run = run < left ? run : left;
                            if (run == 0) break;  // (a fresh word only) in front of a sample that has to be decoded
                            ci += __builtin_popcount(sw & (0xffffffffu >> (32 - run)));
                            last_c = (sw >> (run - 1)) & 1u;
                            m += run;
                            kw >>= (run & 31); sw >>= (run & 31);  // run = 32: the word is used up, see below
                            if (m >= S || (m & 31) != 0) break;    // the list's end, or a sample that has to be decoded
                            kw = knA[(m >> 5) * 32 + j]; sw = slA[(m >> 5) * 32 + j];  // the run reached the word's end: on into the next
                        }
                        if constexpr (TCG) {
                            // the two coarse depths a jump needs, requested together: the last consumed one and the new head
                            const float pc = tc_sorted(ci > 0 ? ci - 1 : 0);
                            tcn = tc_sorted(ci < Sc ? ci : Sc - 1);
                            st.prev_t = last_c ? pc : tfA[(m - ci - 1 > 0 ? m - ci - 1 : 0) * 32 + j];
                        } else
                        st.prev_t = last_c ? tcA[(ci - 1) * 32 + j] : tfA[(m - ci - 1) * 32 + j];
                        st.prev_sigma = P3D_SIGMA_MASKED;
                        prev_skipped = true; first = false;
                        ppx = ox + st.prev_t * dx; ppy = oy + st.prev_t * dy; ppz = oz + st.prev_t * dz;  // the jump moved prev_t
                        done = m >= S;
                    }
                    if (__builtin_amdgcn_ballot_w64(!done) == 0) break;
                    // bit 0 of the two words is sample m.  A finished lane's bits are stale: it needs a valid address and nothing else
                    take_c = (sw & 1u) != 0u;
                    known = !done && (kw & 1u) != 0u;
                } else {
                    // the walk without the registers (the LDS-resident 96-key kernel): the words are read where they are used
                    if (!done && (first || st.prev_sigma <= 602.0f)) {
                        // jump over the run of known samples that starts at m (one iteration per 32-bit word the run touches)
                        bool any = false, last_c = false;
                        while (m < S) {
                            const int sh = m & 31, left = (32 - sh < S - m) ? 32 - sh : S - m;
                            const uint32_t kr = knA[(m >> 5) * 32 + j] >> sh, sr = slA[(m >> 5) * 32 + j] >> sh;
                            int run = (~kr != 0u) ? __builtin_ctz(~kr) : 32;
                            run = run < left ? run : left;
                            if (run > 0) {
                                const uint32_t inrun = run >= 32 ? 0xffffffffu : ((1u << run) - 1u);
                                ci += __builtin_popcount(sr & inrun);
                                last_c = (sr >> (run - 1)) & 1u;
                                any = true;
                                m += run;
                            }
                            if (run < left) break;  // stopped in front of a sample that has to be decoded
                        }
                        if (any) {
                            st.prev_t = last_c ? tcA[(ci - 1) * 32 + j] : tfA[(m - ci - 1) * 32 + j];
                            st.prev_sigma = P3D_SIGMA_MASKED;
                            prev_skipped = true; first = false;
                        }
                        done = m >= S;
                    }
                    if (__builtin_amdgcn_ballot_w64(!done) == 0) break;
                    const int mm = done ? S - 1 : m;  // finished lanes: any valid address
                    const uint32_t kb = knA[(mm >> 5) * 32 + j] >> (mm & 31), sb = slA[(mm >> 5) * 32 + j] >> (mm & 31);
                    take_c = (sb & 1u) != 0u;
                    known = !done && (kb & 1u) != 0u;
                }
                const int cq = ci < Sc ? ci : Sc - 1, fq = (m - ci < Sf) ? m - ci : (Sf > 0 ? Sf - 1 : 0);
                if constexpr (TCG) t = take_c ? tcn : tfA[fq * 32 + j];
                else t = (take_c || Sf == 0) ? tcA[cq * 32 + j] : tfA[fq * 32 + j];
                if (!done) { ++m; ci += take_c ? 1 : 0; }
                if constexpr (WALK_REGS) {
                    kw >>= 1; sw >>= 1;
                    if (!done && (m & 31) == 0 && m < S) { kw = knA[(m >> 5) * 32 + j]; sw = slA[(m >> 5) * 32 + j]; }  // used one step later: under the decode
                }
                if constexpr (TCG) {
                    if (!done && take_c) tcn = tc_sorted(ci < Sc ? ci : Sc - 1);  // used one step later at the earliest: under the decode
                }
            }
            P3D_PHASE(P3D_PH_SELECT);
            const bool have = EARLY ? !done : true;
            const float px = ox + t * dx, py = oy + t * dy, pz = oz + t * dz;
            float sigma = P3D_SIGMA_MASKED;
            f32x16 rgb = 0.0f;
            const bool live = have && !known;
            bool skipped = true;
            if (__builtin_amdgcn_ballot_w64(live) != 0) {
                bool have_rgb;  // EARLY: colour on demand (p3d_decode.hpp, LAZY): a step whose live samples are all masked has none
                if constexpr (FAST) have_rgb = p3d_decode_wave_fast<true, true, EARLY, true, INTERIOR>(lds, cx.rs, cx.g, cx.cfg, px, py, pz, sigma, rgb, live);
                else have_rgb = p3d_decode_wave<true, true, EARLY, INTERIOR>(lds, cx.rs, cx.g, cx.cfg, px, py, pz, sigma, rgb, live);
                if constexpr (!DUMP) ndec += 1;
                skipped = !live || !have_rgb;  // per lane: a lane whose gathers were suppressed has no colour
                if (known) sigma = P3D_SIGMA_MASKED;
            }
            P3D_PHASE(P3D_PH_DECODE);
            if constexpr (DUMP) {
                if (dump && p.dumps.depths_sorted) p.dumps.depths_sorted[ray * S + m] = t;
                if (dump && p.dumps.sigma_sorted) p.dumps.sigma_sorted[ray * S + m] = sigma;
            }
            // (the guard decodes below are wave-level operations: every lane must reach them, also the ones without a sample)
            const bool marching = have && !first;
            P3dInterval iv = {0.0f, 0.0f, 0.0f, 0.0f};
            if (marching) iv = p3d_march_interval(st, t, sigma);
            if constexpr (!CARRY_POS) { ppx = ox + st.prev_t * dx; ppy = oy + st.prev_t * dy; ppz = oz + st.prev_t * dz; }
            // one wave-level test in front of the guard's two (k_render_slots<4, ...> spilled 80 more registers with it inside the guard)
            if (early && (!WALK_REGS || __builtin_amdgcn_ballot_w64(marching && (prev_skipped || skipped) && iv.w != 0.0f) != 0))
                p3d_guard_colours<FAST>(lds, cx, marching, iv.w, prev_skipped, prev_rgb, ppx, ppy, ppz, skipped, rgb, px, py, pz);
            if (have) {
                if (!first) p3d_composite_interval<false>(acc, st, iv, prev_rgb, rgb, ppx, ppy, ppz, px, py, pz);
                st.prev_t = t; st.prev_sigma = sigma;
                if constexpr (CARRY_POS) { ppx = px; ppy = py; ppz = pz; }  // o + prev_t * d of the next step, bit for bit: the same expression
                prev_rgb = rgb;
                prev_skipped = skipped;
                first = false;
                if constexpr (!EARLY) ++m;
            }
            P3D_PHASE(P3D_PH_MARCH);
        }
    }
    // ---- outputs (per ray; the depth clamp is global: k_render_finish), depth range
    p3d_ray_outputs<false, DUMP>(p, ray, h, active, acc, st);
    p3d_wave_minmax(active, tmin, tmax);
    P3D_PHASE(P3D_PH_OUT);
    P3D_PHASE_FLUSH();
    p3d_depth_range_atomics<!DUMP>(p, cx.nlo, lane, tmin, tmax, ndec);
}

// v of lane ^ X within each half-wave (X < 32): ds_swizzle in bit mode (and 0x1f, or 0, xor X) — the crossbar, no address VGPR
template <int X>
P3D_DEV float p3d_lane_xor(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, v), 0x1f | (X << 10)));
}

// x[k] of a 2- or 4-entry register array by selects of VALUES (a dynamic index, or a select of the entries' addresses, puts the
// array in scratch)
template <int N>
P3D_DEV float p3d_select(const float (&x)[N], int k) {
    static_assert(N == 2 || N == 4, "two or four entries");
    const float x0 = x[0], x1 = x[1];
    if constexpr (N == 2) {
        return (k & 1) ? x1 : x0;
    } else {
        const float x2 = x[2], x3 = x[3];
        return (k & 2) ? ((k & 1) ? x3 : x2) : ((k & 1) ? x1 : x0);
    }
}

// =====================================================================================================================
// k_render_slots: the same algorithm for SMALL launches (fewer 32-ray tiles than the chip has SIMDs, e.g. the pipeline's single
// 128^2-ray views: 512 tiles on 1024 SIMDs, each wave alone on its SIMD and ALU-bound at ~4.7 us per decode step).  A wave owns
// RPW = 32 / SLOTS rays and decodes SLOTS consecutive samples of every ray per step: lane j = ray (j % RPW) x sample slot (j / RPW)
// x channel half, so a launch makes SLOTS times as many waves, each with 1 / SLOTS of the decode steps.  SLOTS = 2: a 128^2-ray
// view makes 1024 waves, one per SIMD.  SLOTS = 4 (round 4): 2048 waves = TWO per SIMD (with two slots every step's bookkeeping
// was exposed latency: ~4 us per step whether it decodes or not, profiles/history/r03_notes.txt).  Per-wave LDS rows hold the
// wave's RPW rays (6.6 KB per wave at 96+96 with four slots).
// Everything per ray (depth rows in LDS, marcher, cdf, inverse-CDF draws, sort, merge, compositing) is executed identically by
// all lanes of the ray — same inputs, same order, same results, so the arithmetic contract and the accumulation order are
// untouched — and only the decode differs: after it the lanes exchange sigma and the skipped flag to every lane of the ray (the
// marcher state — transmittance, weights, the guards' decisions — is identical on them) and the 16 colour channels only towards
// slot 0, whose lanes write the outputs; the other slots accumulate colours in another order and never store them (48 crossbar
// moves per step with four slots instead of 48 + 192 selects).  Then every lane consumes the step's samples in order.
// Bit-identical to k_render.  No dumps on this path (the host falls back to k_render for them).
// FAST (P3D_FLAG_FAST_COLOR): the final pass decodes in tolerance mode exactly as k_render<…, FAST = true> does (two-term f16 MLP
// operands, hardware transcendentals, the exact mask guard, rays dropped below a transmittance of P3D_FAST_TD_CUT); the coarse pass, and
// with it every importance draw, stays on the exact contract.
// WO ("weights only", P3D_FLAG_WEIGHTS_ONLY; four-slot tolerance-mode instantiations only): the launch is asked for the accumulated
// opacity (wsum) and depth alone — the occlusion pass of paste_front (training/triplane.py:565-578 reads `image_weights` of a second
// render and nothing else).  A ray's weights depend on depths and densities only, so the final pass decodes DENSITIES (layer 1 + the
// sigma row, the coarse pass's cost), exchanges no colours, runs no colour guards and composites nothing but W and D: wsum and depth
// are bit-identical to the full launch's, feat / xyz are not written.
// Registers: one workgroup per CU is all a small launch has, and every instantiation but the four-slot tolerance ones is compiled for
// one wave per SIMD (up to 512 registers).  The four-slot tolerance ones are compiled for two (<= 256 registers; 128^2 rays = 2048
// waves).  The EXACT four-slot ones under the 256-register cap spilled 108-127 VGPRs (164-176 B of scratch per lane, round 4), and
// the host picks them only for launches of <= 8192 rays = <= 1024 waves — one per SIMD whatever the cap.
template <int SLOTS, int NF, bool FAST, bool WO = false>
__global__ __launch_bounds__(64 * P3D_RENDER_WAVES, p3d_render_slots_occ(SLOTS, FAST)) void k_render_slots(RenderParams p) {
    static_assert(SLOTS == 2 || SLOTS == 4, "16 rays x 2 slots or 8 rays x 4 slots per wave");
    static_assert(!WO || (FAST && SLOTS == 4), "the weights-only launch exists for the tolerance mode (the renderer class's default, what the paste runs)");
    constexpr int RPW = 32 / SLOTS;  // rays per wave
    constexpr int RS = RPW;          // floats per LDS row
    extern __shared__ __attribute__((aligned(16))) float lds[];
    p3d_load_mlp_to_lds(lds, p.w0, p.b0, p.w1, p.b1, !FAST);
    if constexpr (FAST) p3d_load_mlp_f16_to_lds(lds, p.w0, p.w1);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 31, h = lane >> 5;
    const int jr = j % RPW, slot = j / RPW;  // ray of the wave, sample slot
    const int nwaves = blockDim.x >> 6;
    long long tile = (long long)blockIdx.x * nwaves + wave;  // RPW-ray tiles
    if (tile >= p.ntiles) return;  // no workgroup barrier below this line
    float* wl = lds + (FAST ? P3D_LDS_FAST_FLOATS : P3D_LDS_MLP_FLOATS) + 4 + (size_t)wave * p.lds_rows * RS;
    const int Sc = p.Sc, Sf = P3D_NF_EXACT(NF) ? NF : p.Sf, S = Sc + Sf;
    const P3dRayCtx cx = p3d_ray_setup(p, p3d_slots_tile_ray<RPW>(p, tile, jr), Sc, Sf);
    const bool active = cx.active;
    const size_t ray = cx.ray;
    const float ox = cx.ox, oy = cx.oy, oz = cx.oz, dx = cx.dx, dy = cx.dy, dz = cx.dz;
    const bool early = !(cx.cfg.flags & P3D_FLAG_NO_EARLY_OUT);
    int ndec = 0;
    // xk = v of the lane whose slot differs by k (lane ^ RPW k; x2, x3: four slots only).  Scalars rather than an array, and
    // of_slot's select tree rather than p3d_select's: with those the four-slot instantiations spilled SGPRs or allocated scratch.
    struct Slots { float x0, x1, x2, x3; };
    auto exchange = [](float v) {
        Slots s{v, p3d_lane_xor<RPW>(v), v, v};
        if constexpr (SLOTS == 4) { s.x2 = p3d_lane_xor<2 * RPW>(v); s.x3 = p3d_lane_xor<3 * RPW>(v); }
        return s;
    };
    // the value of sample slot q of this lane's ray, on EVERY lane of the ray, from exchange(): the lane whose slot is q sits at
    // lane ^ RPW (slot ^ q)
    auto of_slot = [&](int q, Slots s) {
        const int k = slot ^ q;
        return (k & 1) ? ((k & 2) ? s.x3 : s.x1) : ((k & 2) ? s.x2 : s.x0);
    };

    // LDS rows of this wave: row(i)[jr]; all slots of a ray write the same values
    float* tcA = wl;
    float* wcA = tcA + Sc * RS;
    float* tfA = (NF > 0) ? wcA : wcA + Sc * RS;
    auto tc_lds = [&](int i) { return tcA[i * RS + jr]; };

    bool unsorted = false;
    {
        const P3dSpacing sp = p3d_spacing_of(p, ray, Sc);
        float prev = -__builtin_inff();
        for (int i = 0; i < Sc; ++i) {
            const float t = p3d_stratified_depth(i, Sc, cx.jitter(i), sp);
            tcA[i * RS + jr] = t;
            unsorted |= (t < prev);
            prev = t;
        }
    }
    float tmin = __builtin_inff(), tmax = -__builtin_inff();
    if (Sf > 0) {
        // ---- coarse pass, SLOTS samples per step
        MarchState st = p3d_march_start();
        for (int i = 0; i < Sc; i += SLOTS) {
            float tq[SLOTS];
#pragma unroll
            for (int q = 0; q < SLOTS; ++q) tq[q] = tcA[(i + q < Sc ? i + q : Sc - 1) * RS + jr];
            const float t = p3d_select(tq, slot);
            const float px = ox + t * dx, py = oy + t * dy, pz = oz + t * dz;
            float sigma = P3D_SIGMA_MASKED;
            bool skip = false, live = true;
            if (early) {
                live = !(cx.cropped(px, pz) || st.Td < 1e-60);  // slots > 0: Td before the step's first interval — conservative, still exact
                skip = __builtin_amdgcn_ballot_w64(live) == 0;
            }
            if (!skip) {
                f32x16 dummy;
                p3d_decode_wave<false, true>(lds, cx.rs, cx.g, cx.cfg, px, py, pz, sigma, dummy, live);
                ndec += 1;
            }
            const Slots sx = exchange(sigma);
#pragma unroll
            for (int q = 0; q < SLOTS; ++q) {
                if (i + q < Sc) {  // uniform
                    const float sq = of_slot(q, sx);
                    if (i + q > 0) wcA[(i + q - 1) * RS + jr] = p3d_march_interval(st, tq[q], sq).w;
                    st.prev_t = tq[q]; st.prev_sigma = sq;
                }
            }
        }
        // ---- pdf -> cdf, draws, sort
        const int Ns = Sc - 3;
        p3d_pdf_to_cdf<RS>(wcA, Ns, jr);
        if constexpr (NF > 0) {
            // the padded capacity, k_render's text (see there why not one shared function): all loads first, eight draws in lock-step
            float tf[NF];
            constexpr int DB = P3D_DRAW_BATCH;
#pragma unroll
            for (int i = 0; i < NF; ++i) tf[i] = (i < Sf) ? cx.u(i) : 0.0f;
#pragma unroll
            for (int i0 = 0; i0 < NF; i0 += DB) {
                if (i0 < Sf) {  // wave-uniform
                    float ub[DB], vb[DB];
                    int kb[DB];
#pragma unroll
                    for (int q = 0; q < DB; ++q) ub[q] = tf[i0 + q];
                    p3d_inverse_cdf<DB, RS>(wcA, tc_lds, Ns, jr, ub, vb, kb);
#pragma unroll
                    for (int q = 0; q < DB; ++q) tf[i0 + q] = (i0 + q < Sf) ? vb[q] : __builtin_inff();
                } else {
#pragma unroll
                    for (int q = 0; q < DB; ++q) tf[i0 + q] = __builtin_inff();
                }
            }
            p3d_sort_network<NF>(tf);
#pragma unroll
            for (int i = 0; i < NF; ++i)
                if (i < Sf) tfA[i * RS + jr] = tf[i];
        } else {
            // the generic path sorts in LDS: only slot 0 may move the keys (all slots of a ray share the column)
            for (int i = 0; i < Sf; ++i) {
                const float ui[1] = {cx.u(i)};
                float v[1];
                int k[1];
                p3d_inverse_cdf<1, RS>(wcA, tc_lds, Ns, jr, ui, v, k);
                tfA[i * RS + jr] = v[0];
            }
            if (slot == 0 && h == 0) p3d_lds_insertion_sort<RS>(tfA, Sf, jr);
        }
        if (__builtin_amdgcn_ballot_w64(unsorted) != 0 && slot == 0 && h == 0) p3d_lds_insertion_sort<RS>(tcA, Sc, jr);
    }
    // ---- final pass: SLOTS merged samples per step
    MarchState st = p3d_march_start();
    P3dAccum acc;
    f32x16 prev_rgb = 0.0f;
    float ppx = 0.0f, ppy = 0.0f, ppz = 0.0f;
    {
        int ci = 0, fi = 0;
        float ta = tcA[jr], tb = (Sf > 0) ? tfA[jr] : __builtin_inff();
        bool prev_skipped = false;
        auto next_depth = [&]() {  // unify_samples' merge: ties take the coarse sample first (stable sort)
            const bool take_c = (ci < Sc) && (fi >= Sf || ta <= tb);
            const float t = take_c ? ta : tb;
            ci += take_c ? 1 : 0;
            fi += take_c ? 0 : 1;
            const int cq = ci < Sc ? ci : Sc - 1, fq = fi < Sf ? fi : (Sf > 0 ? Sf - 1 : 0);
            const float nv = (take_c ? tcA : tfA)[(take_c ? cq : fq) * RS + jr];  // (selects, not a store through a selected pointer)
            ta = take_c ? nv : ta;
            tb = take_c ? tb : nv;
            tmin = __builtin_fminf(tmin, t);
            tmax = __builtin_fmaxf(tmax, t);
            return t;
        };
        // the second half of k_render's loop body, for one sample whose decode (or skip) has already happened
        auto consume = [&](int m, float t, float px, float py, float pz, float sigma, f32x16 rgb, bool skipped) {
            if (m > 0) {
                const P3dInterval iv = p3d_march_interval(st, t, sigma);
                if (early && !WO) p3d_guard_colours<FAST>(lds, cx, true, iv.w, prev_skipped, prev_rgb, ppx, ppy, ppz, skipped, rgb, px, py, pz);
                p3d_composite_interval<WO>(acc, st, iv, prev_rgb, rgb, ppx, ppy, ppz, px, py, pz);
            }
            st.prev_t = t; st.prev_sigma = sigma;
            prev_rgb = rgb;
            prev_skipped = skipped;
            ppx = px; ppy = py; ppz = pz;
        };
        for (int m = 0; m < S; m += SLOTS) {
            float tq[SLOTS], pxq[SLOTS], pyq[SLOTS], pzq[SLOTS];
#pragma unroll
            for (int q = 0; q < SLOTS; ++q) {
                tq[q] = (m + q < S) ? next_depth() : tq[q > 0 ? q - 1 : 0];  // (uniform condition)
                pxq[q] = ox + tq[q] * dx; pyq[q] = oy + tq[q] * dy; pzq[q] = oz + tq[q] * dz;
            }
            const float px = p3d_select(pxq, slot), py = p3d_select(pyq, slot), pz = p3d_select(pzq, slot);
            float sigma = P3D_SIGMA_MASKED;
            f32x16 rgb = 0.0f;
            bool skipped = false, live = true;
            if (early) {
                // exact mode: below 1e-60 every later weight is exactly 0.  Tolerance mode: the transmittance bounds what the rest
                // of the ray can still add — stop at P3D_FAST_TD_CUT (p3d_decode.hpp, as in k_render)
                live = !(cx.cropped(px, pz) || st.Td < (FAST ? P3D_FAST_TD_CUT : 1e-60));
                skipped = __builtin_amdgcn_ballot_w64(live) == 0;
            }
            if (!skipped) {
                if constexpr (FAST) p3d_decode_wave_fast<!WO, true, false, true>(lds, cx.rs, cx.g, cx.cfg, px, py, pz, sigma, rgb, live);
                else p3d_decode_wave<true, true>(lds, cx.rs, cx.g, cx.cfg, px, py, pz, sigma, rgb, live);
                ndec += 1;
                skipped = !live;
            }
            // exchange (see the header): sigma and the skipped flag to every lane of the ray; the colours of sample q at
            // lane ^ RPW q, which holds them only for the slot-0 lanes
            const Slots sx = exchange(sigma), kx = exchange(skipped ? 1.0f : 0.0f);
            f32x16 r1 = rgb, r2 = rgb, r3 = rgb;
            if constexpr (!WO) {
#pragma unroll
                for (int c = 0; c < 16; ++c) { const Slots x = exchange(rgb[c]); r1[c] = x.x1; r2[c] = x.x2; r3[c] = x.x3; }
            }
            consume(m, tq[0], pxq[0], pyq[0], pzq[0], of_slot(0, sx), rgb, of_slot(0, kx) != 0.0f);
            if (m + 1 < S) consume(m + 1, tq[1], pxq[1], pyq[1], pzq[1], of_slot(1, sx), r1, of_slot(1, kx) != 0.0f);
            if constexpr (SLOTS == 4) {
                if (m + 2 < S) consume(m + 2, tq[2], pxq[2], pyq[2], pzq[2], of_slot(2, sx), r2, of_slot(2, kx) != 0.0f);
                if (m + 3 < S) consume(m + 3, tq[3], pxq[3], pyq[3], pzq[3], of_slot(3, sx), r3, of_slot(3, kx) != 0.0f);
            }
        }
    }
    // ---- outputs (slot 0's lanes), depth range
    p3d_ray_outputs<WO, false>(p, ray, h, active && slot == 0, acc, st);
    p3d_wave_minmax(active, tmin, tmax);
    p3d_depth_range_atomics<true>(p, cx.nlo, lane, tmin, tmax, ndec);
}

__global__ void k_minmax_init(uint32_t* g, int nviews) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) {
        g[0] = 0xffffffffu;
        g[1] = 0u;
        g[2] = 0u;  // [2..3]: 64-bit count of wave-level decode steps of the launch (statistics for bench.py)
        g[3] = 0u;
    }
    if (i < nviews) { g[4 + 2 * i] = 0xffffffffu; g[5 + 2 * i] = 0u; }  // per-view ranges (P3D_FLAG_PER_VIEW_CLAMP)
}

// rays_per_view > 0: ray i is clamped to the range of ITS view (g + 4 + 2 * (i / rays_per_view)); 0: one range for the call
__global__ void k_render_finish(float* depth, long long n, const uint32_t* g, float* dump_tminmax, long long rays_per_view) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0 && dump_tminmax) { dump_tminmax[0] = p3d_ord2f(g[0]); dump_tminmax[1] = p3d_ord2f(g[1]); }
    if (i < n) {
        const uint32_t* mm = rays_per_view > 0 ? g + 4 + 2 * (i / rays_per_view) : g;
        const float lo = p3d_ord2f(mm[0]), hi = p3d_ord2f(mm[1]);
        float d = depth[i];
        d = d < lo ? lo : d;  // torch.clamp(x, min, max) = min(max(x, min), max)
        d = d > hi ? hi : d;
        depth[i] = d;
    }
}

// =====================================================================================================================
// operator-level stand-alone stages (one thread per ray)
// =====================================================================================================================
__global__ void k_stratified(float start, float end, float delta, int S, const float* __restrict__ jitter, long long NR,
                             float* __restrict__ out) {
    long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= NR) return;
    const P3dSpacing sp = p3d_spacing_fixed(start, end, delta, S);
    for (int i = 0; i < S; ++i) out[r * S + i] = p3d_stratified_fixed(i, S, jitter[r * S + i], sp);
}

__global__ void k_minmax_decode(const uint32_t* g, float* out) {
    out[0] = p3d_ord2f(g[0]);
    out[1] = p3d_ord2f(g[1]);
}

__global__ void k_depth_minmax(const float* __restrict__ d, long long n, uint32_t* g) {
    float lo = __builtin_inff(), hi = -__builtin_inff();
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        lo = __builtin_fminf(lo, d[i]);
        hi = __builtin_fmaxf(hi, d[i]);
    }
    p3d_wave_minmax(true, lo, hi);
    if ((threadIdx.x & 63) == 0) {
        atomicMin(g, p3d_f2ord(lo));
        atomicMax(g + 1, p3d_f2ord(hi));
    }
}

// MipRayMarcher2.run_forward, one thread per (ray, channel-slice): thread handles channels k = c0, c0+KS, ...
// To keep the weights bit-identical across the slices every thread recomputes them (cheap) — ray_marcher.py:25-57.
__global__ void k_composite(const float* __restrict__ colors, const float* __restrict__ sigma,
                            const float* __restrict__ depths, long long NR, int S, int K, int white_back,
                            float* __restrict__ out_rgb, float* __restrict__ out_depth, float* __restrict__ out_w) {
    long long r = (long long)blockIdx.x * blockDim.y + threadIdx.y;
    if (r >= NR) return;
    const int c0 = threadIdx.x, KS = blockDim.x;
    const float* col = colors + r * S * K;
    const float* sg = sigma + r * S;
    const float* t = depths + r * S;
    MarchState st = p3d_march_start(t[0], sg[0]);
    float C[8];  // up to 8 channels per thread (K <= 8*KS)
#pragma unroll
    for (int q = 0; q < 8; ++q) C[q] = 0.0f;
    for (int i = 1; i < S; ++i) {
        const P3dInterval iv = p3d_march_interval(st, t[i], sg[i]);
        if (out_w && c0 == 0) out_w[r * (S - 1) + i - 1] = iv.w;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            int k = c0 + q * KS;
            if (k < K) C[q] = p3d_composite_channel(iv.w, col[(i - 1) * K + k], col[i * K + k], C[q]);
        }
        p3d_march_accumulate(st, iv);
        st.prev_t = t[i]; st.prev_sigma = sg[i];
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        int k = c0 + q * KS;
        if (k < K) out_rgb[r * K + k] = p3d_white_back_rescale(C[q], white_back, st.W);
    }
    if (c0 == 0) out_depth[r] = p3d_ray_depth(st);
}

// sample_importance + sample_pdf, one thread per ray, scratch in registers/local memory — renderer.py:328-387
__global__ void k_importance(const float* __restrict__ depths, const float* __restrict__ weights, long long NR, int Sc,
                             int Sf, const float* __restrict__ u, float* __restrict__ out_depths,
                             int* __restrict__ out_inds) {
    long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= NR) return;
    const float* t = depths + r * Sc;
    const float* w = weights + r * (Sc - 1);
    const int Ns = Sc - 3;
    float cdf[P3D_MAX_S];
    double sum = 0.0;
    for (int jj = 0; jj < Ns; ++jj) {
        float v = p3d_pdf_bin(w[jj], w[jj + 1], w[jj + 2]);
        sum += (double)v;
        cdf[jj + 1] = v;
    }
    float fsum = (float)sum;
    double acc = 0.0;
    cdf[0] = 0.0f;
    for (int jj = 0; jj < Ns; ++jj) cdf[jj + 1] = p3d_cdf_step(acc, cdf[jj + 1], fsum);
    for (int i = 0; i < Sf; ++i) {
        float ui = u[r * Sf + i];
        int lo = 0, hi = Ns + 1;
        while (lo < hi) {
            int mid = (lo + hi) >> 1;
            if (cdf[mid] <= ui) lo = mid + 1; else hi = mid;
        }
        int k = lo;
        int below = k - 1 > 0 ? k - 1 : 0;
        int above = k < Ns ? k : Ns;
        float den = cdf[above] - cdf[below];
        if (den < 1e-5f) den = 1.0f;
        float bb = 0.5f * (t[below] + t[below + 1]);
        float ba = 0.5f * (t[above] + t[above + 1]);
        out_depths[r * Sf + i] = bb + ((ui - cdf[below]) / den) * (ba - bb);
        if (out_inds) out_inds[r * Sf + i] = k;
    }
}

// unify_samples permutation (stable ascending), one thread per ray, rank counting — renderer.py:289-301
__global__ void k_unify_perm(const float* __restrict__ tc, const float* __restrict__ tf, long long NR, int Sc, int Sf,
                             int* __restrict__ perm) {
    long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= NR) return;
    const int S = Sc + Sf;
    const float* a = tc + r * Sc;
    const float* b = tf + r * Sf;
    for (int i = 0; i < S; ++i) {
        float ki = i < Sc ? a[i] : b[i - Sc];
        int rank = 0;
        for (int q = 0; q < S; ++q) {
            float kq = q < Sc ? a[q] : b[q - Sc];
            rank += (kq < ki || (kq == ki && q < i)) ? 1 : 0;
        }
        perm[r * S + rank] = i;
    }
}

// sigma2density + the two masks of get_eg3d_volume (_util/eg3d_metrics3d.py:65-69,153-163), one HBM pass:
//   d = 1 - exp(-softplus(sigma - 1));  cropmask -> d = -1000;  cull (sic, evaluated on the DENSITIES, renderer.py:150-153):
//   1 - exp(-softplus(d - 1)) < cull_thresh -> d = -1000.   Contract math (include/p3d_numerics.h).
P3D_DEV float p3d_density_of(float sigma, bool cropped, float cull_thresh) {
    float d = 1.0f - p3d_exp_nonpos(-p3d_softplus(sigma - 1.0f));
    if (cropped) d = -1000.0f;
    if (cull_thresh >= 0.0f) {
        const float a2 = 1.0f - p3d_exp_nonpos(-p3d_softplus(d - 1.0f));
        if (a2 < cull_thresh) d = -1000.0f;
    }
    return d;
}
// four values per thread (16-byte loads / stores); the host passes vec = 1 only when sigma / out are 16-byte and cropmask
// 4-byte aligned
__global__ void k_sigma2density(const float* __restrict__ sigma, const unsigned char* __restrict__ cropmask, long long M,
                                float cull_thresh, float* __restrict__ out, int vec) {
    const long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i >= M) return;
    if (vec && i + 3 < M) {
        const float4 s4 = *reinterpret_cast<const float4*>(sigma + i);
        uchar4 c4 = make_uchar4(0, 0, 0, 0);
        if (cropmask) c4 = *reinterpret_cast<const uchar4*>(cropmask + i);
        float4 d4;
        d4.x = p3d_density_of(s4.x, c4.x != 0, cull_thresh);
        d4.y = p3d_density_of(s4.y, c4.y != 0, cull_thresh);
        d4.z = p3d_density_of(s4.z, c4.z != 0, cull_thresh);
        d4.w = p3d_density_of(s4.w, c4.w != 0, cull_thresh);
        *reinterpret_cast<float4*>(out + i) = d4;
    } else {
        for (long long k = i; k < i + 4 && k < M; ++k) out[k] = p3d_density_of(sigma[k], cropmask && cropmask[k], cull_thresh);
    }
}

// =====================================================================================================================
// C ABI
// =====================================================================================================================
static inline int p3d_check_launch() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? P3D_OK : (int)e;
}

// hipFuncAttributeMaxDynamicSharedMemorySize is sticky per (kernel, device): raise it only when a launch needs more than any
// earlier one did (one call per kernel instantiation in steady state instead of one per launch).
template <typename K>
static hipError_t p3d_ensure_dynamic_lds(K kernel, size_t bytes) {
    static std::atomic<size_t> granted[64];  // per instantiation, indexed by device ordinal
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::atomic<size_t>& g = granted[dev & 63];
    if (bytes <= g.load(std::memory_order_acquire)) return hipSuccess;
    e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess) {
        size_t cur = g.load(std::memory_order_relaxed);
        while (cur < bytes && !g.compare_exchange_weak(cur, bytes, std::memory_order_release)) {}
    }
    return e;
}

// Calls f(std::integral_constant<int, NF>()) with the fine-depth capacity nf of a render launch (48, 64, 96, or 0: the generic path)
template <typename F>
static int p3d_with_nf(int nf, F f) {
#ifdef P3D_ONLY_NF  // development builds (tools/resource_usage.py -D P3D_ONLY_NF=48): compile ONE fine-depth capacity
    (void)nf;
    return f(std::integral_constant<int, P3D_ONLY_NF>());
#else
    if (nf == 48) return f(std::integral_constant<int, 48>());
    if (nf == 64) return f(std::integral_constant<int, 64>());
    if (nf == 96) return f(std::integral_constant<int, 96>());
    return f(std::integral_constant<int, 0>());
#endif
}

static P3dDecodeCfg make_cfg(const p3d_opts* o) {
    P3dDecodeCfg c;
    c.coord_scale = o->coord_scale;
    c.crop_limit = o->crop_limit;
    c.cull_thresh = o->cull_thresh;
    p3d_cull_band(o->cull_thresh, &c.cull_s_lo, &c.cull_s_hi);
    c.plane_mode = o->plane_mode;
    c.flags = o->flags;
    return c;
}

extern "C" {

// (p3d_build_info lives in p3d_paste.hip: the small translation unit that is recompiled when any source changes)
int p3d_abi_version(void) { return P3D_ABI_VERSION; }

int p3d_struct_layout(int which, size_t* out, int cap) {
    if (!out || cap <= 0) return P3D_E_ARG;
    int n = 0;
#define P3D_PUT(v) do { if (n >= cap) return P3D_E_RANGE; out[n++] = (size_t)(v); } while (0)
#define P3D_OFF(T, f) P3D_PUT(offsetof(T, f))
    switch (which) {
    case P3D_STRUCT_OPTS:
        P3D_PUT(sizeof(p3d_opts));
        P3D_OFF(p3d_opts, coord_scale); P3D_OFF(p3d_opts, ray_start); P3D_OFF(p3d_opts, ray_end); P3D_OFF(p3d_opts, depth_delta);
        P3D_OFF(p3d_opts, crop_limit); P3D_OFF(p3d_opts, cull_thresh); P3D_OFF(p3d_opts, Sc); P3D_OFF(p3d_opts, Sf);
        P3D_OFF(p3d_opts, plane_mode); P3D_OFF(p3d_opts, flags);
        break;
    case P3D_STRUCT_DUMPS:
        P3D_PUT(sizeof(p3d_dumps));
        P3D_OFF(p3d_dumps, depths_coarse); P3D_OFF(p3d_dumps, sigma_coarse); P3D_OFF(p3d_dumps, weights_coarse);
        P3D_OFF(p3d_dumps, depths_fine); P3D_OFF(p3d_dumps, inds); P3D_OFF(p3d_dumps, depths_sorted); P3D_OFF(p3d_dumps, sigma_sorted);
        P3D_OFF(p3d_dumps, depth_unclamped); P3D_OFF(p3d_dumps, tminmax);
        break;
    case P3D_STRUCT_PASTE_ARGS:
        P3D_PUT(sizeof(p3d_paste_args));
        P3D_OFF(p3d_paste_args, weights); P3D_OFF(p3d_paste_args, xyz); P3D_OFF(p3d_paste_args, occ); P3D_OFF(p3d_paste_args, rays_o);
        P3D_OFF(p3d_paste_args, rays_d); P3D_OFF(p3d_paste_args, front); P3D_OFF(p3d_paste_args, image);
        P3D_OFF(p3d_paste_args, out_image); P3D_OFF(p3d_paste_args, out_paste); P3D_OFF(p3d_paste_args, out_mask);
        P3D_OFF(p3d_paste_args, out_mask_weights); P3D_OFF(p3d_paste_args, out_mask_edges); P3D_OFF(p3d_paste_args, out_mask_occ);
        P3D_OFF(p3d_paste_args, out_mask_dxyz);
        P3D_OFF(p3d_paste_args, N); P3D_OFF(p3d_paste_args, r); P3D_OFF(p3d_paste_args, S); P3D_OFF(p3d_paste_args, front_shared);
        P3D_OFF(p3d_paste_args, normalize_images);
        P3D_OFF(p3d_paste_args, thresh_weight); P3D_OFF(p3d_paste_args, thresh_edges); P3D_OFF(p3d_paste_args, thresh_occ);
        P3D_OFF(p3d_paste_args, thresh_dxyz); P3D_OFF(p3d_paste_args, box_warp);
        break;
    case P3D_STRUCT_CONV_ARGS:
        P3D_PUT(sizeof(p3d_conv_args));
        P3D_OFF(p3d_conv_args, x); P3D_OFF(p3d_conv_args, w); P3D_OFF(p3d_conv_args, w_f16); P3D_OFF(p3d_conv_args, styles);
        P3D_OFF(p3d_conv_args, demod_coefs); P3D_OFF(p3d_conv_args, noise); P3D_OFF(p3d_conv_args, bias); P3D_OFF(p3d_conv_args, fir);
        P3D_OFF(p3d_conv_args, y); P3D_OFF(p3d_conv_args, workspace); P3D_OFF(p3d_conv_args, saturated); P3D_OFF(p3d_conv_args, x_img);
        P3D_OFF(p3d_conv_args, y_img); P3D_OFF(p3d_conv_args, y_img_styles);
        P3D_OFF(p3d_conv_args, rgb_w); P3D_OFF(p3d_conv_args, rgb_styles); P3D_OFF(p3d_conv_args, rgb_partial); P3D_OFF(p3d_conv_args, workspace_bytes);
        P3D_OFF(p3d_conv_args, N); P3D_OFF(p3d_conv_args, I); P3D_OFF(p3d_conv_args, H); P3D_OFF(p3d_conv_args, W); P3D_OFF(p3d_conv_args, O);
        P3D_OFF(p3d_conv_args, ks); P3D_OFF(p3d_conv_args, up); P3D_OFF(p3d_conv_args, demodulate); P3D_OFF(p3d_conv_args, noise_per_sample);
        P3D_OFF(p3d_conv_args, act); P3D_OFF(p3d_conv_args, mma);
        P3D_OFF(p3d_conv_args, alpha); P3D_OFF(p3d_conv_args, gain); P3D_OFF(p3d_conv_args, clamp); P3D_OFF(p3d_conv_args, rgb_channels); P3D_OFF(p3d_conv_args, w_f16_layout);
        break;
    default:
        return P3D_E_RANGE;
    }
#undef P3D_OFF
#undef P3D_PUT
    return n;
}

int p3d_planes_to_nhwc_f32(const float* src, int n3, int C, int H, int W, float* dst, void* stream) {
    if (!src || !dst || n3 <= 0 || H <= 0 || W <= 0) return P3D_E_ARG;
    if (C != P3D_C) return P3D_E_RANGE;
    int HW = H * W;
    dim3 grid((HW + 63) / 64, n3);
    hipLaunchKernelGGL(k_planes_to_nhwc, grid, dim3(256), 0, (hipStream_t)stream, src, dst, HW);
    return p3d_check_launch();
}

int p3d_triplane_decode_f32(const float* planes, int N, int H, int W, const float* coords, int64_t M, const float* w0,
                            const float* b0, const float* w1, const float* b1, const p3d_opts* opts, float* out_sigma,
                            float* out_rgb, void* stream) {
    if (!planes || !coords || !w0 || !b0 || !w1 || !b1 || !opts || !out_sigma || N <= 0 || M <= 0) return P3D_E_ARG;
    if (H <= 0 || W <= 0 || (long long)H * W * 128 * 3 >= 0x7ffffff0LL) return P3D_E_RANGE;
    DecodeParams p;
    p.planes = planes; p.coords = coords; p.w0 = w0; p.b0 = b0; p.w1 = w1; p.b1 = b1;
    p.out_sigma = out_sigma; p.out_rgb = out_rgb; p.M = M; p.H = H; p.W = W;
    p.tiles_per_img = (M + 31) / 32;
    p.ntiles = p.tiles_per_img * N;
    p.cfg = make_cfg(opts);
    p.grid_n = 0; p.grid_lo = 0; p.vsize = p.goff0 = p.goff1 = p.goff2 = 0.0f; p.out_cropmask = nullptr; p.mask_limit = 0.0f;
    long long blocks = (p.ntiles + P3D_WAVES_PER_WG - 1) / P3D_WAVES_PER_WG;
    if (blocks > 256 * 16) blocks = 256 * 16;  // grid-stride beyond 16 workgroups per CU
    const size_t lds_bytes = (size_t)(P3D_LDS_MLP_FLOATS + 4) * 4;
    if (out_rgb)
        hipLaunchKernelGGL((k_decode_points<true, false, false>), dim3((unsigned)blocks), dim3(P3D_WG), lds_bytes, (hipStream_t)stream, p);
    else
        hipLaunchKernelGGL((k_decode_points<false, false, false>), dim3((unsigned)blocks), dim3(P3D_WG), lds_bytes, (hipStream_t)stream, p);
    return p3d_check_launch();
}

int p3d_grid_density_f32(const float* planes, int H, int W, int grid_n, int64_t lo, int64_t hi, float voxel_size, float off0,
                         float off1, float off2, const float* w0, const float* b0, const float* w1, const float* b1,
                         const p3d_opts* opts, float* out_sigma, unsigned char* out_cropmask, float mask_limit, void* stream) {
    if (!planes || !w0 || !b0 || !w1 || !b1 || !opts || !out_sigma || grid_n <= 1 || lo < 0 || hi <= lo) return P3D_E_ARG;
    if (H <= 0 || W <= 0 || (long long)H * W * 128 * 3 >= 0x7ffffff0LL || hi > (int64_t)grid_n * grid_n * grid_n || grid_n > 1290)
        return P3D_E_RANGE;  // grid_n^3 < 2^31: the kernel's index arithmetic is 32-bit
    DecodeParams p;
    p.planes = planes; p.coords = nullptr; p.w0 = w0; p.b0 = b0; p.w1 = w1; p.b1 = b1;
    p.out_sigma = out_sigma; p.out_rgb = nullptr; p.out_cropmask = out_cropmask; p.mask_limit = mask_limit; p.M = hi - lo; p.H = H; p.W = W;
    p.tiles_per_img = (p.M + 31) / 32;
    p.ntiles = p.tiles_per_img;
    p.cfg = make_cfg(opts);
    p.grid_n = grid_n; p.grid_lo = lo; p.vsize = voxel_size; p.goff0 = off0; p.goff1 = off1; p.goff2 = off2;
    long long blocks = (p.ntiles + P3D_WAVES_PER_WG - 1) / P3D_WAVES_PER_WG;
    // grid-stride beyond 16 workgroups per CU; an ODD workgroup count, so that the stride (4 tiles per workgroup) is not a
    // multiple of the tiles per grid row: with P3D_FLAG_SKIP_CROPPED the masked ends of every row would otherwise always fall
    // on the same waves (measured: 10.7 ms instead of the expected ~7.5 at 512^3 with half of the grid masked)
    if (blocks > 256 * 16 - 1) blocks = 256 * 16 - 1;
    // four variants: exact / tolerance-mode decoder (P3D_FLAG_FAST_COLOR), texel boxes staged through LDS or direct gathers
    // (measurements: DESIGN.md §4.3)
    const bool fastd = (opts->flags & P3D_FLAG_FAST_COLOR) != 0;
    // LDS-staged texel boxes only on request: with quad-cooperative gathers the direct tolerance query is faster (512^3: 7.7 ms
    // direct, 10.0 staged; exact: 12.7 direct, 22.8 staged); P3D_FLAG_NO_STAGING is accepted and has nothing left to switch off
    const bool staged = (opts->flags & P3D_FLAG_FORCE_STAGING) != 0;
    const size_t lds_bytes = (size_t)((fastd ? P3D_LDS_FAST_FLOATS - P3D_LDS_B0P : P3D_LDS_MLP_FLOATS) + 4 +
                                      (staged ? P3D_WAVES_PER_WG * P3D_BOX_FLOATS_PER_WAVE : 0)) * 4;
    hipError_t e = hipSuccess;
#define P3D_LAUNCH_GRID(SV, FV)                                                                                       \
    do {                                                                                                              \
        e = p3d_ensure_dynamic_lds(k_decode_points<false, SV, FV>, lds_bytes);                                        \
        if (e == hipSuccess)                                                                                          \
            hipLaunchKernelGGL((k_decode_points<false, SV, FV>), dim3((unsigned)blocks), dim3(P3D_WG), lds_bytes, (hipStream_t)stream, p); \
    } while (0)
    if (staged) { if (fastd) P3D_LAUNCH_GRID(true, true); else P3D_LAUNCH_GRID(true, false); }
    else { if (fastd) P3D_LAUNCH_GRID(false, true); else P3D_LAUNCH_GRID(false, false); }
    if (e != hipSuccess) return (int)e;
    return p3d_check_launch();
}

int p3d_decode_features_f32(const float* feats, int N, int64_t M, const float* w0, const float* b0, const float* w1, const float* b1,
                            int force_sigmoid, float* out_sigma, float* out_rgb, void* stream) {
    if (!feats || !w0 || !b0 || !w1 || !b1 || !out_sigma || !out_rgb || N <= 0 || M <= 0) return P3D_E_ARG;
    if ((((uintptr_t)feats | (uintptr_t)out_rgb) & 15) != 0) return P3D_E_RANGE;  // 16-byte rows of 32 floats
    DecodeFeatParams p;
    p.feats = feats; p.w0 = w0; p.b0 = b0; p.w1 = w1; p.b1 = b1; p.out_sigma = out_sigma; p.out_rgb = out_rgb;
    p.M = M; p.tiles_per_img = (M + 31) / 32; p.ntiles = p.tiles_per_img * N;
    memset(&p.cfg, 0, sizeof(p.cfg));
    p.cfg.flags = force_sigmoid ? P3D_FLAG_FORCE_SIGMOID : 0;
    const size_t lds_bytes = (size_t)(P3D_LDS_MLP_FLOATS + 4) * 4;
    long long blocks = (p.ntiles + P3D_WAVES_PER_WG - 1) / P3D_WAVES_PER_WG;
    if (blocks > 256 * 8) blocks = 256 * 8;  // grid-stride: the weight image is loaded once per workgroup
    hipError_t e = p3d_ensure_dynamic_lds(k_decode_features, lds_bytes);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_decode_features, dim3((unsigned)blocks), dim3(P3D_WG), lds_bytes, (hipStream_t)stream, p);
    return p3d_check_launch();
}

size_t p3d_render_workspace_bytes(int N, int64_t R, int Sc, int Sf) {
    (void)R; (void)Sc; (void)Sf;
    return p3d_render_plan_workspace_bytes(N);
}

#ifdef P3D_PHASE_TIMING
// measurement builds only (tools/phase_timing.py): the section totals of every k_render wave since the last reset
int p3d_phase_read(unsigned long long* out, int n, int reset) {
    unsigned long long v[P3D_PH_N];
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpyFromSymbol(v, HIP_SYMBOL(g_p3d_phase), sizeof(v)) != hipSuccess) return -1;
    for (int q = 0; q < n && q < P3D_PH_N; ++q) out[q] = v[q];
    if (reset) {
        memset(v, 0, sizeof(v));
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_p3d_phase), v, sizeof(v)) != hipSuccess) return -1;
    }
    return P3D_PH_N;
}
// ... and the per-wave records of the LAST k_render launch: out[4 * i ..] = {start, end (100 MHz ticks), block, XCD} of wave slot i < n
int p3d_phase_read_waves(unsigned long long* out, int n) {
    if (!out || n < 0 || n > P3D_WAVE_RECORDS) return -1;
    P3dWaveRecord* v = (P3dWaveRecord*)malloc(sizeof(P3dWaveRecord) * (size_t)(n > 0 ? n : 1));
    if (!v) return -1;
    const bool ok = hipDeviceSynchronize() == hipSuccess &&
                    hipMemcpyFromSymbol(v, HIP_SYMBOL(g_p3d_wave), sizeof(P3dWaveRecord) * (size_t)n) == hipSuccess;
    for (int i = 0; ok && i < n; ++i) {
        out[4 * i] = v[i].t0; out[4 * i + 1] = v[i].t1; out[4 * i + 2] = v[i].block; out[4 * i + 3] = v[i].xcc;
    }
    free(v);
    return ok ? n : -1;
}
#endif
int p3d_render_plan_info(int N, int64_t R, int ray_tile_w, const p3d_opts* opts, int has_dumps, int has_ray_limits, int64_t* out, int cap) {
    if (!opts) return P3D_E_ARG;
    const RenderPlan pl = p3d_render_plan(N, R, ray_tile_w, *opts, has_dumps != 0, has_ray_limits != 0);
    if (pl.err) return pl.err;
    if (!out || cap < 6) return P3D_E_ARG;
    const int64_t info[6] = {pl.slots, pl.ntiles, pl.decode_steps_full, pl.grid, pl.block, (int64_t)pl.lds_bytes};
    for (int i = 0; i < 6; ++i) out[i] = info[i];
    return P3D_OK;
}

int p3d_render_taps_info(int N, int H, int W, int64_t R, int ray_tile_w, const p3d_opts* opts, int has_dumps, int has_ray_limits) {
    if (!opts) return P3D_E_ARG;
    if (H <= 0 || W <= 0) return P3D_E_RANGE;
    const RenderPlan pl = p3d_render_plan(N, R, ray_tile_w, *opts, has_dumps != 0, has_ray_limits != 0);
    if (pl.err) return pl.err;
    return p3d_render_plan_has_interior(pl) && p3d_render_interior_taps(H, W, *opts) ? 1 : 0;
}

int p3d_render_f32(const float* planes, int N, int H, int W, const float* rays_o, const float* rays_d, int64_t R,
                   int ray_tile_w, const float* jitter, const float* u, const float* w0, const float* b0,
                   const float* w1, const float* b1, const p3d_opts* opts, float* out_feat, float* out_depth,
                   float* out_wsum, float* out_xyz, void* workspace, size_t workspace_bytes, const p3d_dumps* dumps,
                   void* stream) {
    return p3d_render_limits_f32(planes, N, H, W, rays_o, rays_d, R, ray_tile_w, jitter, u, w0, b0, w1, b1, nullptr, nullptr, opts,
                                 out_feat, out_depth, out_wsum, out_xyz, workspace, workspace_bytes, dumps, stream);
}

static int render_impl(const float* planes, int N, int H, int W, const float* rays_o, const float* rays_d, int64_t R,
                       int ray_tile_w, const float* jitter, const float* u, int rng, uint64_t seed, const float* w0, const float* b0,
                       const float* w1, const float* b1, const float* ray_start, const float* ray_end, const p3d_opts* opts,
                       float* out_feat, float* out_depth, float* out_wsum, float* out_xyz, void* workspace,
                       size_t workspace_bytes, const p3d_dumps* dumps, void* stream);

int p3d_render_limits_f32(const float* planes, int N, int H, int W, const float* rays_o, const float* rays_d, int64_t R,
                          int ray_tile_w, const float* jitter, const float* u, const float* w0, const float* b0,
                          const float* w1, const float* b1, const float* ray_start, const float* ray_end, const p3d_opts* opts,
                          float* out_feat, float* out_depth, float* out_wsum, float* out_xyz, void* workspace,
                          size_t workspace_bytes, const p3d_dumps* dumps, void* stream) {
    return render_impl(planes, N, H, W, rays_o, rays_d, R, ray_tile_w, jitter, u, 0, 0, w0, b0, w1, b1, ray_start, ray_end, opts, out_feat,
                       out_depth, out_wsum, out_xyz, workspace, workspace_bytes, dumps, stream);
}

int p3d_render_rng_f32(const float* planes, int N, int H, int W, const float* rays_o, const float* rays_d, int64_t R, int ray_tile_w,
                       uint64_t seed, const float* w0, const float* b0, const float* w1, const float* b1, const float* ray_start,
                       const float* ray_end, const p3d_opts* opts, float* out_feat, float* out_depth, float* out_wsum, float* out_xyz,
                       void* workspace, size_t workspace_bytes, const p3d_dumps* dumps, void* stream) {
    return render_impl(planes, N, H, W, rays_o, rays_d, R, ray_tile_w, nullptr, nullptr, 1, seed, w0, b0, w1, b1, ray_start, ray_end, opts,
                       out_feat, out_depth, out_wsum, out_xyz, workspace, workspace_bytes, dumps, stream);
}

static int render_impl(const float* planes, int N, int H, int W, const float* rays_o, const float* rays_d, int64_t R,
                       int ray_tile_w, const float* jitter, const float* u, int rng, uint64_t seed, const float* w0, const float* b0,
                       const float* w1, const float* b1, const float* ray_start, const float* ray_end, const p3d_opts* opts,
                       float* out_feat, float* out_depth, float* out_wsum, float* out_xyz, void* workspace,
                       size_t workspace_bytes, const p3d_dumps* dumps, void* stream) {
    if ((ray_start == nullptr) != (ray_end == nullptr)) return P3D_E_ARG;  // both or neither
    if (!planes || !rays_o || !rays_d || (!jitter && !rng) || !w0 || !b0 || !w1 || !b1 || !opts || !out_feat || !out_depth ||
        !out_wsum || !out_xyz || !workspace || N <= 0 || R <= 0)
        return P3D_E_ARG;
    const int Sc = opts->Sc, Sf = opts->Sf;
    if (Sc < 4 || Sc > P3D_MAX_S || Sf < 0 || Sf > P3D_MAX_S) return P3D_E_RANGE;
    if (Sf > 0 && !u && !rng) return P3D_E_ARG;
    if (H <= 0 || W <= 0 || (long long)H * W * 128 * 3 >= 0x7ffffff0LL) return P3D_E_RANGE;
    if (workspace_bytes < p3d_render_plan_workspace_bytes(N)) return P3D_E_WORKSPACE;
    const RenderPlan pl = p3d_render_plan(N, R, ray_tile_w, *opts, dumps != nullptr, ray_start != nullptr);
    if (pl.err) return pl.err;
    hipStream_t st = (hipStream_t)stream;
    RenderParams p;
    p.planes = planes; p.rays_o = rays_o; p.rays_d = rays_d; p.jitter = jitter; p.u = u;
    p.rng = rng; p.seed_lo = (uint32_t)seed; p.seed_hi = (uint32_t)(seed >> 32);
    p.wide_rows = p3d_render_wide_rows(rng, jitter, u, Sc, Sf);
    p.serial_merge = (opts->flags & P3D_FLAG_SERIAL_MERGE) ? 1 : 0;
    p.w0 = w0; p.b0 = b0; p.w1 = w1; p.b1 = b1;
    p.out_feat = out_feat; p.out_depth = out_depth; p.out_wsum = out_wsum; p.out_xyz = out_xyz;
    p.gminmax = (uint32_t*)workspace;
    p.per_view_clamp = (opts->flags & P3D_FLAG_PER_VIEW_CLAMP) ? 1 : 0;
    if (dumps) p.dumps = *dumps; else memset(&p.dumps, 0, sizeof(p.dumps));
    p.R = R; p.H = H; p.W = W; p.Sc = Sc; p.Sf = Sf;
    p.ray_start = opts->ray_start; p.ray_end = opts->ray_end; p.depth_delta = opts->depth_delta;
    p.ray_start_arr = ray_start; p.ray_end_arr = ray_end;
    p.disparity = (opts->flags & P3D_FLAG_DISPARITY) ? 1 : 0;
    p.white_back = (opts->flags & P3D_FLAG_WHITE_BACK) ? 1 : 0;
    p.cfg = make_cfg(opts);
    p.tile_w = pl.tile_w; p.tiles_x = pl.tiles_x; p.tiles_per_img = pl.tiles_per_img; p.ntiles = pl.ntiles;
    p.lds_rows = pl.lds_rows; p.order = pl.order;
    const bool interior = p3d_render_plan_has_interior(pl) && p3d_render_interior_taps(H, W, *opts);  // which gather set-up k_render runs
    hipLaunchKernelGGL(k_minmax_init, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, p.gminmax, p.per_view_clamp ? N : 0);
    auto launch = [&](void (*kernel)(RenderParams)) {
        hipError_t e = p3d_ensure_dynamic_lds(kernel, pl.lds_bytes);
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL(kernel, dim3(pl.grid), dim3(pl.block), pl.lds_bytes, st, p);
        return p3d_check_launch();
    };
    const int rc = p3d_with_nf(pl.nf, [&](auto nfc) {
        constexpr int NF = decltype(nfc)::value;
        if constexpr (NF == 48 || NF == 96)
            if (pl.kernel == RenderKernel::SLOTS4_WO) return launch(k_render_slots<4, NF, true, true>);
        auto mode = [&](auto fc) {
            constexpr bool F = decltype(fc)::value;
            switch (pl.kernel) {
            case RenderKernel::DUMP: return launch(k_render<NF, true, F, false>);
            case RenderKernel::PLAIN: return launch(k_render<NF, false, F, false>);
            // (EARLY_TCG: NF == 96 only, the default TCG of that instantiation)
            case RenderKernel::EARLY_TCG: return interior ? launch(k_render<NF, false, F, true, p3d_render_tcg(NF, false, true), true>)
                                                          : launch(k_render<NF, false, F, true>);
            case RenderKernel::EARLY:
                if constexpr (p3d_render_nf_has_interior(NF, false))
                    if (interior) return launch(k_render<NF, false, F, true, false, true>);
                return launch(k_render<NF, false, F, true, false>);
            case RenderKernel::SLOTS2: return launch(k_render_slots<2, NF, F>);
            default: return launch(k_render_slots<4, NF, F>);  // SLOTS4 (SLOTS4_WO at NF = 48 / 96: above)
            }
        };
        return pl.fast ? mode(std::true_type()) : mode(std::false_type());
    });
    if (rc) return rc;
    long long NR = (long long)N * R;
    hipLaunchKernelGGL(k_render_finish, dim3((unsigned)((NR + 255) / 256)), dim3(256), 0, st, out_depth, NR, p.gminmax,
                       dumps ? dumps->tminmax : nullptr, p.per_view_clamp ? (long long)R : 0LL);
    return p3d_check_launch();
}

int p3d_sample_stratified_f32(float ray_start, float ray_end, float depth_delta, int S, const float* jitter, int64_t NR,
                              float* out, void* stream) {
    if (!jitter || !out || NR <= 0) return P3D_E_ARG;
    if (S < 2 || S > P3D_MAX_S) return P3D_E_RANGE;
    hipLaunchKernelGGL(k_stratified, dim3((unsigned)((NR + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ray_start,
                       ray_end, depth_delta, S, jitter, (long long)NR, out);
    return p3d_check_launch();
}

size_t p3d_composite_workspace_bytes(int64_t NR, int S, int K) {
    (void)NR; (void)S; (void)K;
    return 16;  // order-mapped global depth min / max (+ padding)
}

int p3d_depth_minmax_f32(const float* depths, int64_t n, float* out_minmax, void* workspace, size_t workspace_bytes, void* stream) {
    if (!depths || !out_minmax || !workspace || n <= 0) return P3D_E_ARG;
    if (workspace_bytes < 16) return P3D_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    uint32_t* g = (uint32_t*)workspace;
    hipLaunchKernelGGL(k_minmax_init, dim3(1), dim3(64), 0, st, g, 0);
    hipLaunchKernelGGL(k_depth_minmax, dim3(1024), dim3(256), 0, st, depths, (long long)n, g);
    hipLaunchKernelGGL(k_minmax_decode, dim3(1), dim3(1), 0, st, (const uint32_t*)g, out_minmax);
    return p3d_check_launch();
}

int p3d_composite_f32(const float* colors, const float* sigma, const float* depths, int64_t NR, int S, int K,
                      int white_back, float* out_rgb, float* out_depth, float* out_weights, void* workspace,
                      void* stream) {
    if (!colors || !sigma || !depths || !out_rgb || !out_depth || !workspace || NR <= 0) return P3D_E_ARG;
    if (S < 2 || K < 1 || K > 64) return P3D_E_RANGE;
    hipStream_t st = (hipStream_t)stream;
    uint32_t* g = (uint32_t*)workspace;
    hipLaunchKernelGGL(k_minmax_init, dim3(1), dim3(64), 0, st, g, 0);
    hipLaunchKernelGGL(k_depth_minmax, dim3(1024), dim3(256), 0, st, depths, (long long)NR * S, g);
    dim3 blk(8, 32);
    hipLaunchKernelGGL(k_composite, dim3((unsigned)((NR + 31) / 32)), blk, 0, st, colors, sigma, depths, (long long)NR, S,
                       K, white_back, out_rgb, out_depth, out_weights);
    hipLaunchKernelGGL(k_render_finish, dim3((unsigned)((NR + 255) / 256)), dim3(256), 0, st, out_depth, (long long)NR, g,
                       (float*)nullptr, 0LL);
    return p3d_check_launch();
}

int p3d_importance_f32(const float* depths, const float* weights, int64_t NR, int Sc, int Sf, const float* u,
                       float* out_depths, int32_t* out_inds, void* stream) {
    if (!depths || !weights || !u || !out_depths || NR <= 0) return P3D_E_ARG;
    if (Sc < 4 || Sc > P3D_MAX_S || Sf < 1) return P3D_E_RANGE;
    hipLaunchKernelGGL(k_importance, dim3((unsigned)((NR + 63) / 64)), dim3(64), 0, (hipStream_t)stream, depths, weights,
                       (long long)NR, Sc, Sf, u, out_depths, out_inds);
    return p3d_check_launch();
}

int p3d_unify_perm_f32(const float* tc, const float* tf, int64_t NR, int Sc, int Sf, int32_t* perm, void* stream) {
    if (!tc || !tf || !perm || NR <= 0) return P3D_E_ARG;
    if (Sc < 1 || Sf < 0) return P3D_E_RANGE;
    hipLaunchKernelGGL(k_unify_perm, dim3((unsigned)((NR + 63) / 64)), dim3(64), 0, (hipStream_t)stream, tc, tf,
                       (long long)NR, Sc, Sf, perm);
    return p3d_check_launch();
}

int p3d_sigma2density_f32(const float* sigma, const unsigned char* cropmask, int64_t M, float cull_thresh, float* out_density,
                          void* stream) {
    if (!sigma || !out_density || M <= 0) return P3D_E_ARG;
    const int vec = (((uintptr_t)sigma | (uintptr_t)out_density) & 15) == 0 && ((uintptr_t)cropmask & 3) == 0;
    hipLaunchKernelGGL(k_sigma2density, dim3((unsigned)((M + 1023) / 1024)), dim3(256), 0, (hipStream_t)stream, sigma, cropmask,
                       (long long)M, cull_thresh, out_density, vec);
    return p3d_check_launch();
}

}  // extern "C"
