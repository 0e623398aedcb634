// p3d_clip.hip — CLIP's ViT-B/32 image tower, clip's front end, the cosine and PSNR's reductions (include/p3d_clip.h).
//
//   k_clip_gemm<TM>    out = epi(A W): TM (64 or 32) rows x 64 columns per workgroup over K in chunks of 64, the next chunk's operands in
//                      flight in registers while the matrix cores work on this one (the loop of k_enc_conv; A is k-contiguous here, so
//                      its lanes run along k and it sits row-major in LDS at a pitch of 66 floats, which the MFMA reads without a bank
//                      conflict).  The linear workgroup id is dealt so that the row tiles of one weight slab share an XCD;
//   k_clip_reduce      the partial sums in ascending split order, then the epilogue: once, after the reduction;
//   k_clip_layernorm   one wave per row, two passes; <true>: the row is tok + pos[t] (the embedding step);
//   k_clip_attention   one (image, head, query block) per workgroup, the block's rows of Q and the head's K and V in LDS, one wave per
//                      query row;
//   k_clip_cosine      one wave per pair;
//   k_clip_resize_h/v  PIL's 8-bit bicubic resample as integer sums, horizontal then vertical through a uint8 workspace;
//   k_psnr_partial / k_psnr_final   sum of squared differences, minimum and maximum in one pass;
//   p3d_clip_forward_f32   walks a host table of step records: one C call per network.
// Every sum runs in a fixed order and nothing is accumulated with atomics: the results are bitwise reproducible for the same plan.
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "../../include/p3d_clip.h"
#include "p3d_clip_plan.hpp"

#define CL_WG 256
#define CL_KC P3D_CLIP_KC
#define CL_LDA (64 + 2)  // A rows in LDS: lanes (r, kq) of an MFMA read hit bank (2 r + kq) % 32, all different in a 32-lane half
#define CL_LDB (64 + 4)

typedef float cl_f32x4 __attribute__((ext_vector_type(4)));

struct ClipGemm {
    const float* a;
    const float* w;
    const float* bias;
    const float* res;
    float* out;
    float* ws;
    int M, K, Nout, gelu, split, cps, mt, nt, groups;
    int patch, S, G, T1;  // patch mode (patch > 0): G = S / patch patches per side, T1 = G * G per image
    int64_t total;        // M * Nout
};

// bias, QuickGELU, residual: the one place they are applied
__device__ __forceinline__ float cl_finish(const ClipGemm& c, float z, int n, int64_t idx) {
    float v = c.bias ? z + c.bias[n] : z;
    if (c.gelu) v = v * (1.0f / (1.0f + expf(-1.702f * v)));
    if (c.res) v = c.res[idx] + v;
    return v;
}

// Waves (wave >> 1, wave & 1): rows wm = (TM / 2)(wave >> 1), columns wn = 32 (wave & 1); TM / 32 x 2 blocks of v_mfma_f32_16x16x4_f32
// (A[l&15][k=l>>4], B[k=l>>4][l&15]; D col = l&15, row = 4*(l>>4) + r) per wave.
template <int TM>
__global__ __launch_bounds__(CL_WG) void k_clip_gemm(ClipGemm c) {
    constexpr int MI = TM / 32, RA = TM / 4;
    __shared__ float As[TM][CL_LDA];
    __shared__ float Bs[CL_KC][CL_LDB];
    // the deal: XCD = id % 8, place = id / 8; the mt row tiles of slab g take consecutive places of one XCD
    const int id = blockIdx.x, place = id >> 3;
    const int mi_tile = place % c.mt, g = (place / c.mt) * P3D_CLIP_XCDS + (id & 7);
    if (g >= c.groups) return;  // (the whole workgroup: no barrier has been reached)
    const int n0 = (g % c.nt) * 64, split = g / c.nt, m0 = mi_tile * TM;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = (wave >> 1) * (TM / 2), wn = (wave & 1) * 32;
    const int kbeg = split * c.cps * CL_KC;
    const int kend = min(c.K, kbeg + c.cps * CL_KC);
    // A: this lane stages element k = chunk + lane of rows m0 + wave + 4 j; B: column n0 + lane of rows chunk + wave + 4 j
    int rowbase[RA];
    unsigned rowin = 0;
#pragma unroll
    for (int j = 0; j < RA; ++j) {
        const int m = m0 + wave + 4 * j;
        const bool in = m < c.M;
        rowin |= (unsigned)in << j;
        if (c.patch > 0) {
            const int n = in ? m / c.T1 : 0, r = in ? m % c.T1 : 0;
            rowbase[j] = ((n * 3) * c.S + (r / c.G) * c.patch) * c.S + (r % c.G) * c.patch;
        } else {
            rowbase[j] = in ? m * c.K : 0;
        }
    }
    const bool n_in = n0 + lane < c.Nout;
    float ra[RA], rb[CL_KC / 4];
    unsigned pa = 0, pb = 0;
    int knext = kbeg;
    // fetch() only ISSUES loads — every one unconditional, from a clamped index (element 0 where the operand is out of range);
    // commit() applies the predicates as it writes the operands to LDS.
    auto fetch = [&]() {
        const int k = knext + lane;
        const bool kin = k < kend;
        int koff = k;
        if (c.patch > 0) {
            const int pp = c.patch * c.patch, ch = k / pp, rem = k % pp;
            koff = (ch * c.S + rem / c.patch) * c.S + rem % c.patch;
        }
        pa = kin ? rowin : 0u;
#pragma unroll
        for (int j = 0; j < RA; ++j) ra[j] = c.a[(pa >> j & 1) ? rowbase[j] + koff : 0];
        pb = 0;
#pragma unroll
        for (int j = 0; j < CL_KC / 4; ++j) {
            const int kb = knext + wave + 4 * j;
            const bool wb = kb < kend && n_in;
            rb[j] = c.w[wb ? (int64_t)kb * c.Nout + n0 + lane : 0];
            pb |= (unsigned)wb << j;
        }
        knext += CL_KC;
    };
    cl_f32x4 acc[MI][2];
#pragma unroll
    for (int u = 0; u < MI; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v) acc[u][v] = cl_f32x4{0.f, 0.f, 0.f, 0.f};
    fetch();
    for (int k0 = kbeg; k0 < kend; k0 += CL_KC) {
#pragma unroll
        for (int j = 0; j < RA; ++j) As[wave + 4 * j][lane] = (pa >> j & 1) ? ra[j] : 0.f;
#pragma unroll
        for (int j = 0; j < CL_KC / 4; ++j) Bs[wave + 4 * j][lane] = (pb >> j & 1) ? rb[j] : 0.f;
        __syncthreads();
        if (k0 + CL_KC < kend) fetch();
#pragma unroll
        for (int kk = 0; kk < CL_KC; kk += 4) {
            const int kr = kk + (lane >> 4), r = lane & 15;
            float a[MI];
#pragma unroll
            for (int mi = 0; mi < MI; ++mi) a[mi] = As[wm + 16 * mi + r][kr];
            const float b0 = Bs[kr][wn + r], b1 = Bs[kr][wn + 16 + r];
#pragma unroll
            for (int mi = 0; mi < MI; ++mi) {
                acc[mi][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mi], b0, acc[mi][0], 0, 0, 0);
                acc[mi][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mi], b1, acc[mi][1], 0, 0, 0);
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
            const int n = n0 + wn + 16 * ni + (lane & 15);
            if (n >= c.Nout) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + wm + 16 * mi + 4 * (lane >> 4) + r;
                if (m >= c.M) continue;
                const int64_t idx = (int64_t)m * c.Nout + n;
                if (c.split == 1) c.out[idx] = cl_finish(c, acc[mi][ni][r], n, idx);
                else c.ws[(int64_t)split * c.total + idx] = acc[mi][ni][r];
            }
        }
}

__global__ __launch_bounds__(CL_WG) void k_clip_reduce(ClipGemm c) {
    const int64_t i = (int64_t)blockIdx.x * CL_WG + threadIdx.x;
    if (i >= c.total) return;
    float z = c.ws[i];
    for (int s = 1; s < c.split; ++s) z = z + c.ws[(int64_t)s * c.total + i];
    c.out[i] = cl_finish(c, z, (int)(i % c.Nout), i);
}

// the butterfly of "the wave tree" (include/p3d_clip.h)
__device__ __forceinline__ float cl_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = v + __shfl_xor(v, o, 64);
    return v;
}

template <bool EMBED>
__global__ __launch_bounds__(CL_WG) void k_clip_layernorm(const float* __restrict__ x, int M, int D, int64_t ldx, const float* __restrict__ cls,
                                                          const float* __restrict__ pos, int T, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, float eps, float* __restrict__ y) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;  // (no barrier below)
    const float* xr;
    const float* pr = nullptr;
    if (EMBED) {
        const int n = row / T, t = row % T;
        xr = t == 0 ? cls : x + ((int64_t)n * (T - 1) + (t - 1)) * D;
        pr = pos + (int64_t)t * D;
    } else {
        xr = x + (int64_t)row * ldx;
    }
    auto at = [&](int d) { return EMBED ? xr[d] + pr[d] : xr[d]; };
    float s = 0.f;
    for (int d = lane; d < D; d += 64) s = s + at(d);
    const float mean = cl_wave_sum(s) / (float)D;
    float q = 0.f;
    for (int d = lane; d < D; d += 64) {
        const float e = at(d) - mean;
        q = q + e * e;
    }
    const float var = cl_wave_sum(q) / (float)D;
    const float r = 1.0f / __builtin_sqrtf(var + eps);
    float* yr = y + (int64_t)row * D;
    for (int d = lane; d < D; d += 64) yr[d] = ((at(d) - mean) * r) * gamma[d] + beta[d];
}

__global__ __launch_bounds__(CL_WG) void k_clip_attention(const float* __restrict__ qkv, int T, int heads, int D, int rows,
                                                          float* __restrict__ out) {
    __shared__ float Qs[P3D_CLIP_MAX_T][64];
    __shared__ float Ks[P3D_CLIP_MAX_T][65];
    __shared__ float Vs[P3D_CLIP_MAX_T][64];
    __shared__ float Ps[4][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = blockIdx.x / heads, h = blockIdx.x % heads;
    const int r0 = blockIdx.y * rows, r1 = min(T, r0 + rows);
    const float* base = qkv + (int64_t)n * T * 3 * D + 64 * h;
    for (int i = tid; i < T * 64; i += CL_WG) {
        const int j = i >> 6, ch = i & 63;
        const float* row = base + (int64_t)j * 3 * D;
        if (j >= r0 && j < r1) Qs[j - r0][ch] = row[ch];  // (only this block's query rows)
        Ks[j][ch] = row[D + ch];
        Vs[j][ch] = row[2 * D + ch];
    }
    __syncthreads();
    for (int it = r0; it < r1; it += 4) {  // (the same trip count for the four waves: the barriers below are uniform)
        const int i = it + wave;
        const bool live = i < r1;
        float s = -__builtin_inff();
        if (live && lane < T) {
            float acc = 0.f;
#pragma unroll 16
            for (int ch = 0; ch < 64; ++ch) acc = __builtin_fmaf(Qs[i - r0][ch], Ks[lane][ch], acc);
            s = 0.125f * acc;
        }
        float m = s;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) m = __builtin_fmaxf(m, __shfl_xor(m, o, 64));
        Ps[wave][lane] = (live && lane < T) ? expf(s - m) : 0.f;
        __syncthreads();
        if (live) {
            float l = 0.f, acc = 0.f;
            for (int j = 0; j < T; ++j) {
                const float p = Ps[wave][j];
                l = l + p;
                acc = __builtin_fmaf(p, Vs[j][lane], acc);
            }
            out[((int64_t)n * T + i) * D + 64 * h + lane] = acc / l;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(CL_WG) void k_clip_cosine(const float* __restrict__ a, const float* __restrict__ b, int pairs, int D,
                                                       float* __restrict__ sim) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= pairs) return;
    const float* ar = a + (int64_t)row * D;
    const float* br = b + (int64_t)row * D;
    float dot = 0.f, aa = 0.f, bb = 0.f;
    for (int d = lane; d < D; d += 64) {
        const float u = ar[d], v = br[d];
        dot = __builtin_fmaf(u, v, dot);
        aa = __builtin_fmaf(u, u, aa);
        bb = __builtin_fmaf(v, v, bb);
    }
    dot = cl_wave_sum(dot), aa = cl_wave_sum(aa), bb = cl_wave_sum(bb);
    if (lane == 0) sim[row] = dot / (__builtin_sqrtf(aa) * __builtin_sqrtf(bb));
}

// ---- the front end ----------------------------------------------------------------------------------------------------------------
struct ClipPrep {
    const float* img;
    const int32_t* tabx;
    const int32_t* taby;
    unsigned char* tmp;
    float* out;
    int N, C, H, W, S, ksx, ksy, row_lo, rows;
};

__device__ __forceinline__ int cl_clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// tmp[n][c][y - row_lo][x] for the kept columns x < S and the source rows row_lo <= y < row_lo + rows
__global__ __launch_bounds__(CL_WG) void k_clip_resize_h(ClipPrep p) {
    const int64_t i = (int64_t)blockIdx.x * CL_WG + threadIdx.x;
    if (i >= (int64_t)p.N * 3 * p.rows * p.S) return;
    const int x = (int)(i % p.S), y = (int)((i / p.S) % p.rows), pl = (int)(i / ((int64_t)p.S * p.rows));
    const int32_t* rec = p.tabx + (int64_t)x * (2 + p.ksx);
    const int xmin = min(max(rec[0], 0), p.W - 1);
    const int n = min(min(max(rec[1], 0), p.ksx), p.W - xmin);
    const float* src = p.img + (((int64_t)(pl / 3) * p.C + pl % 3) * p.H + p.row_lo + y) * p.W + xmin;
    int ss = 1 << 21;
    for (int t = 0; t < n; ++t) {
        const float v = __builtin_fminf(__builtin_fmaxf(src[t], 0.f), 1.f) * 255.f;
        ss += rec[2 + t] * (int)__builtin_floorf(v);
    }
    p.tmp[i] = (unsigned char)cl_clip8(ss >> 22);
}

__global__ __launch_bounds__(CL_WG) void k_clip_resize_v(ClipPrep p, float m0, float m1, float m2, float s0, float s1, float s2) {
    const int64_t i = (int64_t)blockIdx.x * CL_WG + threadIdx.x;
    if (i >= (int64_t)p.N * 3 * p.S * p.S) return;
    const int x = (int)(i % p.S), y = (int)((i / p.S) % p.S), pl = (int)(i / ((int64_t)p.S * p.S));
    const int32_t* rec = p.taby + (int64_t)y * (2 + p.ksy);
    const int ymin = min(max(rec[0] - p.row_lo, 0), p.rows - 1);
    const int n = min(min(max(rec[1], 0), p.ksy), p.rows - ymin);
    const unsigned char* src = p.tmp + ((int64_t)pl * p.rows + ymin) * p.S + x;
    int ss = 1 << 21;
    for (int t = 0; t < n; ++t) ss += rec[2 + t] * (int)src[(int64_t)t * p.S];
    const int ch = pl % 3;
    const float mean = ch == 0 ? m0 : (ch == 1 ? m1 : m2), sd = ch == 0 ? s0 : (ch == 1 ? s1 : s2);
    p.out[i] = ((float)cl_clip8(ss >> 22) / 255.f - mean) / sd;
}

// ---- PSNR -------------------------------------------------------------------------------------------------------------------------
// the workgroup's value of (sum, min, max): each wave's butterfly, then the four waves ascending; valid in thread 0
__device__ __forceinline__ void cl_block3(float& s, float& mn, float& mx) {
    __shared__ float red[3][4];
    s = cl_wave_sum(s);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        mn = __builtin_fminf(mn, __shfl_xor(mn, o, 64));
        mx = __builtin_fmaxf(mx, __shfl_xor(mx, o, 64));
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) red[0][wave] = s, red[1][wave] = mn, red[2][wave] = mx;
    __syncthreads();
    s = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
    mn = __builtin_fminf(__builtin_fminf(red[1][0], red[1][1]), __builtin_fminf(red[1][2], red[1][3]));
    mx = __builtin_fmaxf(__builtin_fmaxf(red[2][0], red[2][1]), __builtin_fmaxf(red[2][2], red[2][3]));
}

__global__ __launch_bounds__(CL_WG) void k_psnr_partial(const float* __restrict__ pred, const float* __restrict__ target, int64_t count,
                                                        float* __restrict__ ws) {
    const int B = gridDim.x;
    float s = 0.f, mn = __builtin_inff(), mx = -__builtin_inff();
    for (int64_t i = (int64_t)blockIdx.x * CL_WG + threadIdx.x; i < count; i += (int64_t)B * CL_WG) {
        const float t = target[i], d = pred[i] - t;
        s = __builtin_fmaf(d, d, s);
        mn = __builtin_fminf(mn, t), mx = __builtin_fmaxf(mx, t);
    }
    cl_block3(s, mn, mx);
    if (threadIdx.x == 0) ws[blockIdx.x] = s, ws[B + blockIdx.x] = mn, ws[2 * B + blockIdx.x] = mx;
}

__global__ __launch_bounds__(CL_WG) void k_psnr_final(const float* __restrict__ ws, int B, float* __restrict__ out3) {
    float s = 0.f, mn = __builtin_inff(), mx = -__builtin_inff();
    for (int b = threadIdx.x; b < B; b += CL_WG) {
        s = s + ws[b];
        mn = __builtin_fminf(mn, ws[B + b]), mx = __builtin_fmaxf(mx, ws[2 * B + b]);
    }
    cl_block3(s, mn, mx);
    if (threadIdx.x == 0) out3[0] = s, out3[1] = mn, out3[2] = mx;
}

// ---- entry points -----------------------------------------------------------------------------------------------------------------
extern "C" int p3d_clip_resize_plan(int H, int W, int S, int* out8) {
    if (!out8) return P3D_E_ARG;
    ClipResize r;
    const int rc = clip_resize_plan(H, W, S, &r);
    if (rc) return rc;
    out8[0] = r.h, out8[1] = r.w, out8[2] = r.offy, out8[3] = r.offx, out8[4] = r.ksy, out8[5] = r.ksx, out8[6] = r.row_lo, out8[7] = r.row_hi;
    return 0;
}

extern "C" int p3d_clip_resize_table(int in, int out, int first, int count, int ksize, int32_t* tab) {
    return clip_resize_table(in, out, first, count, ksize, tab);
}

static int cl_prepare_check(int N, int C, int H, int W, int S, ClipResize* r, size_t* need) {
    *need = 0;
    if (N <= 0 || C <= 0) return P3D_E_ARG;
    const int rc = clip_resize_plan(H, W, S, r);
    if (rc) return rc;
    if (C < 3) return P3D_E_RANGE;
    const int64_t lim = 0x7fffffff;
    if ((int64_t)N * C * H * W >= lim * 64 || (int64_t)N * 3 * (r->row_hi - r->row_lo) * S >= lim || (int64_t)N * 3 * S * S >= lim) return P3D_E_RANGE;
    *need = clip_prepare_workspace(N, *r, S);
    return 0;
}

extern "C" size_t p3d_clip_prepare_workspace_bytes(int N, int H, int W, int S) {
    ClipResize r;
    size_t need;
    return cl_prepare_check(N, 3, H, W, S, &r, &need) ? 0 : need;
}

static int cl_prepare_launch(const float* img, int N, int C, int H, int W, int S, const int32_t* tabx, const int32_t* taby, float* out,
                             const ClipResize& r, void* workspace, hipStream_t s) {
    ClipPrep p;
    p.img = img, p.tabx = tabx, p.taby = taby, p.tmp = (unsigned char*)workspace, p.out = out;
    p.N = N, p.C = C, p.H = H, p.W = W, p.S = S, p.ksx = r.ksx, p.ksy = r.ksy, p.row_lo = r.row_lo, p.rows = r.row_hi - r.row_lo;
    const int64_t n1 = (int64_t)N * 3 * p.rows * S, n2 = (int64_t)N * 3 * S * S;
    hipLaunchKernelGGL(k_clip_resize_h, dim3((unsigned)((n1 + CL_WG - 1) / CL_WG)), dim3(CL_WG), 0, s, p);
    hipLaunchKernelGGL(k_clip_resize_v, dim3((unsigned)((n2 + CL_WG - 1) / CL_WG)), dim3(CL_WG), 0, s, p, 0.48145466f, 0.4578275f, 0.40821073f,
                       0.26862954f, 0.26130258f, 0.27577711f);
    return (int)hipGetLastError();
}

extern "C" int p3d_clip_prepare_f32(const float* img, int N, int C, int H, int W, int S, const int32_t* tabx, const int32_t* taby, float* out,
                                    void* workspace, size_t workspace_bytes, void* stream) {
    if (!img || !tabx || !taby || !out || !workspace) return P3D_E_ARG;
    ClipResize r;
    size_t need;
    const int rc = cl_prepare_check(N, C, H, W, S, &r, &need);
    if (rc) return rc;
    if (workspace_bytes < need) return P3D_E_WORKSPACE;
    return cl_prepare_launch(img, N, C, H, W, S, tabx, taby, out, r, workspace, (hipStream_t)stream);
}

extern "C" int p3d_clip_gemm_plan(int M, int K, int Nout, int force_plan, int* out4) {
    ClipPlan p;
    const int rc = clip_gemm_plan(M, K, Nout, force_plan, &p);
    if (rc) return rc;
    if (out4) out4[0] = p.tile, out4[1] = p.split, out4[2] = p.cps, out4[3] = (int)p.wgs;
    return (p.tile << 8) | p.split;
}

extern "C" size_t p3d_clip_gemm_workspace_bytes(int M, int K, int Nout, int force_plan) {
    ClipPlan p;
    if (clip_gemm_plan(M, K, Nout, force_plan, &p)) return 0;
    return clip_gemm_workspace(p, M, Nout);
}

// the checks of one GEMM: flags, sizes, the patch mode's restatements, plan
static int cl_gemm_check(int M, int K, int Nout, int flags, int N, int S, int patch, int force_plan, ClipPlan* p, size_t* need) {
    *need = 0;
    if (flags & ~(P3D_CLIP_GELU | P3D_CLIP_PATCH)) return P3D_E_RANGE;
    const int rc = clip_gemm_plan(M, K, Nout, force_plan, p);
    if (rc) return rc;
    if (flags & P3D_CLIP_PATCH) {
        if (N <= 0 || S <= 0 || patch <= 0) return P3D_E_ARG;
        if (S > P3D_CLIP_MAX_S || S % patch) return P3D_E_RANGE;
        const int64_t G = S / patch;
        if ((int64_t)N * G * G != M || (int64_t)3 * patch * patch != K || (int64_t)N * 3 * S * S >= 0x7fffffff) return P3D_E_RANGE;
    } else if (N || S || patch) {
        return P3D_E_RANGE;
    }
    *need = clip_gemm_workspace(*p, M, Nout);
    if (p->split > 1 && ((int64_t)M * Nout + CL_WG - 1) / CL_WG > 0x7fffffff) return P3D_E_RANGE;
    return 0;
}

static int cl_gemm_launch(const float* a, int M, int K, const float* w, int Nout, const float* bias, const float* res, int flags, int S,
                          int patch, float* out, const ClipPlan& p, void* workspace, hipStream_t s) {
    ClipGemm c;
    c.a = a, c.w = w, c.bias = bias, c.res = res, c.out = out, c.ws = (float*)workspace;
    c.M = M, c.K = K, c.Nout = Nout, c.gelu = (flags & P3D_CLIP_GELU) != 0, c.split = p.split, c.cps = p.cps, c.mt = p.mt, c.nt = p.nt;
    c.groups = p.nt * p.split;
    c.patch = (flags & P3D_CLIP_PATCH) ? patch : 0, c.S = S, c.G = c.patch ? S / patch : 1, c.T1 = c.G * c.G;
    c.total = (int64_t)M * Nout;
    if (p.tm == 64) hipLaunchKernelGGL(k_clip_gemm<64>, dim3((unsigned)p.grid), dim3(CL_WG), 0, s, c);
    else hipLaunchKernelGGL(k_clip_gemm<32>, dim3((unsigned)p.grid), dim3(CL_WG), 0, s, c);
    if (p.split > 1) hipLaunchKernelGGL(k_clip_reduce, dim3((unsigned)((c.total + CL_WG - 1) / CL_WG)), dim3(CL_WG), 0, s, c);
    return (int)hipGetLastError();
}

extern "C" int p3d_clip_gemm_f32(const float* a, int M, int K, const float* w, int Nout, const float* bias, const float* res, int flags, int N,
                                 int S, int patch, float* out, int force_plan, void* workspace, size_t workspace_bytes, void* stream) {
    if (!a || !w || !out) return P3D_E_ARG;
    ClipPlan p;
    size_t need;
    const int rc = cl_gemm_check(M, K, Nout, flags, N, S, patch, force_plan, &p, &need);
    if (rc) return rc;
    if (need && !workspace) return P3D_E_ARG;
    if (workspace_bytes < need) return P3D_E_WORKSPACE;
    return cl_gemm_launch(a, M, K, w, Nout, bias, res, flags, S, patch, out, p, workspace, (hipStream_t)stream);
}

static int cl_ln_check(int M, int D, int64_t ldx, float eps) {
    if (M <= 0 || D <= 0) return P3D_E_ARG;
    if (ldx < D || !(eps >= 0.f) || (int64_t)M * D >= 0x7fffffff || ldx > ((int64_t)1 << 40) / M) return P3D_E_RANGE;
    return 0;
}

extern "C" int p3d_clip_layernorm_f32(const float* x, int M, int D, int64_t ldx, const float* gamma, const float* beta, float eps, float* y,
                                      void* stream) {
    if (!x || !gamma || !beta || !y) return P3D_E_ARG;
    const int rc = cl_ln_check(M, D, ldx, eps);
    if (rc) return rc;
    hipLaunchKernelGGL(k_clip_layernorm<false>, dim3((unsigned)((M + 3) / 4)), dim3(CL_WG), 0, (hipStream_t)stream, x, M, D, ldx,
                       (const float*)nullptr, (const float*)nullptr, 1, gamma, beta, eps, y);
    return (int)hipGetLastError();
}

static int cl_embed_check(int N, int T, int D, float eps) {
    if (N <= 0 || T <= 0 || D <= 0) return P3D_E_ARG;
    if ((int64_t)N * T >= 0x7fffffff / D) return P3D_E_RANGE;
    return cl_ln_check(N * T, D, D, eps);
}

extern "C" int p3d_clip_embed_f32(const float* patches, const float* cls, const float* pos, int N, int T, int D, const float* gamma,
                                  const float* beta, float eps, float* y, void* stream) {
    if (!cls || !pos || !gamma || !beta || !y || (!patches && T > 1)) return P3D_E_ARG;
    const int rc = cl_embed_check(N, T, D, eps);
    if (rc) return rc;
    hipLaunchKernelGGL(k_clip_layernorm<true>, dim3((unsigned)((N * T + 3) / 4)), dim3(CL_WG), 0, (hipStream_t)stream, patches, N * T, D,
                       (int64_t)D, cls, pos, T, gamma, beta, eps, y);
    return (int)hipGetLastError();
}

extern "C" int p3d_clip_attention_plan(int N, int T, int heads, int* out4) {
    if (!out4) return P3D_E_ARG;
    ClipAttnPlan p;
    const int rc = clip_attn_plan(N, T, heads, &p);
    if (rc) return rc;
    out4[0] = (int)p.wgs, out4[1] = p.qblocks, out4[2] = p.rows, out4[3] = p.lds_bytes;
    return 0;
}

static int cl_attn_check(int N, int T, int heads, int D, ClipAttnPlan* p) {
    const int rc = clip_attn_plan(N, T, heads, p);
    if (rc) return rc;
    if (D <= 0) return P3D_E_ARG;
    return D == P3D_CLIP_HEAD_DIM * heads ? 0 : P3D_E_RANGE;
}

static int cl_attn_launch(const float* qkv, int N, int T, int heads, int D, float* out, const ClipAttnPlan& p, hipStream_t s) {
    hipLaunchKernelGGL(k_clip_attention, dim3((unsigned)(N * heads), (unsigned)p.qblocks), dim3(CL_WG), 0, s, qkv, T, heads, D, p.rows, out);
    return (int)hipGetLastError();
}

extern "C" int p3d_clip_attention_f32(const float* qkv, int N, int T, int heads, int D, float* out, void* stream) {
    if (!qkv || !out) return P3D_E_ARG;
    ClipAttnPlan p;
    const int rc = cl_attn_check(N, T, heads, D, &p);
    if (rc) return rc;
    return cl_attn_launch(qkv, N, T, heads, D, out, p, (hipStream_t)stream);
}

extern "C" int p3d_clip_cosine_f32(const float* a, const float* b, int pairs, int D, float* sim, void* stream) {
    if (!a || !b || !sim || pairs <= 0 || D <= 0) return P3D_E_ARG;
    if ((int64_t)pairs * D >= 0x7fffffff) return P3D_E_RANGE;
    hipLaunchKernelGGL(k_clip_cosine, dim3((unsigned)((pairs + 3) / 4)), dim3(CL_WG), 0, (hipStream_t)stream, a, b, pairs, D, sim);
    return (int)hipGetLastError();
}

extern "C" size_t p3d_psnr_workspace_bytes(int64_t count) { return count > 0 ? (size_t)3 * clip_psnr_blocks(count) * sizeof(float) : 0; }

extern "C" int p3d_psnr_f32(const float* pred, const float* target, int64_t count, float* out3, void* workspace, size_t workspace_bytes,
                            void* stream) {
    if (!pred || !target || !out3 || !workspace || count <= 0) return P3D_E_ARG;
    if (count > ((int64_t)1 << 40)) return P3D_E_RANGE;
    if (workspace_bytes < p3d_psnr_workspace_bytes(count)) return P3D_E_WORKSPACE;
    const int B = clip_psnr_blocks(count);
    hipLaunchKernelGGL(k_psnr_partial, dim3((unsigned)B), dim3(CL_WG), 0, (hipStream_t)stream, pred, target, count, (float*)workspace);
    hipLaunchKernelGGL(k_psnr_final, dim3(1), dim3(CL_WG), 0, (hipStream_t)stream, (const float*)workspace, B, out3);
    return (int)hipGetLastError();
}

extern "C" int p3d_clip_struct_layout(size_t* out, int cap) {
    if (!out || cap <= 0) return P3D_E_ARG;
    int n = 0;
#define CL_PUT(v) do { if (n >= cap) return P3D_E_RANGE; out[n++] = (size_t)(v); } while (0)
#define CL_OFF(f) CL_PUT(offsetof(p3d_clip_step, f))
    CL_PUT(sizeof(p3d_clip_step));
    CL_OFF(kind); CL_OFF(M); CL_OFF(K); CL_OFF(Nout); CL_OFF(N); CL_OFF(T); CL_OFF(heads); CL_OFF(S); CL_OFF(patch); CL_OFF(H); CL_OFF(W);
    CL_OFF(ld); CL_OFF(in); CL_OFF(out); CL_OFF(res); CL_OFF(flags); CL_OFF(plan); CL_OFF(eps); CL_OFF(reserved); CL_OFF(w_off);
    CL_OFF(b_off); CL_OFF(w2_off); CL_OFF(b2_off);
#undef CL_OFF
#undef CL_PUT
    return n;
}

// One record against the table's buffers and blob.  launch == false: the checks alone (*need: the workspace the record asks for).
static int cl_step(const p3d_clip_step& t, const float* weights, int64_t weight_floats, float* arena, const int64_t* buf_off,
                   const int64_t* buf_len, int n_bufs, void* workspace, bool launch, size_t* need, hipStream_t s) {
    *need = 0;
    if (t.in < 0 || t.in >= n_bufs || t.out < 0 || t.out >= n_bufs || t.in == t.out || t.reserved[0] || t.reserved[1]) return P3D_E_RANGE;
    const bool gemm = t.kind == P3D_CLIP_KIND_GEMM;
    if (t.res < -1 || t.res >= n_bufs || t.res == t.in || (!gemm && (t.res != -1 || t.flags || t.plan))) return P3D_E_RANGE;
    const float* x = arena ? arena + buf_off[t.in] : nullptr;
    float* y = arena ? arena + buf_off[t.out] : nullptr;
    auto fits = [&](int b, int64_t n) { return !buf_len || n <= buf_len[b]; };
    auto blob = [&](int64_t off, int64_t n) { return off >= 0 && n <= weight_floats && off <= weight_floats - n; };
    const bool zero_img = !t.H && !t.W, zero_tok = !t.N && !t.T && !t.heads, zero_patch = !t.S && !t.patch;
    if (gemm) {
        ClipPlan p;
        const int rc = cl_gemm_check(t.M, t.K, t.Nout, t.flags, t.N, t.S, t.patch, t.plan, &p, need);
        if (rc) return rc;
        if (t.T || t.heads || !zero_img || t.ld || t.w2_off || t.b2_off || t.b_off < -1) return P3D_E_RANGE;
        const int64_t n_in = (t.flags & P3D_CLIP_PATCH) ? (int64_t)t.N * 3 * t.S * t.S : (int64_t)t.M * t.K, n_out = (int64_t)t.M * t.Nout;
        if (!fits(t.in, n_in) || !fits(t.out, n_out) || (t.res >= 0 && !fits(t.res, n_out))) return P3D_E_RANGE;
        if (!blob(t.w_off, (int64_t)t.K * t.Nout) || (t.b_off >= 0 && !blob(t.b_off, t.Nout))) return P3D_E_RANGE;
        if (!launch) return 0;
        return cl_gemm_launch(x, t.M, t.K, weights + t.w_off, t.Nout, t.b_off >= 0 ? weights + t.b_off : nullptr,
                              t.res >= 0 ? arena + buf_off[t.res] : nullptr, t.flags, t.S, t.patch, y, p, workspace, s);
    }
    if (t.kind == P3D_CLIP_KIND_LAYERNORM) {
        const int rc = cl_ln_check(t.M, t.K, t.ld, t.eps);
        if (rc) return rc;
        if (t.Nout != t.K || !zero_tok || !zero_patch || !zero_img || t.w2_off || t.b2_off) return P3D_E_RANGE;
        if (!fits(t.in, (int64_t)(t.M - 1) * t.ld + t.K) || !fits(t.out, (int64_t)t.M * t.K)) return P3D_E_RANGE;
        if (!blob(t.w_off, t.K) || !blob(t.b_off, t.K)) return P3D_E_RANGE;
        if (!launch) return 0;
        hipLaunchKernelGGL(k_clip_layernorm<false>, dim3((unsigned)((t.M + 3) / 4)), dim3(CL_WG), 0, s, x, t.M, t.K, (int64_t)t.ld,
                           (const float*)nullptr, (const float*)nullptr, 1, weights + t.w_off, weights + t.b_off, t.eps, y);
        return (int)hipGetLastError();
    }
    if (t.kind == P3D_CLIP_KIND_EMBED) {
        const int rc = cl_embed_check(t.N, t.T, t.K, t.eps);
        if (rc) return rc;
        if (t.M != t.N * t.T || t.Nout != t.K || t.heads || !zero_patch || !zero_img || t.ld) return P3D_E_RANGE;
        if (!fits(t.in, (int64_t)t.N * (t.T - 1) * t.K) || !fits(t.out, (int64_t)t.M * t.K)) return P3D_E_RANGE;
        if (!blob(t.w_off, t.K) || !blob(t.b_off, t.K) || !blob(t.w2_off, t.K) || !blob(t.b2_off, (int64_t)t.T * t.K)) return P3D_E_RANGE;
        if (!launch) return 0;
        hipLaunchKernelGGL(k_clip_layernorm<true>, dim3((unsigned)((t.M + 3) / 4)), dim3(CL_WG), 0, s, x, t.M, t.K, (int64_t)t.K,
                           weights + t.w2_off, weights + t.b2_off, t.T, weights + t.w_off, weights + t.b_off, t.eps, y);
        return (int)hipGetLastError();
    }
    if (t.kind == P3D_CLIP_KIND_ATTENTION) {
        ClipAttnPlan p;
        const int rc = cl_attn_check(t.N, t.T, t.heads, t.Nout, &p);
        if (rc) return rc;
        if (t.M != t.N * t.T || t.K != 3 * t.Nout || !zero_patch || !zero_img || t.ld || t.w_off || t.b_off || t.w2_off || t.b2_off) return P3D_E_RANGE;
        if (!fits(t.in, (int64_t)t.M * t.K) || !fits(t.out, (int64_t)t.M * t.Nout)) return P3D_E_RANGE;
        if (!launch) return 0;
        return cl_attn_launch(x, t.N, t.T, t.heads, t.Nout, y, p, s);
    }
    if (t.kind == P3D_CLIP_KIND_PREPARE) {
        ClipResize r;
        const int rc = cl_prepare_check(t.N, t.K, t.H, t.W, t.S, &r, need);
        if (rc) return rc;
        if (t.M != t.N || t.Nout != 3 || t.T || t.heads || t.patch || t.ld || t.w2_off || t.b2_off) return P3D_E_RANGE;
        if (!fits(t.in, (int64_t)t.N * t.K * t.H * t.W) || !fits(t.out, (int64_t)t.N * 3 * t.S * t.S)) return P3D_E_RANGE;
        if (!blob(t.w_off, (int64_t)t.S * (2 + r.ksx)) || !blob(t.b_off, (int64_t)t.S * (2 + r.ksy))) return P3D_E_RANGE;
        if (!launch) return 0;
        return cl_prepare_launch(x, t.N, t.K, t.H, t.W, t.S, (const int32_t*)(weights + t.w_off), (const int32_t*)(weights + t.b_off), y, r,
                                 workspace, s);
    }
    return P3D_E_RANGE;
}

extern "C" size_t p3d_clip_workspace_bytes(const p3d_clip_step* steps, int n_steps) {
    if (!steps || n_steps <= 0) return 0;
    size_t most = 0;
    for (int i = 0; i < n_steps; ++i) {
        size_t need;
        // (no buffers here: indices are checked against a table as large as the indices ask for)
        if (cl_step(steps[i], nullptr, (int64_t)1 << 62, nullptr, nullptr, nullptr, 0x7fffffff, nullptr, false, &need, nullptr)) return 0;
        if (need > most) most = need;
    }
    return most;
}

extern "C" int p3d_clip_forward_f32(const p3d_clip_step* steps, int n_steps, const float* weights, int64_t weight_floats, float* arena,
                                    int64_t arena_floats, const int64_t* buf_off, const int64_t* buf_len, int n_bufs, void* workspace,
                                    size_t workspace_bytes, void* stream) {
    if (!steps || !weights || !arena || !buf_off || !buf_len) return P3D_E_ARG;
    if (n_steps <= 0 || weight_floats <= 0 || arena_floats <= 0 || n_bufs <= 0) return P3D_E_ARG;
    for (int b = 0; b < n_bufs; ++b)
        if (buf_off[b] < 0 || buf_len[b] < 0 || buf_len[b] > arena_floats || buf_off[b] > arena_floats - buf_len[b]) return P3D_E_RANGE;
    size_t most = 0;
    for (int i = 0; i < n_steps; ++i) {  // every record, before any launch
        size_t need;
        const int rc = cl_step(steps[i], weights, weight_floats, arena, buf_off, buf_len, n_bufs, workspace, false, &need, nullptr);
        if (rc) return rc;
        if (need > most) most = need;
    }
    if (most && !workspace) return P3D_E_ARG;
    if (most > workspace_bytes) return P3D_E_WORKSPACE;
    for (int i = 0; i < n_steps; ++i) {
        size_t need;
        const int rc = cl_step(steps[i], weights, weight_floats, arena, buf_off, buf_len, n_bufs, workspace, true, &need, (hipStream_t)stream);
        if (rc) return rc;
    }
    return 0;
}
