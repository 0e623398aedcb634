// p3d_encoder.hip — the conditioning encoder's layers (include/p3d_encoder.h).
//
//   k_enc_conv<TM>     convolution with folded batch norm: an implicit GEMM of TM (64 or 32) output channels x 64 output pixels per
//                      workgroup — the pixel axis runs over ALL samples, so two 8 x 8 maps are two full tiles — over K = (tap, input
//                      channel) flattened, in chunks of 64 consecutive pairs, the next chunk's operands in flight in registers while
//                      the matrix cores work on this one.  blockIdx.z is the split: a contiguous range of chunks.  Without a split
//                      the kernel finishes its values (bias, residual, ReLU); with one it stores the partial sums;
//   k_enc_reduce       the partial sums in ascending split order, then bias, residual, ReLU: once, after the reduction;
//   k_enc_maxpool      3 x 3 stride-2 maximum, padding 1 as -infinity;
//   k_enc_prepare      bilinear resize + normalisation of the image and of its mirror, one launch;
//   p3d_encoder_forward_f32   walks a host table of layer records: one C call per network.
// Every sum runs in a fixed order and nothing is accumulated with atomics: the results are bitwise reproducible for the same plan.
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "../../include/p3d_encoder.h"
#include "p3d_encoder_plan.hpp"

#define EN_WG 256          // four waves
#define EN_KC P3D_ENC_KC   // K staged through LDS at a time; sixteen operands per lane in flight meanwhile
#define EN_PX 64           // output pixels per workgroup
#define EN_LD (64 + 4)     // LDS row pitch in floats

typedef float en_f32x4 __attribute__((ext_vector_type(4)));

struct EncConv {
    const float* x;
    const float* wk;
    const float* bias;
    const float* res;
    float* out;
    float* ws;
    int Ci, H, W, k, Co, Ho, Wo, stride, pad;
    int K;          // k * k * Ci
    int P;          // N * Ho * Wo
    int relu, split, cps;
    int64_t total;  // N * Co * Ho * Wo
};

// bias, residual, ReLU: the one place they are applied
__device__ __forceinline__ float en_finish(const EncConv& c, float z, int co, int64_t idx) {
    float v = z + c.bias[co];
    if (c.res) v = v + c.res[idx];
    return c.relu ? __builtin_fmaxf(v, 0.f) : v;
}

// Waves (wave >> 1, wave & 1): rows wm = (TM / 2)(wave >> 1), columns wn = 32 (wave & 1); TM / 32 x 2 blocks of v_mfma_f32_16x16x4_f32
// (A[l&15][k=l>>4], B[k=l>>4][l&15]; D col = l&15, row = 4*(l>>4) + r) per wave.
template <int TM>
__global__ __launch_bounds__(EN_WG) void k_enc_conv(EncConv c) {
    constexpr int MI = TM / 32;
    __shared__ float As[EN_KC][EN_LD];
    __shared__ float Bs[EN_KC][EN_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = (wave >> 1) * (TM / 2), wn = (wave & 1) * 32;
    const int p0 = blockIdx.x * EN_PX;
    const int co0 = blockIdx.y * TM;
    const int split = blockIdx.z;
    const int HW = c.Ho * c.Wo;
    const int64_t plane = (int64_t)c.H * c.W;
    const int col = lane;  // this lane stages column `col` of rows wave, wave + 4, ..., wave + EN_KC - 4 of a chunk
    const int p = p0 + col;
    const bool pin = p < c.P;
    const int n = pin ? p / HW : 0, q = pin ? p % HW : 0;
    const int oy = q / c.Wo, ox = q % c.Wo;
    const int by = c.stride * oy - c.pad, bx = c.stride * ox - c.pad;
    const int64_t base = (int64_t)n * c.Ci * plane;
    const bool co_in = col < TM && co0 + col < c.Co;
    const int kbeg = split * c.cps * EN_KC;
    const int kend = min(c.K, kbeg + c.cps * EN_KC);
    // the K index this wave fetches next and its (ty, tx, ci): wave-uniform, stepped by 4 (no division in the loop)
    int kidx = kbeg + wave, kci = kidx % c.Ci, ktx = (kidx / c.Ci) % c.k, kty = (kidx / c.Ci) / c.k;
    // fetch() only ISSUES loads — every one unconditional, from a clamped index (element 0 where the operand is out of range), so that
    // all of a chunk's loads are in flight together; commit() applies the predicates as it writes the operands to LDS.
    float ra[EN_KC / 4], rb[EN_KC / 4];
    unsigned pa = 0, pb = 0;
    auto fetch = [&]() {
        pa = pb = 0;
#pragma unroll
        for (int j = 0; j < EN_KC / 4; ++j) {
            const bool kin = kidx < kend;
            const bool wa = kin && co_in;
            ra[j] = c.wk[wa ? (int64_t)kidx * c.Co + co0 + col : 0];
            pa |= (unsigned)wa << j;
            const int iy = by + kty, ix = bx + ktx;
            const bool wb = kin && pin && iy >= 0 && iy < c.H && ix >= 0 && ix < c.W;
            rb[j] = c.x[wb ? base + kci * plane + (int64_t)iy * c.W + ix : 0];
            pb |= (unsigned)wb << j;
            kidx += 4;
            kci += 4;
            while (kci >= c.Ci) {
                kci -= c.Ci;
                if (++ktx == c.k) {
                    ktx = 0;
                    ++kty;
                }
            }
        }
    };
    en_f32x4 acc[MI][2];
#pragma unroll
    for (int u = 0; u < MI; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v) acc[u][v] = en_f32x4{0.f, 0.f, 0.f, 0.f};
    fetch();
    for (int k0 = kbeg; k0 < kend; k0 += EN_KC) {
#pragma unroll
        for (int j = 0; j < EN_KC / 4; ++j) {  // commit
            As[wave + 4 * j][col] = (pa >> j & 1) ? ra[j] : 0.f;
            Bs[wave + 4 * j][col] = (pb >> j & 1) ? rb[j] : 0.f;
        }
        __syncthreads();
        if (k0 + EN_KC < kend) fetch();
#pragma unroll
        for (int kk = 0; kk < EN_KC; kk += 4) {
            const int kr = kk + (lane >> 4), r = lane & 15;
            float a[MI];
#pragma unroll
            for (int mi = 0; mi < MI; ++mi) a[mi] = As[kr][wm + 16 * mi + r];
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
            const int pc = p0 + wn + 16 * ni + (lane & 15);
            if (pc >= c.P) continue;
            const int64_t pix = (int64_t)(pc / HW) * c.Co * HW + pc % HW;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int co = co0 + wm + 16 * mi + 4 * (lane >> 4) + r;
                if (co >= c.Co) continue;
                const int64_t idx = pix + (int64_t)co * HW;
                if (c.split == 1) c.out[idx] = en_finish(c, acc[mi][ni][r], co, idx);
                else c.ws[(int64_t)split * c.total + idx] = acc[mi][ni][r];
            }
        }
}

__global__ __launch_bounds__(EN_WG) void k_enc_reduce(EncConv c) {
    const int64_t i = (int64_t)blockIdx.x * EN_WG + threadIdx.x;
    if (i >= c.total) return;
    float z = c.ws[i];
    for (int s = 1; s < c.split; ++s) z = z + c.ws[(int64_t)s * c.total + i];
    const int co = (int)((i / ((int64_t)c.Ho * c.Wo)) % c.Co);
    c.out[i] = en_finish(c, z, co, i);
}

__global__ __launch_bounds__(EN_WG) void k_enc_maxpool(const float* __restrict__ x, int64_t total, int H, int W, int Ho, int Wo,
                                                       float* __restrict__ y) {
    const int64_t i = (int64_t)blockIdx.x * EN_WG + threadIdx.x;
    if (i >= total) return;
    const int ox = (int)(i % Wo), oy = (int)((i / Wo) % Ho);
    const float* pl = x + (i / ((int64_t)Wo * Ho)) * H * W;
    float best = -__builtin_inff();
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int iy = 2 * oy - 1 + t / 3, ix = 2 * ox - 1 + t % 3;
        const bool in = iy >= 0 && iy < H && ix >= 0 && ix < W;
        const float v = pl[in ? (int64_t)iy * W + ix : 0];
        if (in && v > best) best = v;
    }
    y[i] = best;
}

// the source cell pair and weights of destination coordinate d: in cells -> out cells (align_corners = False)
__device__ __forceinline__ void en_source(int d, int in, int out, int* i0, int* i1, float* l0, float* l1) {
    const int64_t num = (int64_t)(2 * d + 1) * in - out;
    const int den = 2 * out;
    const int a = num < 0 ? 0 : (int)(num / den), rem = num < 0 ? 0 : (int)(num % den);
    *i0 = a;
    *i1 = a + 1 < in ? a + 1 : in - 1;
    *l1 = (float)rem / (float)den;
    *l0 = (float)(den - rem) / (float)den;
}

__global__ __launch_bounds__(EN_WG) void k_enc_prepare(const float* __restrict__ img, int N, int C, int H, int W,
                                                       const float* __restrict__ mean, const float* __restrict__ std3, int h, int w,
                                                       float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * EN_WG + threadIdx.x;
    if (i >= (int64_t)2 * N * 3 * h * w) return;
    const int x = (int)(i % w), y = (int)((i / w) % h), ch = (int)((i / ((int64_t)w * h)) % 3), row = (int)(i / ((int64_t)w * h * 3));
    const bool mirror = row >= N;
    const float* pl = img + ((int64_t)(mirror ? row - N : row) * C + ch) * H * W;
    int x0, x1, y0, y1;
    float lx0, lx1, ly0, ly1;
    en_source(x, W, w, &x0, &x1, &lx0, &lx1);
    en_source(y, H, h, &y0, &y1, &ly0, &ly1);
    if (mirror) x0 = W - 1 - x0, x1 = W - 1 - x1;
    const float v00 = pl[(int64_t)y0 * W + x0], v01 = pl[(int64_t)y0 * W + x1];
    const float v10 = pl[(int64_t)y1 * W + x0], v11 = pl[(int64_t)y1 * W + x1];
    const float top = __builtin_fmaf(lx1, v01, lx0 * v00), bot = __builtin_fmaf(lx1, v11, lx0 * v10);
    const float r = __builtin_fmaf(ly1, bot, ly0 * top);
    out[i] = (r - mean[ch]) / std3[ch];
}

// ---- entry points -----------------------------------------------------------------------------------------------------------------
static const int64_t EN_MAX_GRID = 0x7fffffff;

static inline int en_out_size(int in, int k, int stride) { return (in + 2 * ((k - 1) / 2) - k) / stride + 1; }

extern "C" int p3d_enc_conv_plan(int N, int Ci, int Co, int Ho, int Wo, int k, int stride, int force_plan, int* out4) {
    EncPlan p;
    const int rc = enc_conv_plan(N, Ci, Co, Ho, Wo, k, stride, force_plan, &p);
    if (rc) return rc;
    if (out4) {
        out4[0] = p.tile, out4[1] = p.split, out4[2] = p.cps;
        out4[3] = (int)(p.wgs > 0x7fffffff ? 0x7fffffff : p.wgs);
    }
    return (p.tile << 8) | p.split;
}

extern "C" size_t p3d_enc_conv_workspace_bytes(int N, int Ci, int Co, int Ho, int Wo, int k, int stride, int force_plan) {
    EncPlan p;
    if (enc_conv_plan(N, Ci, Co, Ho, Wo, k, stride, force_plan, &p)) return 0;
    return enc_conv_workspace(p, N, Co, Ho, Wo);
}

// the checks of one convolution: sizes, plan, workspace.  Fills the plan and the output size.
static int en_conv_check(int N, int Ci, int H, int W, int k, int stride, int Co, int force_plan, size_t workspace_bytes, bool have_ws,
                         EncPlan* p, int* Ho, int* Wo) {
    if (N <= 0 || Ci <= 0 || H <= 0 || W <= 0 || Co <= 0) return P3D_E_ARG;
    if ((k != 1 && k != 3 && k != 7) || (stride != 1 && stride != 2)) return P3D_E_RANGE;
    if ((int64_t)N * Ci * H >= ENC_MAX_ELEMS / W) return P3D_E_RANGE;
    *Ho = en_out_size(H, k, stride), *Wo = en_out_size(W, k, stride);
    const int rc = enc_conv_plan(N, Ci, Co, *Ho, *Wo, k, stride, force_plan, p);
    if (rc) return rc;
    if (p->ptiles > EN_MAX_GRID) return P3D_E_RANGE;
    const size_t need = enc_conv_workspace(*p, N, Co, *Ho, *Wo);
    if (need && (!have_ws || workspace_bytes < need)) return have_ws ? P3D_E_WORKSPACE : P3D_E_ARG;
    if (p->split > 1 && ((int64_t)N * Co * *Ho * *Wo + EN_WG - 1) / EN_WG > EN_MAX_GRID) return P3D_E_RANGE;
    return 0;
}

static int en_conv_launch(const float* x, int N, int Ci, int H, int W, const float* wk, int k, int stride, int Co, const float* bias,
                          const float* res, int flags, float* out, const EncPlan& p, int Ho, int Wo, void* workspace, hipStream_t s) {
    EncConv c;
    c.x = x, c.wk = wk, c.bias = bias, c.res = res, c.out = out, c.ws = (float*)workspace;
    c.Ci = Ci, c.H = H, c.W = W, c.k = k, c.Co = Co, c.Ho = Ho, c.Wo = Wo, c.stride = stride, c.pad = (k - 1) / 2;
    c.K = k * k * Ci, c.P = N * Ho * Wo, c.relu = (flags & P3D_ENC_RELU) != 0, c.split = p.split, c.cps = p.cps;
    c.total = (int64_t)N * Co * Ho * Wo;
    const dim3 grid((unsigned)p.ptiles, (unsigned)p.ctiles, (unsigned)p.split);
    if (p.tm == 64) hipLaunchKernelGGL(k_enc_conv<64>, grid, dim3(EN_WG), 0, s, c);
    else hipLaunchKernelGGL(k_enc_conv<32>, grid, dim3(EN_WG), 0, s, c);
    if (p.split > 1) hipLaunchKernelGGL(k_enc_reduce, dim3((unsigned)((c.total + EN_WG - 1) / EN_WG)), dim3(EN_WG), 0, s, c);
    return (int)hipGetLastError();
}

extern "C" int p3d_enc_conv_f32(const float* x, int N, int Ci, int H, int W, const float* wk, int k, int stride, int Co, const float* bias,
                                const float* res, int flags, float* out, int force_plan, void* workspace, size_t workspace_bytes,
                                void* stream) {
    if (!x || !wk || !bias || !out) return P3D_E_ARG;
    if (flags & ~P3D_ENC_RELU) return P3D_E_RANGE;
    EncPlan p;
    int Ho, Wo;
    const int rc = en_conv_check(N, Ci, H, W, k, stride, Co, force_plan, workspace_bytes, workspace != nullptr, &p, &Ho, &Wo);
    if (rc) return rc;
    return en_conv_launch(x, N, Ci, H, W, wk, k, stride, Co, bias, res, flags, out, p, Ho, Wo, workspace, (hipStream_t)stream);
}

static int en_pool_check(int64_t planes, int H, int W, int64_t* blocks) {
    if (planes <= 0 || H <= 0 || W <= 0) return P3D_E_ARG;
    if (planes >= ENC_MAX_ELEMS / H / W) return P3D_E_RANGE;
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    *blocks = (planes * Ho * Wo + EN_WG - 1) / EN_WG;
    return *blocks > EN_MAX_GRID ? P3D_E_RANGE : 0;
}

static int en_pool_launch(const float* x, int64_t planes, int H, int W, float* y, int64_t blocks, hipStream_t s) {
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    hipLaunchKernelGGL(k_enc_maxpool, dim3((unsigned)blocks), dim3(EN_WG), 0, s, x, planes * Ho * Wo, H, W, Ho, Wo, y);
    return (int)hipGetLastError();
}

extern "C" int p3d_enc_maxpool_f32(const float* x, int64_t planes, int H, int W, float* y, void* stream) {
    if (!x || !y) return P3D_E_ARG;
    int64_t blocks;
    const int rc = en_pool_check(planes, H, W, &blocks);
    if (rc) return rc;
    return en_pool_launch(x, planes, H, W, y, blocks, (hipStream_t)stream);
}

static int en_prepare_check(int N, int C, int H, int W, int h, int w, int64_t* blocks) {
    if (N <= 0 || C <= 0 || H <= 0 || W <= 0 || h <= 0 || w <= 0) return P3D_E_ARG;
    const int lim = 1 << 22;
    if (C < 3 || H >= lim || W >= lim || h >= lim || w >= lim || N > (1 << 20)) return P3D_E_RANGE;
    if ((int64_t)N * C * H >= ENC_MAX_ELEMS / W || (int64_t)N * 6 * h >= ENC_MAX_ELEMS / w) return P3D_E_RANGE;
    *blocks = ((int64_t)2 * N * 3 * h * w + EN_WG - 1) / EN_WG;
    return *blocks > EN_MAX_GRID ? P3D_E_RANGE : 0;
}

extern "C" int p3d_enc_prepare_f32(const float* img, int N, int C, int H, int W, const float* mean, const float* std3, int h, int w,
                                   float* out, void* stream) {
    if (!img || !mean || !std3 || !out) return P3D_E_ARG;
    int64_t blocks;
    const int rc = en_prepare_check(N, C, H, W, h, w, &blocks);
    if (rc) return rc;
    hipLaunchKernelGGL(k_enc_prepare, dim3((unsigned)blocks), dim3(EN_WG), 0, (hipStream_t)stream, img, N, C, H, W, mean, std3, h, w, out);
    return (int)hipGetLastError();
}

extern "C" int p3d_enc_struct_layout(size_t* out, int cap) {
    if (!out || cap <= 0) return P3D_E_ARG;
    int n = 0;
#define EN_PUT(v) do { if (n >= cap) return P3D_E_RANGE; out[n++] = (size_t)(v); } while (0)
#define EN_OFF(f) EN_PUT(offsetof(p3d_enc_layer, f))
    EN_PUT(sizeof(p3d_enc_layer));
    EN_OFF(kind); EN_OFF(N); EN_OFF(Ci); EN_OFF(H); EN_OFF(W); EN_OFF(Co); EN_OFF(Ho); EN_OFF(Wo); EN_OFF(k); EN_OFF(stride);
    EN_OFF(in); EN_OFF(out); EN_OFF(res); EN_OFF(flags); EN_OFF(plan); EN_OFF(reserved); EN_OFF(w_off); EN_OFF(b_off);
#undef EN_OFF
#undef EN_PUT
    return n;
}

// One record against the table's buffers and blob.  launch == false: the checks alone (*need: the workspace the record asks for).
static int en_layer(const p3d_enc_layer& l, const float* weights, int64_t weight_floats, float* arena, const int64_t* buf_off,
                    const int64_t* buf_len, int n_bufs, void* workspace, size_t workspace_bytes, bool launch, size_t* need, hipStream_t s) {
    *need = 0;
    if (l.in < 0 || l.in >= n_bufs || l.out < 0 || l.out >= n_bufs || l.in == l.out || l.reserved != 0) return P3D_E_RANGE;
    const float* x = arena ? arena + buf_off[l.in] : nullptr;
    float* y = arena ? arena + buf_off[l.out] : nullptr;
    auto fits = [&](int b, int64_t n) { return !buf_len || n <= buf_len[b]; };
    auto blob = [&](int64_t off, int64_t n) { return off >= 0 && n <= weight_floats && off <= weight_floats - n; };
    if (l.kind == P3D_ENC_KIND_CONV) {
        if (l.res < -1 || l.res >= n_bufs || l.res == l.out || (l.flags & ~P3D_ENC_RELU)) return P3D_E_RANGE;
        EncPlan p;
        int Ho, Wo;
        int rc = en_conv_check(l.N, l.Ci, l.H, l.W, l.k, l.stride, l.Co, l.plan, launch ? workspace_bytes : (size_t)-1, true, &p, &Ho, &Wo);
        if (rc) return rc;
        if (Ho != l.Ho || Wo != l.Wo) return P3D_E_RANGE;
        const int64_t n_in = (int64_t)l.N * l.Ci * l.H * l.W, n_out = (int64_t)l.N * l.Co * Ho * Wo;
        if (!fits(l.in, n_in) || !fits(l.out, n_out) || (l.res >= 0 && !fits(l.res, n_out))) return P3D_E_RANGE;
        if (!blob(l.w_off, (int64_t)l.k * l.k * l.Ci * l.Co) || !blob(l.b_off, l.Co)) return P3D_E_RANGE;
        *need = enc_conv_workspace(p, l.N, l.Co, Ho, Wo);
        if (!launch) return 0;
        return en_conv_launch(x, l.N, l.Ci, l.H, l.W, weights + l.w_off, l.k, l.stride, l.Co, weights + l.b_off,
                              l.res >= 0 ? arena + buf_off[l.res] : nullptr, l.flags, y, p, Ho, Wo, workspace, s);
    }
    if (l.kind == P3D_ENC_KIND_MAXPOOL) {
        if (l.N <= 0 || l.Ci <= 0) return P3D_E_ARG;
        int64_t blocks;
        const int rc = en_pool_check((int64_t)l.N * l.Ci, l.H, l.W, &blocks);
        if (rc) return rc;
        if (l.Co != l.Ci || l.Ho != (l.H - 1) / 2 + 1 || l.Wo != (l.W - 1) / 2 + 1 || l.res != -1) return P3D_E_RANGE;
        if (!fits(l.in, (int64_t)l.N * l.Ci * l.H * l.W) || !fits(l.out, (int64_t)l.N * l.Ci * l.Ho * l.Wo)) return P3D_E_RANGE;
        if (!launch) return 0;
        return en_pool_launch(x, (int64_t)l.N * l.Ci, l.H, l.W, y, blocks, s);
    }
    if (l.kind == P3D_ENC_KIND_PREPARE) {
        int64_t blocks;
        const int rc = en_prepare_check(l.N, l.Ci, l.H, l.W, l.Ho, l.Wo, &blocks);
        if (rc) return rc;
        if (l.Co != 3 || l.res != -1) return P3D_E_RANGE;
        if (!fits(l.in, (int64_t)l.N * l.Ci * l.H * l.W) || !fits(l.out, (int64_t)2 * l.N * 3 * l.Ho * l.Wo)) return P3D_E_RANGE;
        if (!blob(l.w_off, 3) || !blob(l.b_off, 3)) return P3D_E_RANGE;
        if (!launch) return 0;
        hipLaunchKernelGGL(k_enc_prepare, dim3((unsigned)blocks), dim3(EN_WG), 0, s, x, l.N, l.Ci, l.H, l.W, weights + l.w_off,
                           weights + l.b_off, l.Ho, l.Wo, y);
        return (int)hipGetLastError();
    }
    return P3D_E_RANGE;
}

extern "C" size_t p3d_encoder_workspace_bytes(const p3d_enc_layer* layers, int n_layers) {
    if (!layers || n_layers <= 0) return 0;
    size_t most = 0;
    for (int i = 0; i < n_layers; ++i) {
        size_t need;
        // (no buffers here: indices are checked against a table as large as the indices ask for)
        if (en_layer(layers[i], nullptr, (int64_t)1 << 62, nullptr, nullptr, nullptr, 0x7fffffff, nullptr, 0, false, &need, nullptr)) return 0;
        if (need > most) most = need;
    }
    return most;
}

extern "C" int p3d_encoder_forward_f32(const p3d_enc_layer* layers, int n_layers, const float* weights, int64_t weight_floats, float* arena,
                                       int64_t arena_floats, const int64_t* buf_off, const int64_t* buf_len, int n_bufs, void* workspace,
                                       size_t workspace_bytes, void* stream) {
    if (!layers || !weights || !arena || !buf_off || !buf_len) return P3D_E_ARG;
    if (n_layers <= 0 || weight_floats <= 0 || arena_floats <= 0 || n_bufs <= 0) return P3D_E_ARG;
    for (int b = 0; b < n_bufs; ++b)
        if (buf_off[b] < 0 || buf_len[b] < 0 || buf_len[b] > arena_floats || buf_off[b] > arena_floats - buf_len[b]) return P3D_E_RANGE;
    size_t most = 0;
    for (int i = 0; i < n_layers; ++i) {  // every record, before any launch
        size_t need;
        const int rc = en_layer(layers[i], weights, weight_floats, arena, buf_off, buf_len, n_bufs, workspace, workspace_bytes, false, &need, nullptr);
        if (rc) return rc;
        if (need > most) most = need;
    }
    if (most && !workspace) return P3D_E_ARG;
    if (most > workspace_bytes) return P3D_E_WORKSPACE;
    for (int i = 0; i < n_layers; ++i) {
        size_t need;
        const int rc = en_layer(layers[i], weights, weight_floats, arena, buf_off, buf_len, n_bufs, workspace, workspace_bytes, true, &need,
                                (hipStream_t)stream);
        if (rc) return rc;
    }
    return 0;
}
