"""Cases, float64 reference and gate shared by the tests of the stand-alone ToRGB GEMM (k_torgb, csrc/p3d_torgb.hip; p3d_torgb_f32;
ops.torgb): tests/test_torgb_cases_cpu.py, tests/test_hip_torgb_edges.py.  Not collected.

    y[n,o,p] = clamp(sum_i w[o,i] * s[n,i] * x[n,i,p] + bias[o]) + upsample2d(skip)[n,o,p]

THE GATE is the project's (tests/synthesis_grad_ref.py: GATE_C, REL_L2, gate) on the pre-clamp sum: K = I (+ 1 with a bias), absref
= sum_i |w s x| + |bias|, carried through the clamp (1-Lipschitz), plus the skip image's four-tap part sum |f| |skip| (its fmas and the
final addition round on those magnitudes).  Where absref == 0 the value must be exact.

Every case names the instantiation of k_torgb it is there to reach (csrc/p3d_torgb_plan.hpp); the CPU test checks that against the plan
and checks the coverage conditions listed there.  PX tiles = N * ceil(HW / 128), KS tiles = N * ceil(HW / 32):
    k_torgb<1,false>           O <= 32, PX tiles >= 512
    k_torgb<1,true>            O <= 32, PX tiles < 512
    k_torgb<3,false>           O > 32, PX tiles >= 512
    k_torgb<3,true>            O > 32, PX tiles < 512, 3 * KS tiles > 1024
    k_torgb<1,true,true>       O > 32, 3 * KS tiles <= 1024, I > 512          (MS)
    k_torgb<1,true,true,true>  O > 32, 3 * KS tiles <= 1024, I <= 512         (MS + PRE)
(3 * KS tiles is a multiple of 3: the two sides of the 1024 edge are 1023 and 1026.)"""
import collections

import torch
import torch.nn.functional as F

from modconv_ref import epilogue, lipschitz, setup_filter  # the forward convolution's epilogue and its Lipschitz factor: the same here
from synthesis_grad_ref import f32, upsample2d_ref

PX1, KS1, PX3, KS3, MS, PRE = ("k_torgb<1,false>", "k_torgb<1,true>", "k_torgb<3,false>", "k_torgb<3,true>", "k_torgb<1,true,true>",
                               "k_torgb<1,true,true,true>")
KERNELS = (PX1, KS1, PX3, KS3, MS, PRE)
CLAMP = 0.5  # the pre-clamp sums are of order one (make_inputs): about half of them clip

# filt: the skip image's 4x4 filter, None (no skip), "sym" ([1,3,3,1]) or "asym" (the outer product of (1,2,4,8) and (1,3,5,11): a missing
# flip or swapped axes show)
Case = collections.namedtuple("Case", "id kernel N I O H W bias clamp filt")
CASES = [
    # ---- PX, O <= 32: N * ceil(HW / 128) >= 512; 90 x 91 = 8190 = 64 tiles less 2 pixels, 90 x 92 = 8280 = 64 tiles and 88 pixels
    Case("px1-512tiles-i65", PX1, 8, 65, 3, 90, 91, False, None, None),
    Case("px1-skip-i129-o32", PX1, 8, 129, 32, 90, 92, True, CLAMP, "asym"),
    # ---- PX, O > 32
    Case("px3-512tiles-i64-o33", PX3, 8, 64, 33, 90, 91, False, None, None),
    Case("px3-skip-i7-o96", PX3, 8, 7, 96, 90, 92, True, CLAMP, "sym"),
    # ---- KS, O <= 32: below 512 PX tiles (7 * 73 = 511 at 96 x 97)
    Case("ks1-511tiles-o1", KS1, 7, 10, 1, 96, 97, False, None, None),
    Case("ks1-skip-i200", KS1, 2, 200, 3, 6, 10, True, CLAMP, "asym"),
    Case("ks1-i1-o32", KS1, 2, 1, 32, 5, 7, True, None, None),
    Case("ks1-skip-i1024", KS1, 2, 1024, 3, 4, 6, False, CLAMP, "sym"),
    # ---- KS, O > 32, 3 * KS tiles > 1024 (6 * 57 * 3 = 1026 at 36 x 50; 3 * 115 * 3 = 1035 at 59 x 62)
    Case("ks3-1026-skip-i513", KS3, 6, 513, 40, 36, 50, True, CLAMP, "asym"),
    Case("ks3-511tiles-i3", KS3, 7, 3, 33, 96, 97, False, None, None),
    Case("ks3-i129-o96", KS3, 3, 129, 96, 59, 62, False, CLAMP, None),
    Case("ks3-skip-i64", KS3, 3, 64, 40, 60, 62, True, None, "sym"),
    # ---- MS without PRE: 512 < I <= 1024 (11 * 31 * 3 = 1023 at 22 x 44)
    Case("ms-1023-skip-i513", MS, 11, 513, 40, 22, 44, True, CLAMP, "asym"),
    Case("ms-i1024-o96", MS, 2, 1024, 96, 7, 9, False, None, None),
    Case("ms-n1-skip-i515", MS, 1, 515, 40, 6, 10, False, None, "sym"),
    Case("ms-i577-o33", MS, 2, 577, 33, 3, 5, True, CLAMP, None),
    # ---- MS + PRE: I <= 512 (11 * 31 * 3 = 1023 at 31 x 31)
    Case("pre-1023-i512-o96", PRE, 11, 512, 96, 31, 31, False, None, None),
    Case("pre-skip-i65", PRE, 2, 65, 40, 6, 10, True, CLAMP, "asym"),
    Case("pre-skip-i1", PRE, 3, 1, 33, 4, 4, False, None, "sym"),
    Case("pre-i200-o96", PRE, 2, 200, 96, 5, 9, True, CLAMP, None),
    Case("pre-skip-i129", PRE, 2, 129, 40, 8, 6, True, None, "asym"),
]
CASE_IDS = [c.id for c in CASES]
BY_ID = {c.id: c for c in CASES}

# (id, what changes against `base`, the documented code): calls p3d_torgb_f32 must refuse without writing.  base: N = 2, I = 8, O = 3,
# H = W = 4, with a skip image.
REFUSALS = [
    ("o97", dict(O=97), -2),
    ("i1025", dict(I=1025), -2),
    ("skip-odd-h", dict(H=5), -2),
    ("skip-odd-w", dict(W=5), -2),
    ("skip-without-filter", dict(null=("skipf",)), -1),
    ("filter-without-skip", dict(null=("skip",)), -1),
    ("null-x", dict(null=("x",)), -1),
    ("null-weights", dict(null=("wt",)), -1),
    ("null-styles", dict(null=("styles",)), -1),
    ("null-y", dict(null=("y",)), -1),
    ("n0", dict(N=0), -1),
]


def case_filter(c):
    if c.filt is None:
        return None
    if c.filt == "sym":
        return setup_filter([1, 3, 3, 1])
    f = torch.tensor([1.0, 2.0, 4.0, 8.0]).ger(torch.tensor([1.0, 3.0, 5.0, 11.0]))
    return f / f.sum()


def make_inputs(c, _memo={}):
    """fp32 CPU tensors of one case, seeded by its shape, made once per process and shared (never modified).  Weights N(0,1) / sqrt(I),
    styles 1 + N(0,1) / 2, x N(0,1): pre-clamp sums of order one, so that CLAMP clips about half of them."""
    if c.id not in _memo:
        g = torch.Generator().manual_seed(c.N * 7919 + c.I * 131 + c.O * 17 + c.H * 5 + c.W)
        t = dict(x=torch.randn(c.N, c.I, c.H, c.W, generator=g), s=torch.randn(c.N, c.I, generator=g) * 0.5 + 1.0,
                 w=torch.randn(c.O, c.I, generator=g) / c.I ** 0.5)
        t["bias"] = torch.randn(c.O, generator=g) * 0.3 if c.bias else None
        t["skip"] = torch.randn(c.N, c.O, c.H // 2, c.W // 2, generator=g) if c.filt else None
        t["f"] = case_filter(c)
        _memo[c.id] = t
    return _memo[c.id]


def torgb_ref(x, w, s, bias=None, clamp=None, skip=None, f=None):
    """The float64 reference of one call and its gate scale: dict(y, pre, absref, K, clipped = the share of clamped values)."""
    d = lambda t: t.double()
    xs = d(s)[:, :, None, None] * d(x)
    pre = torch.einsum("oi,nihw->nohw", d(w), xs)
    ab = torch.einsum("oi,nihw->nohw", d(w).abs(), xs.abs())
    K = x.shape[1]
    if bias is not None:
        pre, ab, K = pre + d(bias)[None, :, None, None], ab + d(bias).abs()[None, :, None, None], K + 1
    # the epilogue of tests/modconv_ref.py (linear, gain 1, the clamp as the binary32 number the kernel receives) and its factor on the scale
    cl = None if clamp is None else f32(clamp)
    y, ab = epilogue(pre, "linear", 0.0, 1.0, cl), lipschitz("linear", 0.0, 1.0) * ab
    clipped = 0.0 if cl is None else float((pre.abs() > cl).double().mean())
    if skip is not None:
        y = upsample2d_ref(d(skip), f) + y
        ab = ab + upsample2d_ref(d(skip).abs(), d(f).abs())
    return dict(y=y, pre=pre, absref=ab, K=K, clipped=clipped)


def case_ref(c, _memo={}):
    if c.id not in _memo:
        t = make_inputs(c)
        _memo[c.id] = torgb_ref(t["x"], t["w"], t["s"], t["bias"], c.clamp, t["skip"], t["f"])
    return _memo[c.id]


def tiles(c):
    HW = c.H * c.W
    return c.N * -(-HW // 128), c.N * -(-HW // 32)


# ---- the same composition on torch's operators: float64 (what the reference must equal), binary32 (a legitimate result), seeded faults ----
FAULTS = ("chunk_edge_channel", "last_odd_channel", "tile_shifted", "bias_after_clamp", "clamp_after_skip", "skip_parity", "skip_border",
          "styles_other_item", "px_tile_last_pixel")
# fault -> the case that must fail with it
FAULT_CASE = {"chunk_edge_channel": "pre-skip-i129", "last_odd_channel": "ms-1023-skip-i513", "tile_shifted": "ks3-i129-o96",
              "bias_after_clamp": "pre-i200-o96", "clamp_after_skip": "ks1-skip-i200", "skip_parity": "ks3-skip-i64",
              "skip_border": "px3-skip-i7-o96", "styles_other_item": "ks1-i1-o32", "px_tile_last_pixel": "px1-512tiles-i65"}


def _upsample_torch(skip, f, fault=None):
    """upsample2d on F.conv2d, not on upsample2d_ref: zero-insert, pad (2, 1), correlate with the flipped filter times 4."""
    N, C, H, W = skip.shape
    z = skip.new_zeros(N, C, 2 * H, 2 * W)
    if fault == "skip_parity":
        z[:, :, ::2, 1::2] = skip
    else:
        z[:, :, ::2, ::2] = skip
    if fault == "skip_border":  # the border taps read the nearest sample instead of zero
        z = F.pad(F.pad(z, [0, 1, 0, 1]), [2, 0, 2, 0], mode="replicate")
    else:
        z = F.pad(z, [2, 1, 2, 1])
    k = (f.to(skip.dtype) * 4).flip([0, 1])[None, None].repeat(C, 1, 1, 1)
    return F.conv2d(z, k, groups=C)


def torgb_torch(x, w, s, bias=None, clamp=None, skip=None, f=None, dtype=torch.float32, order="plain", fault=None):
    """ToRGBLayer.forward + the skip connection on torch's operators in `dtype`.  order: "plain" (per-sample weights w * s through
    F.conv2d: the reference network's own formulation), "modx" (w against s * x, one matrix product) or "quarters" (the KS waves' order:
    every 64-channel chunk's four 16-channel quarters go to four partial sums, which are added in order)."""
    assert fault is None or fault in FAULTS
    x, w, s = x.to(dtype), w.to(dtype), s.to(dtype)
    N, I, H, W = x.shape
    O = w.shape[0]
    if fault == "styles_other_item":
        s = s.roll(1, 0)
    keep = torch.ones(I, dtype=torch.bool)
    if fault == "chunk_edge_channel":
        keep[64] = False
    if fault == "last_odd_channel":
        assert I % 2 == 1
        keep[I - 1] = False
    w = w * keep.to(dtype)[None, :]
    if order == "plain":
        ww = w[None] * s[:, None, :]
        v = torch.cat([F.conv2d(x[n:n + 1], ww[n][:, :, None, None]) for n in range(N)])
    else:
        xs = (s[:, :, None, None] * x).reshape(N, I, H * W)
        if order == "modx":
            v = torch.matmul(w, xs)
        else:
            k = torch.arange(I)
            v = None
            for q in range(4):
                idx = k[(k % 64) // 16 == q]
                part = torch.matmul(w[:, idx], xs[:, idx]) if len(idx) else xs.new_zeros(N, O, H * W)
                v = part if v is None else v + part
        v = v.reshape(N, O, H, W)
    if fault == "tile_shifted":
        v = torch.cat([v[:, :32], v[:, 32:64].roll(1, 1), v[:, 64:]], dim=1)
    b = None if bias is None else bias.to(dtype)[None, :, None, None]
    cl = None if clamp is None else f32(clamp)
    if b is not None and fault != "bias_after_clamp":
        v = v + b
    if cl is not None and fault != "clamp_after_skip":
        v = v.clamp(-cl, cl)
    if b is not None and fault == "bias_after_clamp":
        v = v + b
    if skip is not None:
        v = _upsample_torch(skip.to(dtype), f, fault) + v
    if cl is not None and fault == "clamp_after_skip":
        v = v.clamp(-cl, cl)
    if fault == "px_tile_last_pixel":  # the last pixel of a 128-pixel tile written from its neighbour's lane
        v = v.reshape(N, O, H * W).clone()
        v[:, :, 127] = v[:, :, 126]
        v = v.reshape(N, O, H, W)
    return v


def case_torch(c, dtype=torch.float32, order="plain", fault=None):
    t = make_inputs(c)
    return torgb_torch(t["x"], t["w"], t["s"], t["bias"], c.clamp, t["skip"], t["f"], dtype, order, fault)


def weights_t(w):
    """What p3d_torgb_weights_f32 writes: [O][I] -> [I][32 or 96], transposed, the channels padded with zeros."""
    O, I = w.shape
    wt = w.new_zeros(I, 32 if O <= 32 else 96)
    wt[:, :O] = w.t()
    return wt
