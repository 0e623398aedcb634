"""The float64 reference of the FORWARD modulated convolution (p3d_modconv2d_ex_f32, include/panic3d_hip.h) and its error gate.

Written from the header's contract and networks_stylegan2.py's formulas (modulated_conv2d :40-97, bias_act after it :350-352,
conv2d_resample.py:114-128 for up = 2), tap by tap, without torch's convolutions: `torch_modconv_ref` below — the torch conv2d /
conv_transpose2d formulation the older forward tests use — is what tests/test_modconv_cases_cpu.py pins it against.

    xs[n,i]   = styles[n,i] * x[n,i]                                   (the modulated input; an ActImage input holds exactly that)
    up = 1:   c[n,o,y,x]   = sum_{i,ky,kx} w[o,i,ky,kx] * xs[n,i,y+ky-p,x+kx-p]        (zero outside the map; p = ks // 2)
    up = 2:   T[n,o,2y+ky,2x+kx] += w[o,i,ky,kx] * xs[n,i,y,x]          ((2H+1) x (2W+1): the stride-2 transposed convolution)
              c[n,o,Y,X]   = sum_{fy,fx} F[fy,fx] * Tpad[Y+fy,X+fx],  F = 4 * flip(f), Tpad = T with one zero all round
    pre       = d[n,o] * c + noise[(n,) Y, X] + bias[o],   d = rsqrt(sum_{i,k} (w*s)^2 + 1e-8), the caller's dcoef, or 1
    y         = clamp(act(pre) * gain),   act: identity or v < 0 ? alpha * v : v

Next to every sum the same sum over absolute values (`absref`, with |noise| and |bias| added): the scale of an fp32 evaluation's
rounding error, element by element.  THE GATE is the project's (tests/synthesis_grad_ref.py: GATE_C, REL_L2, gate):
    |ours - ref| <= GATE_C * sqrt(K) * 2^-24 * absref,   K = I * ks^2,
on the pre-activation value, carried through the epilogue by its Lipschitz factor gain * max(1, |alpha|) (the clamp is
1-Lipschitz), i.e. absref_y = lip * absref_pre.  Operand modes other than fp32 add terms to that SCALE (never to GATE_C); each is a
formula below with its derivation.  The other outputs (the ActImage of the next layer, the riding ToRGB's partial sums, their
combination) have reference parts at the end."""
import math

import torch
import torch.nn.functional as F

from synthesis_grad_ref import EPS32, GATE_C, REL_L2, gate, gate_ratio, rel_l2  # noqa: F401  (the one gate of the project)

F16_MIN_NORMAL = 2.0 ** -14   # the matrix cores flush f16 operands below this (include/panic3d_hip.h, two-term operands)
X2_SCALE_X, X2_SCALE_W = 16.0, 64.0  # the header's 2^4 on s*x and 2^6 on w; the accumulators are scaled back by 2^-10


def torch_modconv_ref(x, w, s, noise, up, demod, bias, f, dcoef=None):
    """Plain PyTorch (CPU) restatement of modulated_conv2d + noise + bias in x's dtype: per-sample weights, torch's own conv2d /
    conv_transpose2d, the FIR as a grouped conv2d.  Any H, W; noise [OH,OW] or [N,1,OH,OW]; dcoef [N,O] replaces the demodulation."""
    N, I, H, W = x.shape
    O, _, k, _ = w.shape
    ww = w.unsqueeze(0) * s.reshape(N, 1, I, 1, 1)
    if dcoef is not None:
        ww = ww * dcoef.reshape(N, O, 1, 1, 1)
    elif demod:
        ww = ww * (ww.square().sum(dim=[2, 3, 4], keepdim=True) + 1e-8).rsqrt()
    ys = []
    for n in range(N):
        if up == 1:
            y = F.conv2d(x[n:n + 1], ww[n], padding=k // 2)
        else:
            y = F.conv_transpose2d(x[n:n + 1], ww[n].transpose(0, 1), stride=2)
            ff = (f * 4).flip([0, 1])[None, None].repeat(O, 1, 1, 1)
            y = F.conv2d(F.pad(y, [1, 1, 1, 1]), ff, groups=O)
        ys.append(y)
    y = torch.cat(ys)
    if noise is not None:
        y = y + noise
    if bias is not None:
        y = y + bias.reshape(1, -1, 1, 1)
    return y


# ---- the contraction, tap by tap ------------------------------------------------------------------------------------------------
def conv_taps(xs, w, up):
    """c of the module docstring BEFORE the FIR pass: [N,O,H,W] (up = 1) or the intermediate T [N,O,2H+1,2W+1] (up = 2)."""
    N, I, H, W = xs.shape
    O, _, k, _ = w.shape
    if up == 1:
        p = k // 2
        xp = F.pad(xs, [p, p, p, p])
        out = xs.new_zeros((N, O, H, W))
        for ky in range(k):
            for kx in range(k):
                out += torch.einsum("oi,nihw->nohw", w[:, :, ky, kx], xp[:, :, ky:ky + H, kx:kx + W])
        return out
    T = xs.new_zeros((N, O, 2 * H + 1, 2 * W + 1))
    for ky in range(3):
        for kx in range(3):
            T[:, :, ky:ky + 2 * H:2, kx:kx + 2 * W:2] += torch.einsum("oi,nihw->nohw", w[:, :, ky, kx], xs)
    return T


def fir_taps(T, F4):
    """The FIR pass of an up-sampling layer: T [.., 2H+1, 2W+1] padded by one, correlated with F4 (= 4 * flip(f)) -> [.., 2H, 2W]."""
    OH, OW = T.shape[-2] - 1, T.shape[-1] - 1
    Tp = F.pad(T, [1, 1, 1, 1])
    out = T.new_zeros(T.shape[:-2] + (OH, OW))
    for fy in range(4):
        for fx in range(4):
            out += F4[fy, fx] * Tp[..., fy:fy + OH, fx:fx + OW]
    return out


def fir4(f, dtype=torch.float64, gain=4.0, flip=True):
    """What the C ABI's `fir` holds: the 4x4 filter flipped and multiplied by up^2 (upfirdn2d.py:193-196)."""
    ff = f.to(dtype) * gain
    return ff.flip([0, 1]) if flip else ff


def contraction(xs, w, up, f):
    c = conv_taps(xs, w, up)
    return fir_taps(c, fir4(f, xs.dtype)) if up == 2 else c


def demod_coefs(w, s, dtype=torch.float64):
    """d[n,o] = rsqrt(sum_i (sum_taps w[o,i]^2) * s[n,i]^2 + 1e-8)   (networks_stylegan2.py:70-73)."""
    w2 = w.to(dtype).square().sum(dim=(2, 3))
    return ((s.to(dtype).square()[:, None, :] * w2[None]).sum(dim=2) + 1e-8).rsqrt()


def epilogue(pre, act, alpha, gain, clamp):
    """bias_act.py:93-122 after the bias: act (linear / lrelu(alpha)), * gain, clamp (None: none)."""
    v = torch.where(pre < 0, pre * alpha, pre) if act == "lrelu" else pre
    v = v * gain
    return v.clamp(-clamp, clamp) if clamp is not None else v


def lipschitz(act, alpha, gain):
    return abs(gain) * (max(1.0, abs(alpha)) if act == "lrelu" else 1.0)


# ---- operand modes ----------------------------------------------------------------------------------------------------------------
def f16_round(v):
    """RNE to f16 and back, exactly (torch's .half() is RNE; f16 -> f64 is exact)."""
    return v.float().half().double()


def x2_split(v, scale):
    """The header's two-term operand of v (fp32): A = scale * v, hi = f16(A), lo = f16(A - hi), as float64."""
    A = v.float() * scale                      # a power of two: exact
    hi = A.half()
    lo = (A - hi.float()).half()               # A - hi is exact in fp32 (Sterbenz-like: hi is A to 11 bits)
    return A.double(), hi.double(), lo.double()


def flushed(h):
    """A matrix-core f16 operand: subnormals read as zero."""
    return torch.where(h.abs() < F16_MIN_NORMAL, torch.zeros_like(h), h)


def x2_operand_error(v, scale, margin=1.0):
    """|A - (hi + lo)| of the two-term operand of v as the matrix cores see it, bounded element by element, in units of A.
    (a) Representation.  hi = rn16(A): |A - hi| <= 2^-11 |A|.  lo = rn16(A - hi): |A - hi - lo| <= 2^-11 |A - hi| <= 2^-22 |A|.
    (b) The contract's flush floor.  A part below 2^-14 in magnitude is a subnormal f16, which the matrix cores read as zero: the
        operand then loses that part, |lo| (or |hi| when A itself is that small), on top of (a).  Most lo parts are normal (the
        header scales the operands for that), so the term is taken where it applies, not everywhere.  `margin` widens the test
        |part| < margin * 2^-14 for operands that are only known to fp32 round-off (the image output's values)."""
    A, hi, lo = x2_split(v, scale)
    e = 2.0 ** -22 * A.abs()
    for part in (lo, hi):
        e = e + torch.where(part.abs() < margin * F16_MIN_NORMAL, part.abs(), torch.zeros_like(part))
    return A, e


def f16_flush_error(h):
    """One-term mode: the operand is f16(v) exactly (the reference takes it pre-rounded); what remains of the operand's own error is
    the flush floor: a subnormal f16(v) reads as zero, an error of |f16(v)| < 2^-14."""
    return torch.where(h.abs() < F16_MIN_NORMAL, h.abs(), torch.zeros_like(h))


# ---- the reference of one call --------------------------------------------------------------------------------------------------
def modconv_ref(x, w, s, *, up=1, demodulate=True, dcoef=None, noise=None, bias=None, f=None, act="linear", alpha=0.2, gain=1.0,
                clamp=None, mma="f32", dtype=torch.float64):
    """One call, every option of the C ABI.  x [N,I,H,W], w [O,I,ks,ks], s [N,I] fp32 tensors; dcoef [N,O] (the caller's) or None;
    noise None / [OH,OW] / [N,1,OH,OW]; bias [O] or None; f the 4x4 filter (up = 2).  mma: "f32", "f16" (operands pre-rounded as
    the header documents: f16(s*x) with s*x the fp32 product, f16(w); the demodulation from the fp32 weights) or "x2".
    Returns a dict: pre, y (dtype), absref_pre, absref_y (float64-class scales INCLUDING the mode's extra terms, so that
    gate(name, ours, ref["y"], ref["absref_y"], ref["K"]) is the whole check), K, lip."""
    N, I, H, W = x.shape
    O, _, ks, _ = w.shape
    K = I * ks * ks
    xs32 = s.float()[:, :, None, None] * x.float()            # the fp32 product every kernel forms first
    xs = (s.to(dtype)[:, :, None, None] * x.to(dtype)) if mma != "f16" else f16_round(xs32).to(dtype)
    wd = w.to(dtype) if mma != "f16" else f16_round(w).to(dtype)
    d = dcoef.to(dtype).reshape(N, O) if (demodulate and dcoef is not None) else demod_coefs(w, s, dtype) if demodulate else None
    c = contraction(xs, wd, up, f)
    ca = contraction(xs.abs(), wd.abs(), up, f.abs() if f is not None else None)
    extra = torch.zeros_like(ca)
    if mma == "x2":
        # Two-term operands.  The kernel sums (A_hi B_hi + A_lo B_hi + A_hi B_lo) / 1024 for A = 16 s x, B = 64 w:
        #   A B - (that) = (A - A_hi - A_lo) B + A (B - B_hi - B_lo) - [cross terms of second order] + A_lo B_lo,
        # so per product, in units of A B / 1024 = (s x) w:
        #   e_A |B| + |A| e_B      the operands' representation error and flush floor (x2_operand_error),
        #   |A_lo| |B_lo| <= 2^-11 |A| * 2^-11 |B| = 2^-22 |A| |B|      the dropped lo * lo product.
        # Summed over the same taps and filter as the result (all terms >= 0).
        A, eA = x2_operand_error(xs32, X2_SCALE_X)
        B, eB = x2_operand_error(w, X2_SCALE_W)
        fa = f.abs() if f is not None else None
        extra = (contraction(eA.to(dtype), B.abs().to(dtype), up, fa) + contraction(A.abs().to(dtype), eB.to(dtype), up, fa)) / 1024.0 \
            + 2.0 ** -22 * ca
    elif mma == "f16":
        fa = f.abs() if f is not None else None
        extra = contraction(f16_flush_error(xs).to(dtype), wd.abs(), up, fa) + contraction(xs.abs(), f16_flush_error(wd).to(dtype), up, fa)
    if d is not None:
        c, ca, extra = c * d[:, :, None, None], ca * d[:, :, None, None].abs(), extra * d[:, :, None, None].abs()
    if noise is not None:
        nz = noise.to(dtype).reshape(-1, 1, H * up, W * up)
        c, ca = c + nz, ca + nz.abs()
    if bias is not None:
        c, ca = c + bias.to(dtype)[None, :, None, None], ca + bias.to(dtype).abs()[None, :, None, None]
    lip = lipschitz(act, alpha, gain)
    # the extra terms are absolute errors: in the gate's scale sqrt(K) * 2^-24 * absref they count as absref += extra / (sqrt(K) 2^-24)
    absref_pre = ca.double() + extra.double() / (math.sqrt(K) * EPS32)
    return dict(pre=c, y=epilogue(c, act, alpha, gain, clamp), absref_pre=absref_pre, absref_y=lip * absref_pre, K=K, lip=lip)


# ---- the other outputs ------------------------------------------------------------------------------------------------------------
def image_ref(ref, next_styles):
    """ActImage.float() of the image output: next_styles[n,o] * y.  Its gate: |ns| times y's, plus the f16 rounding of the image —
    the image stores the two-term operand of v = fp32(ns * y): one fp32 rounding of the product (2^-24 |v|), the representation
    error and the flush floor of x2_operand_error (the flush test with a margin of 2: v is known to round-off only), and one more
    fp32 rounding in ActImage.float()'s (hi + lo) / 16 (2^-24 |v|)."""
    ns = next_styles.double()[:, :, None, None]
    v = ns * ref["y"].double()
    A, e = x2_operand_error(v, X2_SCALE_X, margin=2.0)
    e = e / X2_SCALE_X + 2.0 ** -23 * v.abs()
    return v, ns.abs() * ref["absref_y"] + e / (math.sqrt(ref["K"]) * EPS32)


def torgb_partial_ref(ref, rgb_w, rgb_styles):
    """The riding ToRGB's partial sums [O/64,N,R,H,W]: per 64-channel group, sum_o rgb_w[r,o] * rgb_styles[n,o] * y[n,o].
    Gate: K = K_conv + 64 (the sum continues over 64 channels), absref = sum |rgb_w rgb_styles| * (absref_y + |y|): y's own error
    carried through the 1x1 sum, plus the sum's rounding on its terms' magnitudes."""
    y = ref["y"].double()
    N, O, H, W = y.shape
    m = rgb_w.double()[None] * rgb_styles.double()[:, None, :]          # [N,R,O]
    G = O // 64
    part = torch.einsum("nrgo,ngohw->gnrhw", m.reshape(N, -1, G, 64), y.reshape(N, G, 64, H, W))
    ab = torch.einsum("nrgo,ngohw->gnrhw", m.abs().reshape(N, -1, G, 64), (ref["absref_y"] + y.abs()).reshape(N, G, 64, H, W))
    return part, ab, ref["K"] + 64


def torgb_ref(ref, rgb_w, rgb_styles, rgb_bias=None):
    """The stand-alone ToRGB layer on y (networks_stylegan2.py:376-380, no clamp, no skip): what torgb_combine of the partials gives."""
    part, ab, _ = torgb_partial_ref(ref, rgb_w, rgb_styles)
    img, ab = part.sum(dim=0), ab.sum(dim=0)
    if rgb_bias is not None:
        img, ab = img + rgb_bias.double()[None, :, None, None], ab + rgb_bias.double().abs()[None, :, None, None]
    return img, ab, ref["K"] + ref["y"].shape[1]


# ---- the inputs of a case (tests/modconv_cases.py), the same on the CPU and on the GPU ---------------------------------------------
def setup_filter(taps):
    """upfirdn2d.setup_filter of a 1-D filter: the outer product, normalised to DC gain 1."""
    t = torch.tensor(taps, dtype=torch.float32)
    f = t.ger(t)
    return f / f.sum()


def make_inputs(c):
    """fp32 CPU tensors of one case, seeded by its shape.  Magnitudes of order one throughout (weights scaled by 1/sqrt(K) where
    nothing demodulates), so that a clamp clips and the two-term domain is respected.  A caller-supplied dcoef is NOT the true
    demodulation: every (sample, channel) has a coefficient of its own that only the caller knows."""
    g = torch.Generator().manual_seed(c.N * 7919 + c.I * 131 + c.O * 17 + c.H * 5 + c.W + c.ks * 3 + c.up)
    K = c.I * c.ks * c.ks
    t = dict(x=torch.randn(c.N, c.I, c.H, c.W, generator=g), s=torch.randn(c.N, c.I, generator=g) * 0.5 + 1.0)
    t["w"] = torch.randn(c.O, c.I, c.ks, c.ks, generator=g) * (1.0 if c.demod is True else 1.0 / math.sqrt(K))
    t["dcoef"] = torch.rand(c.N, c.O, generator=g) + 0.5 if c.demod == "dcoef" else None
    OH, OW = c.H * c.up, c.W * c.up
    t["noise"] = None if c.noise is None else torch.randn((OH, OW) if c.noise == "const" else (c.N, 1, OH, OW), generator=g) * 0.3
    t["bias"] = torch.randn(c.O, generator=g) * 0.2 if c.bias else None
    t["f"] = setup_filter(c.taps)
    t["ns"] = torch.randn(c.N, c.O, generator=g) * 0.3 + 1.0
    if c.R:
        t["rgb_w"] = torch.randn(c.R, c.O, generator=g)
        t["rgb_s"] = (torch.randn(c.N, c.O, generator=g) * 0.3 + 1.0) / math.sqrt(c.O)
        t["rgb_b"] = torch.randn(c.R, generator=g) * 0.2
    return t


def case_ref(c, t, dtype=torch.float64):
    return modconv_ref(t["x"], t["w"], t["s"], up=c.up, demodulate=c.demod is not False, dcoef=t["dcoef"], noise=t["noise"], bias=t["bias"],
                       f=t["f"], act=c.act, alpha=c.alpha, gain=c.gain, clamp=c.clamp, mma=c.mma, dtype=dtype)
