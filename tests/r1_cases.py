"""Cases shared by the R1 penalty's tests (tests/test_r1_cpu.py, tests/test_hip_r1.py) and by the generator of their fixture
(tests/golden/make_golden_r1.py): the network-level run (the penalty of the small network of tests/discriminator_cases.py at two image
scales, and the gradient of its weighted mean for every parameter) written once for either implementation of DualDiscriminator and
for the float64 restatement; torch stand-ins of the three device operators of include/p3d_r1.h, written from the header's formulas;
float64 references of the single operators; the loss-level cases.  Not collected."""
import math

import torch
import torch.nn.functional as F

import discriminator_cases as DC
import loss_cases as LC
from train_step_cases import bias_act_backward_torch

GAMMA, GAIN = 10.0, 1.7
SCALES = {"s150": DC.IMG_SCALE, "s1": 1.0}  # the fixture network's own image scale (it reaches the clamp), and 1


def r1_inputs(scale):
    inp = DC.discriminator_inputs()
    k = scale / DC.IMG_SCALE
    return dict(inp, image=inp["image"] * k, image_raw=inp["image_raw"] * k)


def sumsq_torch(g_image, g_raw=None):
    s = g_image.square().sum(dim=list(range(1, g_image.ndim)))
    return s if g_raw is None else s + g_raw.square().sum(dim=list(range(1, g_raw.ndim)))


def run_network(forward, params, inp, device="cpu", penalty=sumsq_torch, guard=None, dtype=torch.float32):
    """loss_orthocondA.py:707-738's Dreg on a discriminator: forward(image, image_raw) -> logits; params: name -> leaf.  Returns the
    penalty [N], both image gradients (the first backward's results), and name -> gradient of (penalty * GAMMA / 2).mean() * GAIN for
    every parameter that received one.  guard: a context manager around the first backward (the reference's no_weight_gradients)."""
    image, raw = (inp[k].to(device=device, dtype=dtype).clone().requires_grad_(True) for k in ("image", "image_raw"))
    for p in params.values():
        p.grad = None
    logits = forward(image, raw)
    if guard is None:
        g_image, g_raw = torch.autograd.grad([logits.sum()], [image, raw], create_graph=True, only_inputs=True)
    else:
        with guard:
            g_image, g_raw = torch.autograd.grad([logits.sum()], [image, raw], create_graph=True, only_inputs=True)
    pen = penalty(g_image, g_raw)
    (pen * (GAMMA / 2)).mean().mul(GAIN).backward()
    return dict(penalty=pen.detach().cpu(), g_image=g_image.detach().cpu(), g_raw=g_raw.detach().cpu(),
                grads={n: p.grad.detach().cpu().clone() for n, p in params.items() if p.grad is not None})


def run_module(D, inp, device="cpu", **kw):
    """run_network on a DualDiscriminator module (the reference's or this package's)."""
    c, feats = inp["c"].to(device), inp["feats"].to(device)
    return run_network(lambda image, raw: D({"image": image, "image_raw": raw}, c.clone(), {"resnet_feats": feats}), dict(D.named_parameters()), inp,
                       device, **kw)


def run_f64(state, inp):
    """run_network on DC.discriminator_f64 in float64: the truth every binary32 run is measured against.  state: name -> tensor."""
    p64 = {n: v.detach().cpu().double().requires_grad_(True) for n, v in state.items()}
    return run_network(lambda image, raw: DC.discriminator_f64(p64, image, raw, inp["c"].double(), inp["feats"].double()), p64, inp,
                       dtype=torch.float64)


def err(a, b):
    return float((torch.as_tensor(a).double() - torch.as_tensor(b).double()).norm())


# ---- torch stand-ins of the device operators (include/p3d_r1.h), in the dtype of their arguments -----------------------------------
def conv2d_mask_impl_torch(h, wk, pre, act, gain, clamp, stride, pad, fault=None):
    """p3d_conv2d_mask_f32: the correlation, then the rule of bias_act's backward from pre.  fault 'nomask': the mask left out."""
    g = gain if gain is not None else (DC.SQRT2 if act == "lrelu" else 1.0)
    z = F.conv2d(h, DC.weight_of(wk), stride=stride, padding=pad)
    if fault == "nomask":
        return z * DC.R.f32(g)
    return bias_act_backward_torch(pre, z, 1 if act == "lrelu" else 0, 0.2, DC.R.f32(g), clamp)[0]


def mbstd_backward2_torch(x, gy, h, G, Fc, fault=None):
    """p3d_mbstd_backward2_f32 from the header's formulas.  fault 'no_d_term': the d_j * sum(h d) term dropped."""
    N, C, H, W = x.shape
    M, c = N // G, C // Fc
    kE = 1.0 / (G * c * H * W)
    out_dtype = x.dtype
    x, gy, h = x.double(), gy.double(), h.double()  # as the kernel: binary64 from the binary32 inputs, one rounding at the end
    xg, hg = x.reshape(G, M, C, H, W), h.reshape(G, M, C, H, W)
    d = xg - xg.mean(0)
    sd = (d.square().mean(0) + 1e-8).sqrt()                    # [M,C,H,W]
    hc = hg - hg.mean(0)
    s = (hc * d).sum(0)                                        # [M,C,H,W]
    gs = gy[:, C:].reshape(G, M, Fc, H * W).sum(dim=(0, 3))    # [M,F]
    gsc = gs[:, :, None].expand(M, Fc, c).reshape(1, M, C, 1, 1)
    second = 0 if fault == "no_d_term" else d * (s / (G * sd ** 3))[None]
    gx = kE * gsc * (hc / sd[None] - second)
    gg = kE * (s / sd).reshape(M, Fc, c * H * W).sum(-1)       # [M,F]
    g_extra = gg[None, :, :, None, None].expand(G, M, Fc, H, W).reshape(N, Fc, H, W).contiguous()
    return g_extra.to(out_dtype), gx.reshape(N, C, H, W).to(out_dtype)


def r1_sumsq_impl_torch(a, b):
    return sumsq_torch(a, b)


def install_ops(monkeypatch, ops):
    """DC.install_ops plus the three operators of include/p3d_r1.h, so that the recorded backward and the loss's Dreg run on CPU."""
    DC.install_ops(monkeypatch, ops)
    for name, fn in dict(_conv2d_mask_impl=conv2d_mask_impl_torch, mbstd_backward2=mbstd_backward2_torch, _r1_sumsq_impl=r1_sumsq_impl_torch).items():
        monkeypatch.setattr(ops, name, fn)


# ---- float64 references of the single operators -------------------------------------------------------------------------------------
MBSTD2_SHAPES = dict(DC.MBSTD_SHAPES, wide=(4, 2, 20, 1, 4, 4))  # wide: two groups, c * HW = 320 values per statistic > 256 lanes


def mbstd2_case(name):
    N, group, C, Fc, H, W = MBSTD2_SHAPES[name]
    g = torch.Generator().manual_seed(2100 + sorted(MBSTD2_SHAPES).index(name))
    return dict(x=torch.randn(N, C, H, W, generator=g), gy=torch.randn(N, C + Fc, H, W, generator=g), h=torch.randn(N, C, H, W, generator=g),
                group=group, F=Fc)


def mbstd2_autograd(c, dtype):
    """The double backward by torch autograd of DC.mbstd_any in `dtype`: with g_x = d <y, gy> / dx restricted to the statistic channels'
    share, the gradients of <g_x, h> with respect to gy's statistic channels and to x."""
    x, gy = c["x"].to(dtype).requires_grad_(True), c["gy"].to(dtype).requires_grad_(True)
    C = x.shape[1]
    y = DC.mbstd_any(x, c["group"], c["F"])
    gx, = torch.autograd.grad((y[:, C:] * gy[:, C:]).sum(), x, create_graph=True)
    g_gy, g_x = torch.autograd.grad((gx * c["h"].to(dtype)).sum(), [gy, x])
    return dict(g_extra=g_gy[:, C:].detach(), gx=g_x.detach())


def conv_layer2_f64(c, h):
    """One convolution layer's double backward in float64 from DC.conv_layer_f64's own operators: the gradients of <g_x, h> with respect
    to g_y, wk and the bias (the latter zero: the mask is piecewise constant), g_x the layer's input gradient."""
    d = torch.float64
    x, wk, bias, res, act, gain, clamp, stride, pad, gy = DC.conv_case_args(c)
    x, wk, gy = x.to(d).requires_grad_(True), wk.to(d).requires_grad_(True), gy.to(d).requires_grad_(True)
    bias = bias.to(d).requires_grad_(True) if bias is not None else None
    pre = DC.bias_act_any(F.conv2d(x, DC.weight_of(wk), stride=stride, padding=pad), bias, act, DC.R.f32(gain), None if clamp is None else DC.R.f32(clamp))
    gx, = torch.autograd.grad((pre * gy).sum(), x, create_graph=True)
    outs = torch.autograd.grad((gx * h.to(d)).sum(), [gy, wk] + ([bias] if bias is not None else []), allow_unused=True)
    return dict(g_gy=outs[0].detach(), g_wk=outs[1].detach(), g_bias=None if bias is None else (outs[2].detach() if outs[2] is not None else torch.zeros_like(bias)),
                gx=gx.detach())


def run_conv_layer2(ops, c, h, device, r1=True):
    """ops.conv2d_act(r1=True)'s recorded backward on one case, then the backward of <g_x, h>: (g_x, gradients towards g_y, wk, bias)."""
    t = {k: v.clone().to(device).requires_grad_(True) for k, v in c.items() if isinstance(v, torch.Tensor) and k in ("x", "wk", "bias", "res", "gy")}
    out = ops.conv2d_act(t["x"], t["wk"], t.get("bias"), act=c["act"], gain=c["gain"], clamp=c["clamp"], stride=c["stride"], pad=c["pad"],
                         res=t.get("res"), r1=r1)
    with ops.no_weight_gradients():
        gx, = torch.autograd.grad([out], [t["x"]], [t["gy"]], create_graph=True, only_inputs=True)
    (gx * h.to(device)).sum().backward()
    g = lambda k: t[k].grad.cpu() if k in t and t[k].grad is not None else None
    return dict(gx=gx.detach().cpu(), g_gy=g("gy"), g_wk=g("wk"), g_bias=g("bias"))


# ---- the loss-level cases -----------------------------------------------------------------------------------------------------------
PHASE_CASES = {
    "Dreg-s10": LC._case("Dreg", "s10"),
    "Dreg-s0": LC._case("Dreg", "s0"),
    "Dreg-single": LC._case("Dreg", "s1.5", dual_discrimination=False),
    "Dboth-s1.5": LC._case("Dboth", "s1.5"),
}


# ---- the network-level comparison (CPU stand-ins and the device) -------------------------------------------------------------------
MARGIN = 4.0          # this project's margin for another summation order
REPORT_BOUND = 1e-5   # the penalty and the image gradients, relative (loss_cases.compare_with_fixture's report bound)
_TRUTH = {}


def truth(D, tag):
    """run_f64 for the seeded network at one scale, computed once per process and shared (never modified)."""
    if tag not in _TRUTH:
        _TRUTH[tag] = run_f64({n: p for n, p in D.named_parameters()}, r1_inputs(SCALES[tag]))
    return _TRUTH[tag]


def network_against_fixture(P, device, tag, golden, run=None):
    """One network case: the seeded DualDiscriminator with set_r1_grad() runs run_module with ops.r1_penalty inside
    ops.no_weight_gradients().  Penalty and image gradients to REPORT_BOUND relative (of the largest magnitude) against the fixture and
    float64; the parameters with a gradient are the fixture's, the reference's all-zero gradients are all-zero here; for every
    parameter, on the stored sample, |ours - f64| <= MARGIN |reference - f64| (L2), and the full norm to MARGIN times the same error.
    Returns name -> the ratio |ours - f64| / |reference - f64|."""
    D = DC.fill_discriminator(P.DualDiscriminator(**DC.D_KW)).to(device)
    D.set_r1_grad(True)
    inp = r1_inputs(SCALES[tag])
    ours = (run or run_module)(D, inp, device, penalty=P.ops.r1_penalty, guard=P.ops.no_weight_gradients())
    t64 = truth(D, tag)
    ratios, bad = {}, []
    for k in ("penalty", "g_image", "g_raw"):
        ref32, ref64 = torch.from_numpy(golden[f"{tag}|{k}"]), t64[k]
        top = float(ref64.abs().max())
        e32, e64, r64 = float((ours[k] - ref32).abs().max()) / top, float((ours[k].double() - ref64).abs().max()) / top, float((ref32.double() - ref64).abs().max()) / top
        print(f"{tag} {k}: max |.| {top:.3e}; ours vs reference {e32:.2e}, ours vs float64 {e64:.2e} (reference vs float64 {r64:.2e})")
        if not (e32 <= REPORT_BOUND and e64 <= REPORT_BOUND):
            bad.append((k, e32, e64))
    names = golden[f"{tag}|names"].tolist()
    assert sorted(ours["grads"]) == names, (sorted(set(names) ^ set(ours["grads"])))
    assert sorted(t64["grads"]) == names
    for n in names:
        ref32, g64, g = torch.from_numpy(golden[f"{tag}|g|{n}"]), t64["grads"][n], ours["grads"][n]
        assert torch.isfinite(g).all(), n
        if not ref32.any() and float(golden[f"{tag}|n|{n}"]) == 0.0:
            assert not g.any(), f"{n}: the reference's gradient is exactly zero"
            ratios[n] = 0.0
            continue
        e_ours, e_ref = err(DC.dsub(g), DC.dsub(g64)), err(ref32, DC.dsub(g64))
        n_ours, n_ref, n64 = float(g.double().norm()), float(golden[f"{tag}|n|{n}"]), float(g64.norm())
        ratios[n] = e_ours / e_ref if e_ref > 0 else (0.0 if e_ours == 0 else math.inf)
        print(f"{tag} {n}: |g| {n64:.3e}; |ours - f64| {e_ours:.3e}, |reference - f64| {e_ref:.3e}, ratio {ratios[n]:.3f}; "
              f"rel {e_ours / max(n64, 1e-300):.2e}; norm ours {n_ours:.6e} reference {n_ref:.6e} f64 {n64:.6e}")
        if not e_ours <= MARGIN * e_ref:
            bad.append((n, e_ours, e_ref))
    assert not bad, bad
    return ratios


# ---- the single operators' gates ------------------------------------------------------------------------------------------------------
def conv2d_mask_f64(h, wk, pre, act, gain, clamp, stride, pad):
    """p3d_conv2d_mask_f32 in float64 with the masks of the binary32 pre: (result, sum of |terms|, K) for DC's layer gate."""
    taps, Ci, Co = wk.shape
    z, absz = DC.R.conv_dgrad_ref(h, wk, Co, pre.shape[2], pre.shape[3], stride, pad)
    keep, neg = DC.R.bias_act_masks(pre, 1 if act == "lrelu" else 0, clamp)
    m = keep.double() * torch.where(neg, 0.2, 1.0).double() * DC.R.f32(gain)
    return z * m, absz * m.abs(), taps * Ci + 2


def mask_case(shape, variant):
    """A tangent-layer case on DC's conv case: h in the input's place, pre the layer's own binary32 output before the residual."""
    c = DC.conv_case(shape, variant)
    x, wk, bias, res, act, gain, clamp, stride, pad, gy = DC.conv_case_args(c)
    g = torch.Generator().manual_seed(3000 + 17 * sorted(DC.CONV_SHAPES).index(shape) + 101 * sorted(DC.CONV_VARIANTS).index(variant))
    pre = DC.conv2d_act_impl_torch(x, wk, bias, act, gain, clamp, stride, pad, None)
    return dict(c, h=torch.randn(x.shape, generator=g), pre=pre, gain_value=gain)


def mbstd2_gate(got, c, verbose=""):
    """Per output (the statistic channels' gradient, x's gradient): |got - f64| <= MARGIN |torch's own binary32 double autograd - f64|,
    all three of the same function DC.mbstd_any on the same inputs.  Returns (what failed, name -> ratio)."""
    r64, r32 = mbstd2_autograd(c, torch.float64), mbstd2_autograd(c, torch.float32)
    bad, ratios = [], {}
    for k in ("g_extra", "gx"):
        e, e32 = err(got[k], r64[k]), err(r32[k], r64[k])
        ratios[k] = e / e32 if e32 > 0 else (0.0 if e == 0 else math.inf)
        print(f"{verbose}mbstd2 {k}: |got - f64| {e:.3e}, |torch binary32 - f64| {e32:.3e}, ratio {ratios[k]:.3f} of {MARGIN:g}; rel {e / float(r64[k].norm()):.2e}")
        if not e <= MARGIN * e32:
            bad.append(k)
    return bad, ratios


def run_mbstd2(ops, c, device):
    """ops.minibatch_std(r1=True): the recorded first backward, then the backward of <g_x, h>; the statistic's share alone (the copied
    channels' cotangent is zeroed, so that g_x is mbstd_backward's result)."""
    x = c["x"].clone().to(device).requires_grad_(True)
    C = x.shape[1]
    gy = c["gy"].clone()
    gy[:, :C] = 0
    gy = gy.to(device).requires_grad_(True)
    y = ops.minibatch_std(x, c["group"], c["F"], r1=True)
    gx, = torch.autograd.grad([y], [x], [gy], create_graph=True)
    (gx * c["h"].to(device)).sum().backward()
    return dict(g_extra=gy.grad[:, C:].cpu(), gx=x.grad.cpu(), first=gx.detach().cpu())
