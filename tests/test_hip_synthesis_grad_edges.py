"""GPU (-m gpu): the synthesis backward at ragged shapes against float64 (include/p3d_synthesis_grad.h).

Kernel level: ops.conv_dgrad / conv_wgrad / mod_backward / bias_act_backward on the designed matrix of
tests/synthesis_grad_cases.py (every GEMM tile and K-chunk tail, non-square maps, every documented index map, several wgrad slabs
with a ragged last one, per-sample g_d), each against the float64 reference written from the header (tests/synthesis_grad_ref.py)
under its element-wise gate; bias_act's mask decisions exactly and its values within 2 ulp; two calls give the same bits.
Layer level: modulated_conv2d / torgb / upsample2d under autograd at ragged shapes against float64 autograd, with the branch
decisions of the HIP forward (synthesis_grad_ref.act_masked); and the noise shapes the forward accepts."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import synthesis_grad_cases as SC
import synthesis_grad_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def P():
    import panic3d_amd
    panic3d_amd.build()
    panic3d_amd._lib.lib()
    return panic3d_amd


def _ids(c):
    return "-".join(map(str, c)) if isinstance(c, tuple) else str(c)


# ---- kernel level ----------------------------------------------------------------------------------------------------------
def _dgrad_inputs(case):
    N, Ci, Co, Hi, Wi, Ho, Wo, taps, stride, pad = case
    gen = torch.Generator().manual_seed(N * 7919 + Ci * 131 + Co * 17 + Hi * 5 + Wi + taps + stride * 3 + pad)
    return torch.randn(N, Ci, Hi, Wi, generator=gen), torch.randn(taps, Ci, Co, generator=gen)


@pytest.mark.parametrize("case", SC.DGRAD_CASES, ids=_ids)
def test_conv_dgrad_vs_float64(P, case):
    N, Ci, Co, Hi, Wi, Ho, Wo, taps, stride, pad = case
    g, wk = _dgrad_inputs(case)
    out = P.ops.conv_dgrad(g.to(DEV), wk.to(DEV), Co, Ho, Wo, stride, pad)
    ref, absref = R.conv_dgrad_ref(g, wk, Co, Ho, Wo, stride, pad)
    R.gate("dgrad " + _ids(case), out, ref, absref, taps * Ci)


def _wgrad_inputs(case):
    (kind, N, O, I, Hd, Wd), use_s, with_gd = case
    taps, gmap, xmap, gsz, xsz = SC.WGRAD_MAPS[kind]
    gen = torch.Generator().manual_seed(N * 7919 + O * 131 + I * 17 + Hd * 5 + Wd + taps)
    g = torch.randn(N, O, *gsz(Hd, Wd), generator=gen)
    x = torch.randn(N, I, *xsz(Hd, Wd), generator=gen)
    s = torch.randn(N, I, generator=gen) * 0.5 + 1.0 if use_s else None
    wk = torch.randn(taps, O, I, generator=gen) if with_gd else None
    ds = torch.rand(N, O, generator=gen) + 0.5 if with_gd else None  # a different coefficient for every (sample, channel)
    return taps, gmap, xmap, g, x, s, wk, ds


def _wgrad_call(P, case, g, x, s, wk, ds):
    (kind, N, O, I, Hd, Wd), _, _ = case
    taps, gmap, xmap = SC.WGRAD_MAPS[kind][:3]
    d = lambda t: t.to(DEV) if t is not None else None
    return P.ops.conv_wgrad(d(g), gmap, d(x), d(s), xmap, taps, (Hd, Wd), wk=d(wk), dscale=d(ds))


@pytest.mark.parametrize("case", SC.WGRAD_CASES, ids=_ids)
def test_conv_wgrad_vs_float64(P, case):
    (kind, N, O, I, Hd, Wd), use_s, with_gd = case
    taps, gmap, xmap, g, x, s, wk, ds = _wgrad_inputs(case)
    dw, gd = _wgrad_call(P, case, g, x, s, wk, ds)
    ref = R.conv_wgrad_ref(g, gmap, x, s, xmap, taps, (Hd, Wd), wk=wk, dscale=ds)
    print("slabs, pixels per slab:", R.sg_split(N, O, I, taps, Hd, Wd))
    R.gate("dw " + _ids(case), dw, ref["dw"], ref["abs_dw"], N * Hd * Wd)
    if with_gd:  # the sample's own dW_n (K = its pixels) under a sum over taps and input channels
        R.gate("g_d " + _ids(case), gd, ref["g_d"], ref["abs_g_d"], int((np.sqrt(Hd * Wd) + np.sqrt(taps * I)) ** 2))
    else:
        assert gd is None


@pytest.mark.parametrize("case", SC.MOD_CASES, ids=_ids)
def test_mod_backward_vs_float64(P, case):
    N, C, HW = case
    gen = torch.Generator().manual_seed(N * 1000 + C * 10 + HW)
    x, g = torch.randn(N, C, HW, generator=gen), torch.randn(N, C, HW, generator=gen)
    s = torch.randn(N, C, generator=gen)
    gd = g.to(DEV)
    gs = P.ops.mod_backward(x.to(DEV), s.to(DEV), gd)
    ref, absref, gscaled = R.mod_backward_ref(x, s, g)
    R.gate("g_s " + _ids(case), gs, ref, absref, HW)
    assert torch.equal(gd.cpu(), gscaled.float())  # one fp32 product per element: exact


def _bias_act_inputs(case):
    N, C, HW, act, alpha, gain, clamp, with_ds, alias, noise = case
    gen = torch.Generator().manual_seed(N * 1000 + C * 10 + HW + act)
    y = torch.randn(N, C, HW, generator=gen) * 1.5
    flat = y.view(-1)
    if clamp is not None:
        c = R.f32(clamp)
        y.clamp_(-c, c)  # the forward's clipped output: many elements at |y| == clamp exactly
        flat[3::13] = c
        flat[5::13] = -c
    flat[::7] = 0.0   # y == 0 exactly: alpha under lrelu, 1 under linear
    flat[1::11] = -0.0
    gy = torch.randn(N, C, HW, generator=gen)
    ds = torch.rand(N, C, generator=gen) + 0.5 if with_ds else None
    return y, gy, ds


def _bias_act_call(P, case, y, gy, ds):
    N, C, HW, act, alpha, gain, clamp, with_ds, alias, noise = case
    y, gy = y.to(DEV), gy.to(DEV).clone()
    ds = ds.to(DEV) if ds is not None else None
    if not alias:
        return P.ops.bias_act_backward(y, gy, act, alpha, gain, clamp, dscale=ds, want_noise=noise)
    # g_out aliasing g_y (the header allows it): the C ABI directly, the wrapper allocates its own output
    gb = torch.empty((N, C), dtype=torch.float32, device=DEV)
    gn = torch.empty((N, HW), dtype=torch.float32, device=DEV) if noise else None
    p = P.ops._p
    with P.ops._on(y.device):
        rc = P._lib.lib().p3d_bias_act_backward_f32(p(y), p(gy), N, C, HW, act, float(alpha), float(gain),
                                                     float(clamp if clamp is not None else -1), p(ds), p(gy), p(gb), p(gn), P.ops._stream())
    P._lib.check(rc, "p3d_bias_act_backward_f32")
    return gy, gb, gn


@pytest.mark.parametrize("case", SC.BIAS_ACT_CASES, ids=_ids)
def test_bias_act_backward_vs_float64(P, case):
    N, C, HW, act, alpha, gain, clamp, with_ds, alias, noise = case
    y, gy, ds = _bias_act_inputs(case)
    out, gb, gn = _bias_act_call(P, case, y, gy, ds)
    ref = R.bias_act_backward_ref(y, gy, act, alpha, gain, clamp, ds)
    out = out.cpu()
    assert torch.equal(out == 0, ref["g_out"] == 0)  # the mask decisions, exactly (g_y has no zeros)
    u = R.ulp_distance(out, ref["g_out"])
    print(f"g_out {_ids(case)}: worst {u:.2f} ulp")
    assert u <= R.ULP_MAX, u
    keep, neg = R.bias_act_masks(y, act, clamp)
    if clamp is not None:
        assert (out[y.abs() == R.f32(clamp)] == 0).all() and (y.abs() == R.f32(clamp)).any()
    z = (y == 0) & keep
    assert z.any() or not keep.any()
    want = gy[z].double() * R.f32(gain) * (R.f32(alpha) if act == 1 else 1.0) * (ds[:, :, None].expand_as(y)[z].double() if ds is not None else 1.0)
    assert R.ulp_distance(out[z], want) <= R.ULP_MAX
    R.gate("g_bias " + _ids(case), gb, ref["g_bias"], ref["abs_bias"], HW)
    if noise:
        R.gate("g_noise " + _ids(case), gn, ref["g_noise"], ref["abs_noise"], C)
    else:
        assert gn is None


def test_backward_kernels_reproduce_bitwise(P):
    """The header's promise: the same sizes give the same bits, run to run, at ragged shapes of every kernel."""
    for case in (SC.DGRAD_CASES[5], SC.DGRAD_CASES[27], SC.DGRAD_CASES[-2]):
        g, wk = _dgrad_inputs(case)
        N, Ci, Co, Hi, Wi, Ho, Wo, taps, stride, pad = case
        a, b = (P.ops.conv_dgrad(g.to(DEV), wk.to(DEV), Co, Ho, Wo, stride, pad) for _ in range(2))
        assert torch.equal(a, b), case
    for case in (SC.WGRAD_CASES[5], SC.WGRAD_CASES[13], SC.WGRAD_CASES[17]):
        taps, gmap, xmap, g, x, s, wk, ds = _wgrad_inputs(case)
        a, b = (_wgrad_call(P, case, g, x, s, wk, ds) for _ in range(2))
        assert torch.equal(a[0], b[0]) and (a[1] is None or torch.equal(a[1], b[1])), case
    for case in (SC.BIAS_ACT_CASES[3], SC.BIAS_ACT_CASES[6]):
        y, gy, ds = _bias_act_inputs(case)
        a, b = (_bias_act_call(P, case, y, gy, ds) for _ in range(2))
        assert all(torch.equal(u, v) for u, v in zip(a, b) if u is not None), case
    for N, C, HW in ((3, 17, 4099), (3, 130, 257)):
        gen = torch.Generator().manual_seed(HW)
        x, g, s = torch.randn(N, C, HW, generator=gen).to(DEV), torch.randn(N, C, HW, generator=gen).to(DEV), torch.randn(N, C, generator=gen).to(DEV)
        g1, g2 = g.clone(), g.clone()
        assert torch.equal(P.ops.mod_backward(x, s, g1), P.ops.mod_backward(x, s, g2)) and torch.equal(g1, g2)


# ---- layer level: modulated_conv2d under autograd --------------------------------------------------------------------------------
def _modconv64(x, w, s, d, b, noise, up, ks, f, y_ours, act, gain, clamp):
    xm = x * s[:, :, None, None]
    if ks == 1:
        y = F.conv2d(xm, w)
    elif up == 1:
        y = F.conv2d(xm, w, padding=1)
    else:
        y = F.conv_transpose2d(xm, w.transpose(0, 1), stride=2)
        y = F.conv2d(F.pad(y, [1, 1, 1, 1]), R.fir_ref(f)[None, None].repeat(y.shape[1], 1, 1, 1), groups=y.shape[1])
    if d is not None:
        y = y * d[:, :, None, None]
    if noise is not None:
        y = y + noise
    if b is not None:
        y = y + b[None, :, None, None]
    g = gain if gain is not None else (float(np.sqrt(2)) if act == "lrelu" else 1.0)
    return R.act_masked(y, y_ours, 0.2, g, clamp, act)


# (I, O, H, W, up, ks, noise kind, operands, options): N = 3 throughout.  Options: demodulate / act / bias / gain / clamp overrides,
# and `grad` = which inputs require grad (all by default)
MODCONV_CASES = [
    (20, 70, 13, 13, 1, 3, "const", "f32", {}),  # the forward test's ragged shapes
    (35, 10, 9, 9, 2, 3, "random", "f32", {"clamp": 0.5}),
    (19, 5, 11, 11, 1, 1, None, "f32", {"demodulate": False, "act": "linear", "gain": 1.0}),
    (515, 64, 8, 8, 1, 3, "random", "f32", {}),
    (131, 64, 16, 16, 2, 3, "const", "f32", {"clamp": 0.5}),
    (33, 17, 7, 7, 1, 1, "random", "f32", {"demodulate": False}),  # 1x1 with noise, lrelu, demodulate=False
    (40, 24, 7, 13, 1, 3, "random", "f32", {"bias": False, "gain": None}),  # non-square
    (24, 16, 5, 9, 2, 3, "const", "f32", {"act": "linear", "clamp": 0.5}),  # non-square up-sampling
    (17, 33, 6, 6, 1, 3, "random", "f32", {"demodulate": False, "bias": False}),
    (64, 96, 8, 8, 1, 3, "random", "x2", {"clamp": 0.5}),  # two-term operands (I % 16 == 0)
    (128, 64, 8, 8, 2, 3, "const", "x2", {}),
    (64, 40, 6, 10, 1, 3, "const", "x2", {}),  # non-square, two-term
    (64, 40, 10, 10, 1, 3, "random", "f16", {}),  # the one-term f16 forward
    (32, 24, 6, 6, 2, 3, "const", "f16", {"clamp": 0.5}),
    (20, 70, 13, 13, 1, 3, "random", "f32", {"grad": ("x",)}),  # only some inputs require grad
    (35, 10, 9, 9, 2, 3, "const", "f32", {"grad": ("weight",)}),
    (20, 24, 7, 9, 1, 3, "random", "f32", {"grad": ("noise",)}),
    (35, 10, 9, 9, 2, 3, "const", "f32", {"grad": ("noise",)}),
    (19, 5, 11, 11, 1, 1, None, "f32", {"grad": ("styles", "dcoef")}),
]
NAMES = ("x", "weight", "styles", "dcoef", "bias", "noise")


@pytest.mark.parametrize("case", MODCONV_CASES, ids=lambda c: _ids(c[:8]) + ("-" + "-".join(f"{k}={v}" for k, v in c[8].items()) if c[8] else ""))
def test_modconv_gradients_at_ragged_shapes_vs_float64(P, case):
    I, O, H, W, up, ks, nk, mma, opt = case
    N = 3
    demod = opt.get("demodulate", True)
    act = opt.get("act", "lrelu")
    gain = opt["gain"] if "gain" in opt else (float(np.sqrt(2)) if act == "lrelu" else 1.0)  # None: the activation's default
    clamp = opt.get("clamp")
    want = opt.get("grad", NAMES)
    gen = torch.Generator().manual_seed(I * 131 + O * 7 + H * 3 + W + up + ks + len(want))
    x = torch.randn(N, I, H, W, generator=gen)
    w = torch.randn(O, I, ks, ks, generator=gen)
    s = torch.randn(N, I, generator=gen) * 0.5 + 1.0
    d = ((w.square().sum(dim=(2, 3))[None] * s.square()[:, None, :]).sum(dim=2) + 1e-8).rsqrt() if demod else None
    b = torch.randn(O, generator=gen) * 0.2 if opt.get("bias", True) else None
    Ho, Wo = H * up, W * up
    noise = None if nk is None else torch.randn((Ho, Wo) if nk == "const" else (N, 1, Ho, Wo), generator=gen) * 0.3
    gy = torch.randn(N, O, Ho, Wo, generator=gen)
    f = P.ops.setup_filter([1, 3, 3, 1])
    vals = dict(x=x, weight=w, styles=s, dcoef=d, bias=b, noise=noise)
    dv = {k: (v.to(DEV).requires_grad_(k in want) if v is not None else None) for k, v in vals.items()}
    wf = None
    if mma == "x2":
        wf = P.ops.conv_weights_to_f16(dv["weight"].detach(), split=True, layout=P.ops.conv_weight_layout(I, O, W, up) if ks == 3 else 0)
    elif mma == "f16":
        wf = P.ops.conv_weights_to_f16(dv["weight"].detach())
    y = P.ops.modulated_conv2d(dv["x"], dv["weight"], dv["styles"], noise=dv["noise"], up=up, padding=ks // 2, resample_filter=f.to(DEV),
                               demodulate=demod, bias=dv["bias"], act=act, gain=gain, clamp=clamp, weight_f16=wf,
                               dcoef=dv["dcoef"])
    assert y.grad_fn is not None and tuple(y.shape) == (N, O, Ho, Wo)
    (y * gy.to(DEV)).sum().backward()
    ref = {k: (v.double().requires_grad_(k in want) if v is not None else None) for k, v in vals.items()}
    y64 = _modconv64(ref["x"], ref["weight"], ref["styles"], ref["dcoef"], ref["bias"], ref["noise"], up, ks, f, y.detach().cpu().double(),
                     act, gain, clamp)
    # the one-term f16 forward rounds the operands to f16; its backward is the fp32 one, on the forward's branch decisions
    assert R.rel_l2(y.detach().cpu(), y64.detach()) < (2e-3 if mma == "f16" else 1e-5)
    (y64 * gy.double()).sum().backward()
    for k in NAMES:
        a, r = dv[k], ref[k]
        if a is None:
            continue
        if k not in want:
            assert a.grad is None, k
            continue
        assert a.grad is not None and a.grad.shape == a.shape, k
        e = R.rel_l2(a.grad.cpu(), r.grad)
        print(f"{k}: rel-L2 {e:.2e}")
        assert e <= R.REL_L2, (k, e)


def test_modconv_noise_shapes(P):
    """[H,W], [1,1,H,W] (shared) and [N,1,H,W] (per sample) are accepted, forward and backward agreeing on which; any other layout
    with N·H·W elements ([N,H,W], [N,H·W], [N,1,H·W]) raises instead of being read as one shared map."""
    N, I, O, H = 3, 16, 8, 5
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(N, I, H, H, generator=gen).to(DEV)
    w = torch.randn(O, I, 3, 3, generator=gen).to(DEV)
    s = (torch.randn(N, I, generator=gen) + 1).to(DEV)
    nz = torch.randn(N, 1, H, H, generator=gen).to(DEV)
    kw = dict(up=1, padding=1, demodulate=False, act="linear", gain=1.0)
    with torch.no_grad():
        base = P.ops.modulated_conv2d(x, w, s, **kw)
        per = P.ops.modulated_conv2d(x, w, s, noise=nz, **kw)
        assert torch.allclose(per - base, nz.expand(N, O, H, H), atol=1e-5)  # each sample its own map
        for shared in (nz[1, 0], nz[1:2]):
            y = P.ops.modulated_conv2d(x, w, s, noise=shared.contiguous(), **kw)
            assert torch.allclose(y - base, nz[1:2].expand(N, O, H, H), atol=1e-5)
        for bad in (nz.reshape(N, H, H), nz.reshape(N, H * H), nz.reshape(N, 1, H * H), nz.reshape(1, N, H, H)):
            with pytest.raises(RuntimeError, match="noise must be"):
                P.ops.modulated_conv2d(x, w, s, noise=bad.contiguous(), **kw)
    gy = torch.randn(N, O, H, H, generator=gen).to(DEV)
    for shape in ((H, H), (1, 1, H, H), (N, 1, H, H)):
        n = torch.zeros(shape, device=DEV, requires_grad=True)
        (P.ops.modulated_conv2d(x, w, s, noise=n, **kw) * gy).sum().backward()
        want = gy.sum(1, keepdim=True) if shape[0] == N else gy.sum((0, 1))
        assert n.grad.shape == n.shape and torch.allclose(n.grad, want.reshape(shape), rtol=1e-5, atol=1e-5), shape
    with pytest.raises(RuntimeError, match="noise must be"):
        P.ops.modulated_conv2d(x, w, s, noise=torch.zeros(N, H, H, device=DEV, requires_grad=True), **kw)


# ---- layer level: ToRGB and upsample2d under autograd -----------------------------------------------------------------------------
@pytest.mark.parametrize("O,I,H,W,skip,clamp", [(3, 40, 8, 8, True, None), (17, 72, 6, 10, True, 0.5), (32, 131, 7, 9, False, 0.5),
                                                (33, 40, 12, 8, True, None), (96, 72, 5, 7, False, None), (96, 131, 8, 12, True, 0.5)])
def test_torgb_gradients_at_ragged_shapes_vs_float64(P, O, I, H, W, skip, clamp):
    N = 3
    gen = torch.Generator().manual_seed(O * 1000 + I * 10 + H + W)
    x = torch.randn(N, I, H, W, generator=gen)
    w = torch.randn(O, I, 1, 1, generator=gen)
    s = torch.randn(N, I, generator=gen) / np.sqrt(I)
    b = torch.randn(O, generator=gen) * 0.2
    sk = torch.randn(N, O, H // 2, W // 2, generator=gen) if skip else None
    f = P.ops.setup_filter([1, 3, 3, 1])
    gi = torch.randn(N, O, H, W, generator=gen)
    leaves = [t.to(DEV).requires_grad_(True) for t in (x, w, s, b)] + ([sk.to(DEV).requires_grad_(True)] if skip else [])
    img = P.ops.torgb(leaves[0], P.ops.torgb_weights(leaves[1]), O, leaves[2], bias=leaves[3], clamp=clamp,
                      skip=leaves[4] if skip else None, skip_filter=f.to(DEV))
    (img * gi.to(DEV)).sum().backward()
    with torch.no_grad():
        ylin = P.ops.torgb(leaves[0], P.ops.torgb_weights(leaves[1]), O, leaves[2], bias=leaves[3]).cpu().double()
    if clamp is not None:
        assert (ylin.abs() >= clamp).float().mean() > 0.1  # a clamp that clips
    ref = [t.double().requires_grad_(True) for t in ((x, w, s, b) + ((sk,) if skip else ()))]
    z = F.conv2d(ref[0] * ref[2][:, :, None, None], ref[1]) + ref[3][None, :, None, None]
    if clamp is not None:
        z = torch.where(ylin.abs() < clamp, z, z.detach().clamp(-clamp, clamp))
    if skip:
        z = z + R.upsample2d_ref(ref[4], f)
    assert R.rel_l2(img.detach().cpu(), z.detach()) < 1e-5
    (z * gi.double()).sum().backward()
    for name, a, r in zip(("x", "weight", "styles", "bias", "skip"), leaves, ref):
        e = R.rel_l2(a.grad.cpu(), r.grad)
        print(f"{name}: rel-L2 {e:.2e}")
        assert e <= R.REL_L2, (name, e)


@pytest.mark.parametrize("N,C,H,W,padding", [(3, 5, 7, 11, 0), (2, 3, 5, 4, [1, 0, 2, 1]), (1, 4, 9, 6, [0, 2, 1, 0]), (3, 2, 1, 3, 0)])
def test_upsample2d_gradient_vs_float64(P, N, C, H, W, padding):
    gen = torch.Generator().manual_seed(N * 100 + C * 10 + H + W)
    x = torch.randn(N, C, H, W, generator=gen)
    f = P.ops.setup_filter([1, 3, 3, 1])
    xd = x.to(DEV).requires_grad_(True)
    y = P.ops.upsample2d(xd, f.to(DEV), up=2, padding=padding)
    assert y.grad_fn is not None
    x64 = x.double().requires_grad_(True)
    y64 = R.upsample2d_ref(x64, f, 2, padding)
    assert y.shape == y64.shape and R.rel_l2(y.detach().cpu(), y64.detach()) < 1e-6
    gy = torch.randn(y.shape, generator=gen)
    (y * gy.to(DEV)).sum().backward()
    (y64 * gy.double()).sum().backward()
    e = R.rel_l2(xd.grad.cpu(), x64.grad)
    assert e < 1e-6, e
