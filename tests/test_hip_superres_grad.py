"""GPU (-m gpu): the HIP backward of the 512^2 super-resolution (TriPlaneGenerator.set_superresolution_grad).

The combined-ToRGB backward (p3d_torgb_combine_backward_f32) at ragged shapes against float64, with the clamp mask taken exactly from
the forward's own pre-clamp sums; the grad-mode image against the no-grad call's bits in both operand modes (the ToRGB layers still
riding on conv1 in the default mode); the module's gradients against the reference's fp32 autograd (tests/golden/sr_grad.npz) and the
full-size module against a float64 restatement; G.f end to end; the launch replay around grad-mode calls; the paste's refusal; and the
default (switch off) unchanged."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import p3d_testing as T
import superres_grad_cases as SRC
import synthesis_grad_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def P():
    import panic3d_amd
    panic3d_amd.build()
    panic3d_amd._lib.lib()
    return panic3d_amd


# ---- kernel level ----------------------------------------------------------------------------------------------------------------
# (tiles, N, R, H, W, clamp, skip, bias): tiles 1..4, non-square maps off multiples of 16 / 256, N 1 and 2, clamps that clip on
# both sides, skip on and off
COMBINE_CASES = [(1, 1, 3, 6, 10, 0.8, True, True), (2, 2, 3, 14, 22, 1.0, False, True), (3, 1, 1, 34, 18, None, True, True),
                 (4, 2, 4, 40, 66, 1.5, True, False), (4, 1, 3, 512, 512, 256.0, True, True), (2, 2, 3, 256, 130, 0.9, True, True),
                 (1, 2, 2, 2, 2, 0.3, True, True)]


def _combine_inputs(case):
    tiles, N, Rc, H, W, clamp, skip, bias = case
    gen = torch.Generator().manual_seed(tiles * 1000 + N * 100 + Rc * 10 + H + W)
    scale = 1.0 if clamp is None or clamp < 10 else 100.0
    part = torch.randn(tiles, N, Rc, H, W, generator=gen) * scale
    b = (torch.randn(Rc, generator=gen) * 0.3 * scale if clamp is None or clamp < 10 else torch.tensor([255.0, -255.0, 0.0, 10.0][:Rc])) \
        if bias else None
    g_img = torch.randn(N, Rc, H, W, generator=gen)
    return part, b, g_img


@pytest.mark.parametrize("case", COMBINE_CASES, ids=lambda c: "-".join(map(str, c)))
def test_torgb_combine_backward_vs_float64(P, case):
    tiles, N, Rc, H, W, clamp, skip, bias = case
    part, b, g_img = _combine_inputs(case)
    f = P.ops.setup_filter([1, 3, 3, 1])
    d = lambda t: t.to(DEV) if t is not None else None
    # the forward's own pre-clamp sums: the combine launch without clamp and skip (the same additions in the same order)
    v = P.ops.torgb_combine(d(part), bias=d(b)).cpu()
    keep = torch.ones_like(v, dtype=torch.bool) if clamp is None else v.double().abs() < R.f32(clamp)
    if clamp is not None:
        assert (~keep & (v > 0)).any() and (~keep & (v < 0)).any() and keep.any()  # the clamp clips on both sides
    outs = [P.ops.torgb_combine_backward(d(part), d(g_img), bias=d(b), clamp=clamp, skip_filter=d(f) if skip else None, want_bias=bias)
            for _ in range(2)]
    g_y, g_b, g_skip = outs[0]
    assert torch.equal(g_y.cpu(), torch.where(keep, g_img, torch.zeros_like(g_img)))  # the mask, exactly
    gz = torch.where(keep, g_img.double(), torch.zeros_like(g_img, dtype=torch.float64))
    if bias:
        R.gate("g_bias", g_b.cpu(), gz.sum((0, 2, 3)), gz.abs().sum((0, 2, 3)), N * H * W)
    else:
        assert g_b is None
    if skip:
        s64 = torch.zeros(N, Rc, H // 2, W // 2, dtype=torch.float64, requires_grad=True)
        (R.upsample2d_ref(s64, f) * g_img.double()).sum().backward()
        a64 = torch.zeros_like(s64, requires_grad=True)
        (R.upsample2d_ref(a64, f) * g_img.double().abs()).sum().backward()  # (the filter is non-negative: the |.| sum)
        R.gate("g_skip", g_skip.cpu(), s64.grad, a64.grad, 16)
    else:
        assert g_skip is None
    for a, c in zip(outs[0], outs[1]):  # bitwise reproducible
        assert (a is None and c is None) or torch.equal(a, c)


def test_torgb_combine_backward_argument_errors(P):
    import ctypes as C
    L = P._lib.lib()
    f = C.c_void_p(256)
    assert L.p3d_torgb_combine_backward_f32(None, 1, 1, 3, 4, 4, None, -1.0, f, f, None, None, None, None) == -1
    assert L.p3d_torgb_combine_backward_f32(f, 0, 1, 3, 4, 4, None, -1.0, f, f, None, None, None, None) == -1
    assert L.p3d_torgb_combine_backward_f32(f, 1, 1, 3, 4, 4, None, -1.0, f, f, None, None, f, None) == -1  # g_skip without filter
    assert L.p3d_torgb_combine_backward_f32(f, 1, 1, 3, 5, 4, None, -1.0, f, f, None, f, f, None) == -2  # odd map with a skip


# ---- the module -----------------------------------------------------------------------------------------------------------------
def _sr(P, seed=41):
    return SRC.fill(P.generator.SuperresolutionHybrid8XDC(**SRC.SR_KW), seed).to(DEV).eval()


def _sr_f16(sr, P):  # what TriPlaneGenerator.set_sr_mma_f16 does to its super-resolution
    for m in sr.modules():
        if isinstance(m, (P.stylegan2.SynthesisLayer, P.stylegan2.ToRGBLayer)):
            m.mma_f16 = True


def _leaves():
    rgb, x, ws, g_out, chk = SRC.draws()
    return [t.to(DEV).requires_grad_(True) for t in (rgb, x, ws)] + [g_out.to(DEV)]


@pytest.mark.parametrize("mode", ["default", "f16"])
def test_grad_mode_image_equals_no_grad_image_and_grads_reproduce(P, monkeypatch, mode):
    sr = _sr(P)
    if mode == "f16":
        _sr_f16(sr, P)
    rgb, x, ws, g_out = _leaves()
    with torch.no_grad():
        ref = sr(rgb, x, ws, noise_mode="const").clone()
    sr.record_grad = True
    seen = []
    real = P.ops.torgb_combine
    monkeypatch.setattr(P.ops, "torgb_combine", lambda *a, **k: (seen.append("x" in k), real(*a, **k))[1])
    grads = []
    for _ in range(2):
        for t in [rgb, x, ws] + list(sr.parameters()):
            t.grad = None
        out = sr(rgb, x, ws, noise_mode="const")
        assert out.grad_fn is not None
        assert torch.equal(out.detach(), ref)
        (out * g_out).sum().backward()
        grads.append([t.grad.clone() for t in [rgb, x, ws] + list(sr.parameters())])
    if mode == "default":  # the ToRGB layers rode on conv1 in both blocks, under autograd
        assert seen == [True, True, True, True]
    else:  # mma_f16 keeps ToRGB off conv1: the stand-alone layer and its own backward
        assert not seen
    assert all(torch.isfinite(a).all() for a in grads[0])
    assert all(torch.equal(a, b) for a, b in zip(*grads))


def test_superres_gradients_vs_reference(P):
    g = T.load_golden("sr_grad.npz")
    sr = _sr(P)
    sr.record_grad = True
    rgb, x, ws, g_out = _leaves()
    assert abs(SRC.draws()[4] - float(g["draw_checksum"][0])) < 1e-6 * abs(float(g["draw_checksum"][0]))
    out = sr(rgb, x, ws, noise_mode="const")
    assert SRC.rel_l2(out.detach()[:, :, ::8, ::8].cpu().numpy(), g["out_sub"]) < 1e-5
    (out * g_out).sum().backward()
    SRC.check_against_fixture(sr, rgb, x, ws, g)


def _sr64(p, rgb, x, ws, filt, clamp, conv_branches=None, rgb_pre=None, keep=None):
    """The super-resolution restated in plain torch (superresolution.py:282-293 on networks_stylegan2.py's blocks), constant noise;
    conv_branches / rgb_pre: the HIP forward's layer outputs and ToRGB pre-clamp sums, whose branch decisions both sides differentiate."""
    import synthesis_restatement as S
    nb = (lambda: next(conv_branches)) if conv_branches is not None else (lambda: None)
    nr = (lambda: next(rgb_pre)) if rgb_pre is not None else (lambda: None)
    w = ws[:, -1]
    img = rgb
    for b in ("block0", "block1"):
        x = S._layer(p, b + ".conv0", x, w, 2, filt, clamp, keep, nb())
        x = S._layer(p, b + ".conv1", x, w, 1, filt, clamp, keep, nb())
        W = p[b + ".torgb.weight"]
        s = S._affine(p, b + ".torgb", w) * (1.0 / np.sqrt(W.shape[1]))
        v = F.conv2d(x * s[:, :, None, None], W) + p[b + ".torgb.bias"][None, :, None, None]
        pre = nr()
        if pre is None:
            v = v.clamp(-clamp, clamp)
        else:
            v = torch.where(pre.abs() < clamp, v, v.detach().clamp(-clamp, clamp))
        img = S._upfirdn_up2(img, filt) + v
    return img


def test_fullsize_superres_gradients_vs_float64(P, monkeypatch):
    """128^2 -> 512^2, 256 hidden channels, batch 1, default operands, clamp 256 live: every gradient within relative L2 1e-4 of torch
    autograd of the float64 restatement, which takes each lrelu slope and clamp from the HIP forward (how many branches the float64
    forward takes differently is asserted separately).  A noise strength's gradient (one sum of terms of both signs) is gated against
    the magnitude of those terms, as in the backbone's full-size test."""
    sr = _sr(P)
    sr.record_grad = True
    rgb, x, ws, g_out = _leaves()
    ys, pres = [], []
    mc, tc = P.ops.modulated_conv2d, P.ops.torgb_combine

    def rec_conv(*a, **k):
        out = mc(*a, **k)
        ys.append((out[0] if isinstance(out, tuple) else out).detach().cpu())
        return out

    def rec_combine(part, **k):
        with torch.no_grad():
            pres.append(tc(part, bias=k.get("bias").detach()).cpu())
        return tc(part, **k)
    monkeypatch.setattr(P.ops, "modulated_conv2d", rec_conv)
    monkeypatch.setattr(P.ops, "torgb_combine", rec_combine)
    out = sr(rgb, x, ws, noise_mode="const")
    monkeypatch.setattr(P.ops, "modulated_conv2d", mc)
    monkeypatch.setattr(P.ops, "torgb_combine", tc)
    assert len(ys) == 4 and len(pres) == 2
    (out * g_out).sum().backward()
    pd = {n: t.detach().cpu().double().requires_grad_(t.dtype.is_floating_point) for n, t in list(sr.named_parameters()) + list(sr.named_buffers())}
    in64 = [t.detach().cpu().double().requires_grad_(True) for t in (rgb, x, ws)]
    filt = sr.block0.resample_filter.cpu()
    with torch.no_grad():  # the float64 forward's own branches: how many differ from the HIP forward's
        ys64 = []
        import synthesis_restatement as S
        xx, w = in64[1].detach(), in64[2].detach()[:, -1]
        flips, total = 0, 0
        for b, k in (("block0", 0), ("block1", 2)):
            xx = S._layer({n: t.detach() for n, t in pd.items()}, b + ".conv0", xx, w, 2, filt, 256.0, None, ys[k])
            flips += int(((xx > 0) != (ys[k] > 0)).sum())
            xx = S._layer({n: t.detach() for n, t in pd.items()}, b + ".conv1", xx, w, 1, filt, 256.0, None, ys[k + 1])
            flips += int(((xx > 0) != (ys[k + 1] > 0)).sum())
            total += ys[k].numel() + ys[k + 1].numel()
    assert flips <= 1e-5 * total, (flips, total)
    keep = {}
    ref = _sr64(pd, in64[0], in64[1], in64[2], filt, 256.0, iter(ys), iter(pres), keep)
    assert SRC.rel_l2(out.detach().cpu().numpy(), ref.detach().numpy()) < 1e-5
    (ref * g_out.cpu().double()).sum().backward()
    bad = []
    for name, ours, r in [("rgb", rgb.grad, in64[0].grad), ("x", x.grad, in64[1].grad), ("ws", ws.grad, in64[2].grad)] + \
            [(n, p.grad, pd[n].grad) for n, p in sr.named_parameters()]:
        a, b = ours.detach().cpu().double(), r.detach()
        if name.endswith("noise_strength"):
            layer = name[:-len(".noise_strength")]
            scale = float((keep[layer].grad * pd[layer + ".noise_const"].detach()).abs().sum())
            e = abs(float(a) - float(b)) / max(scale, 1e-30)
        else:
            e = SRC.rel_l2(a.numpy(), b.numpy())
        print(f"{name}: {e:.2e}")
        if not e <= 1e-4:
            bad.append((name, e))
    assert not bad, bad


# ---- the generator ----------------------------------------------------------------------------------------------------------------
def _gen(P, switch):
    import p3d_shared_cases as MC
    G = MC.memo_generator("cuda")
    T.fill_generator_params(G, 3)
    G.set_view_replay(False)
    if switch is not None:
        G.set_superresolution_grad(switch)
    gen = torch.Generator().manual_seed(11)
    cond = {"image_ortho_front": torch.rand(1, 3, 32, 32, generator=gen).cuda(), "resnet_feats": torch.randn(1, 16, generator=gen).cuda()}
    z = torch.randn(1, G.backbone.z_dim, generator=gen).cuda()
    with torch.no_grad():
        ws0 = G.mapping(z, torch.zeros(1, G.backbone.c_dim, device="cuda"), cond)
    x = lambda ws, res=16, **o: dict(ws=ws, cond=cond, elevations=torch.zeros(1, device="cuda"), azimuths=torch.zeros(1, device="cuda"),
                                     neural_rendering_resolution=res, noise_mode="const", triplane_crop=0.1, cull_clouds=0.5, **o)
    return G, ws0, x


def test_generator_f_image_gradient_end_to_end(P):
    """G.f with the switch on and ws requiring grad, a loss on `image`: the image carries a grad_fn, ws.grad is the planes' share
    (autograd.grad(planes, ws, g_planes)) plus the super-resolution's own use of ws, the decoder, super-resolution and backbone get
    finite non-zero gradients, and a second forward + backward gives the same super-resolution and decoder bits."""
    G, ws0, x = _gen(P, True)
    g_img = torch.randn(1, 3, 512, 512, generator=torch.Generator().manual_seed(5)).cuda()
    def call():
        G.zero_grad(set_to_none=True)
        ws = ws0.clone().requires_grad_(True)
        torch.manual_seed(21)
        out = G.f(x(ws, res=128))  # (128^2: the super-resolution's input as rendered — torch's interpolate backward is not bitwise reproducible)
        assert out["image"].grad_fn is not None
        return ws, out["triplane"], (out["image"] * g_img).sum()
    ws, planes, loss = call()
    g_planes, = torch.autograd.grad(loss, planes, retain_graph=True)
    via_planes, = torch.autograd.grad(planes, ws, g_planes, retain_graph=True)
    h = planes.register_hook(lambda g: torch.zeros_like(g))
    direct, = torch.autograd.grad(loss, ws, retain_graph=True)  # the super-resolution's own use of ws
    h.remove()
    assert torch.count_nonzero(via_planes) > 0 and torch.count_nonzero(direct) > 0
    loss.backward()
    assert SRC.rel_l2(ws.grad.cpu().numpy(), (via_planes + direct).cpu().numpy()) < 1e-6
    for name, mod in (("decoder", G.decoder), ("superresolution", G.superresolution), ("backbone", G.backbone.synthesis)):
        gs = [p.grad for p in mod.parameters() if p.grad is not None]
        assert gs and all(torch.isfinite(g).all() for g in gs) and any(torch.count_nonzero(g) > 0 for g in gs), name
    runs = []
    for _ in range(2):  # the same call twice: forward + one backward each
        ws, planes, loss = call()
        loss.backward()
        runs.append({"ws": ws.grad.clone(), **{n: p.grad.clone() for n, p in G.named_parameters() if p.grad is not None}})
    # the super-resolution's and the decoder's gradients are bitwise reproducible; the renderer accumulates plane gradients with float
    # atomics (include/p3d_render_grad.h), so what lies behind the planes — the backbone, ws — agrees to fp32 rounding
    # (1e-4: a noise strength's gradient is one sum of terms of both signs, which magnifies the atomics' rounding)
    assert runs[0].keys() == runs[1].keys()
    exact = [n for n in runs[0] if n.startswith(("superresolution.", "decoder."))]
    assert any(n.startswith("superresolution.") for n in exact) and any(n.startswith("decoder.") for n in exact)
    for n in exact:
        assert torch.equal(runs[0][n], runs[1][n]), n
    for n in runs[0]:
        assert SRC.rel_l2(runs[0][n].cpu().numpy(), runs[1][n].cpu().numpy()) < 1e-4, n


def test_paste_under_autograd_raises(P):
    G, ws0, x = _gen(P, True)
    with pytest.raises(NotImplementedError):
        G.f(x(ws0.clone().requires_grad_(True), paste_params={}))


def test_switch_off_image_stays_inference_only(P):
    """The default (passes before and after the switch exists): under grad, `image` has no grad_fn."""
    G, ws0, x = _gen(P, None)
    out = G.f(x(ws0.clone().requires_grad_(True)))
    assert out["triplane"].grad_fn is not None and out["image"].grad_fn is None
    if hasattr(G, "set_superresolution_grad"):
        G.set_superresolution_grad(False)
        assert G.f(x(ws0.clone().requires_grad_(True)))["image"].grad_fn is None


def test_replayed_views_around_superres_backward_give_cold_bits(P):
    """Replayed no-grad views, grad-mode views with the switch on and a backward through the super-resolution, replayed views again:
    every call bit-identical to a cold twin (test_hip_view_replay.Pair), and replays happen."""
    import test_hip_view_replay as VR
    pair = VR.Pair()
    pair.both("set_superresolution_grad", True)
    A = VR._subject(1)
    for _ in range(3):
        pair.view(A)
    assert pair.total > 0
    before = pair.total
    for i in range(2):
        assert pair.view(A, grad=True) == 0  # (no replay under autograd)
        torch.manual_seed(77 + i)
        out = pair.G.f(VR._x(A))
        assert out["image"].grad_fn is not None
        (out["image"].square().mean() + out["image_raw"].sum()).backward()
        assert any(p.grad is not None and torch.count_nonzero(p.grad) > 0 for p in pair.G.superresolution.parameters())
        pair.G.zero_grad(set_to_none=True)
        for _ in range(2):
            pair.view(A)
    assert pair.total > before
