"""GPU (-m gpu): the HIP backward of the synthesis network (include/p3d_synthesis_grad.h).

Per layer against a float64 restatement of the same formulas (tests/p3d_torch_ops.py's, in float64 on a CPU copy of the inputs; the
bias_act mask decisions are taken from the kernel's own fp32 output so that both sides differentiate the same branch); the whole
network against the reference's fp32 autograd (tests/golden/syn_grad_*.npz); the grad-mode forward against the no-grad call's bits;
run-to-run reproducibility; caches across grad / no-grad calls; G.f with a given ws."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import p3d_testing as T
import synthesis_grad_cases as SC
import synthesis_grad_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
SQRT2 = float(np.sqrt(2))


@pytest.fixture(scope="module")
def P():
    import panic3d_amd
    panic3d_amd.build()
    panic3d_amd._lib.lib()
    return panic3d_amd


_fir64 = R.fir_ref
_act_masked = R.act_masked  # clamp(lrelu(z) * gain) on the branch decisions (slope, clamp) of the kernel's output


def _modconv64(x, w, s, d, b, noise, up, f, y_ours, clamp):
    xm = x * s[:, :, None, None]
    if up == 1:
        y = F.conv2d(xm, w, padding=1)
    else:
        y = F.conv_transpose2d(xm, w.transpose(0, 1), stride=2)
        k = _fir64(f)[None, None].repeat(y.shape[1], 1, 1, 1)
        y = F.conv2d(F.pad(y, [1, 1, 1, 1]), k, groups=y.shape[1])
    z = y * d[:, :, None, None] + noise + b[None, :, None, None]
    return _act_masked(z, y_ours, 0.2, SQRT2, clamp)


LAYER_CASES = [  # (kind, N, I, O, input res, noise kind, clamp)
    ("plain", 1, 512, 512, 4, "const", None),
    ("plain", 2, 512, 512, 8, "random", 0.5),
    ("plain", 1, 512, 512, 32, "const", 0.5),
    ("plain", 2, 256, 256, 64, "random", None),
    ("plain", 1, 128, 128, 256, "const", 0.5),
    ("up", 1, 512, 512, 4, "const", 0.5),
    ("up", 2, 512, 512, 16, "random", None),
    ("up", 1, 512, 256, 32, "const", 0.5),
    ("up", 1, 256, 128, 128, "random", 0.5),
]


# the default two-term operands on every case, fp32 operands (mma_f16 = False) on two
RUNS = [(c, "x2") for c in LAYER_CASES] + [(c, "f32") for c in LAYER_CASES if c[4] in (8, 32)]


@pytest.mark.parametrize("case,mma", RUNS, ids=lambda c: "-".join(map(str, c)) if isinstance(c, tuple) else c)
def test_modconv_layer_gradients_vs_float64(P, case, mma):
    kind, N, I, O, res, nk, clamp = case
    up = 2 if kind == "up" else 1
    gen = torch.Generator().manual_seed(N * 1000 + I + O + res + (7 if up == 2 else 0))
    Ho = res * up
    x = torch.randn(N, I, res, res, generator=gen)
    w = torch.randn(O, I, 3, 3, generator=gen)
    s = torch.randn(N, I, generator=gen) * 0.5 + 1.0
    d = ((w.square().sum(dim=(2, 3))[None] * s.square()[:, None, :]).sum(dim=2) + 1e-8).rsqrt()
    b = torch.randn(O, generator=gen) * 0.2
    raw = torch.randn((Ho, Ho) if nk == "const" else (N, 1, Ho, Ho), generator=gen)
    st = torch.tensor(0.3)
    f = P.ops.setup_filter([1, 3, 3, 1])
    gy = torch.randn(N, O, Ho, Ho, generator=gen)
    leaves = [t.to(DEV).requires_grad_(True) for t in (x, w, s, d, b, st)]
    xg, wg, sg_, dg, bg, stg = leaves
    wf = P.ops.conv_weights_to_f16(wg.detach(), split=True, layout=P.ops.conv_weight_layout(I, O, res, up)) if mma == "x2" and I % 16 == 0 else None
    y = P.ops.modulated_conv2d(xg, wg, sg_, noise=raw.to(DEV) * stg, up=up, padding=1, resample_filter=f.to(DEV), demodulate=True,
                               bias=bg, act="lrelu", gain=SQRT2, clamp=clamp, weight_f16=wf, dcoef=dg)
    assert y.grad_fn is not None
    (y * gy.to(DEV)).sum().backward()
    ref = [t.double().requires_grad_(True) for t in (x, w, s, d, b, st)]
    y64 = _modconv64(ref[0], ref[1], ref[2], ref[3], ref[4], raw.double() * ref[5], up, f, y.detach().cpu().double(), clamp)
    assert SC.rel_l2(y.detach().cpu().numpy(), y64.detach().numpy()) < 1e-5
    (y64 * gy.double()).sum().backward()
    for name, a, r in zip(("x", "weight", "styles", "dcoef", "bias", "noise_strength"), leaves, ref):
        e = SC.rel_l2(a.grad.cpu().numpy(), r.grad.numpy())
        assert e <= 1e-5, (name, e)


@pytest.mark.parametrize("N,I,res,skip,clamp", [(1, 512, 4, False, None), (2, 256, 64, True, 0.5), (1, 128, 256, True, 0.5),
                                                (2, 64, 32, True, None)])
def test_torgb_gradients_vs_float64(P, N, I, res, skip, clamp):
    O = 96
    gen = torch.Generator().manual_seed(res * 7 + I)
    x = torch.randn(N, I, res, res, generator=gen)
    w = torch.randn(O, I, 1, 1, generator=gen)
    s = torch.randn(N, I, generator=gen) / np.sqrt(I)
    b = torch.randn(O, generator=gen) * 0.2
    sk = torch.randn(N, O, res // 2, res // 2, generator=gen) if skip else None
    f = P.ops.setup_filter([1, 3, 3, 1])
    gi = torch.randn(N, O, res, res, generator=gen)
    leaves = [t.to(DEV).requires_grad_(True) for t in (x, w, s, b)] + ([sk.to(DEV).requires_grad_(True)] if skip else [])
    img = P.ops.torgb(leaves[0], P.ops.torgb_weights(leaves[1]), O, leaves[2], bias=leaves[3], clamp=clamp,
                      skip=leaves[4] if skip else None, skip_filter=f.to(DEV))
    (img * gi.to(DEV)).sum().backward()
    with torch.no_grad():
        ylin = P.ops.torgb(leaves[0], P.ops.torgb_weights(leaves[1]), O, leaves[2], bias=leaves[3]).cpu().double()
    ref = [t.double().requires_grad_(True) for t in ((x, w, s, b) + ((sk,) if skip else ()))]
    z = F.conv2d(ref[0] * ref[2][:, :, None, None], ref[1]) + ref[3][None, :, None, None]
    if clamp is not None:
        z = torch.where(ylin.abs() < clamp, z, z.detach())
    if skip:
        up = torch.zeros(N, O, res, res, dtype=torch.float64)
        up[:, :, ::2, ::2] = ref[4]
        k = _fir64(f)[None, None].repeat(O, 1, 1, 1)
        z = z + F.conv2d(F.pad(up, [2, 1, 2, 1]), k, groups=O)
    (z * gi.double()).sum().backward()
    for name, a, r in zip(("x", "weight", "styles", "bias", "skip"), leaves, ref):
        e = SC.rel_l2(a.grad.cpu().numpy(), r.grad.numpy())
        assert e <= 1e-5, (name, e)


def test_synthesis_planes_carry_grad_and_reach_ws(P):
    """The test that fails without the backward: planes = net(ws.requires_grad_(), cond) has a grad_fn and ws.grad is filled."""
    G, net, ws, cond, inj, g_out, sl, g = SC.build(P, "none", DEV)
    planes = net(ws, cond, noise_mode="const")
    assert planes.grad_fn is not None
    (planes * g_out).sum().backward()
    assert ws.grad is not None and torch.isfinite(ws.grad).all() and torch.count_nonzero(ws.grad) > 0


@pytest.mark.parametrize("tag", ["none", "cond"])
def test_synthesis_gradients_vs_reference(P, tag):
    G, net, ws, cond, inj, g_out, sl, g = SC.build(P, tag, DEV)
    out = net(ws, cond, latent_injection=inj, stop_level=sl, noise_mode="const")
    (out * g_out).sum().backward()
    SC.check_against_fixture(net, ws, cond, inj, g)


@pytest.mark.parametrize("mma", [None, "f32"])
@pytest.mark.parametrize("tag", ["none", "cond"])
def test_grad_mode_planes_equal_no_grad_planes_and_grads_reproduce(P, monkeypatch, tag, mma):
    if mma is not None:
        monkeypatch.setattr(P.stylegan2, "DEFAULT_CONV_MMA", mma)
    G, net, ws, cond, inj, g_out, sl, g = SC.build(P, tag, DEV)
    with torch.no_grad():
        ref = net(ws.detach(), cond, noise_mode="const").clone()
    grads = []
    for _ in range(2):
        for t in [ws] + list(net.parameters()) + [cond[k] for k in SC.COND_GRAD]:
            t.grad = None
        out = net(ws, cond, noise_mode="const")
        assert torch.equal(out.detach(), ref)
        (out * g_out).sum().backward()
        grads.append([t.grad.clone() for t in [ws] + list(net.parameters()) + [cond[k] for k in SC.COND_GRAD] if t.grad is not None])
    assert len(grads[0]) == len(grads[1]) and all(torch.equal(a, b) for a, b in zip(*grads))


def test_random_noise_grad_mode_matches_no_grad(P):
    """Pooled random noise under autograd: the same draw values (same seed) and a noise-strength gradient."""
    G, net, ws, cond, inj, g_out, sl, g = SC.build(P, "none", DEV)
    torch.manual_seed(5)
    with torch.no_grad():
        ref = net(ws.detach(), cond, noise_mode="random").clone()
    torch.manual_seed(5)
    out = net(ws, cond, noise_mode="random")
    assert torch.equal(out.detach(), ref)
    (out * g_out).sum().backward()
    ns = net.b8.conv1.noise_strength.grad
    assert ns is not None and torch.isfinite(ns) and ns != 0


def test_alternating_grad_and_no_grad_calls_give_cold_bits(P):
    G, net, ws, cond, inj, g_out, sl, g = SC.build(P, "cond", DEV)
    cold_G, cold_net, cws, ccond, *_ = SC.build(P, "cond", DEV)
    with torch.no_grad():
        cold = cold_net(cws.detach(), ccond, noise_mode="const").clone()
    for i in range(3):
        with torch.no_grad():
            a = net(ws.detach(), cond, noise_mode="const")
        assert torch.equal(a, cold), i
        out = net(ws, cond, noise_mode="const")
        assert torch.equal(out.detach(), cold), i
        (out * g_out).sum().backward()


def test_generator_f_ws_gradient_through_renderer(P):
    """G.f with ws given: ws.grad equals torch.autograd.grad(planes, ws, g_planes), g_planes the renderer backward's plane gradient."""
    import p3d_shared_cases as MC
    G = MC.memo_generator("cuda")
    T.fill_generator_params(G, 3)
    G.set_view_replay(False)
    gen = torch.Generator().manual_seed(11)
    cond = {"image_ortho_front": torch.rand(1, 3, 32, 32, generator=gen).cuda(), "resnet_feats": torch.randn(1, 16, generator=gen).cuda()}
    z = torch.randn(1, G.backbone.z_dim, generator=gen).cuda()
    c = torch.zeros(1, G.backbone.c_dim, device="cuda")
    with torch.no_grad():
        ws0 = G.mapping(z, c, cond)
    ws = ws0.clone().requires_grad_(True)
    out = G.f(dict(ws=ws, cond=cond, elevations=torch.zeros(1, device="cuda"), azimuths=torch.zeros(1, device="cuda"),
                   neural_rendering_resolution=16, noise_mode="const", triplane_crop=0.1, cull_clouds=0.5))
    planes = out["triplane"]
    assert planes.grad_fn is not None and out["image"].grad_fn is None
    loss = out["image_raw"].sum() + out["image_depth"].sum()
    g_planes, = torch.autograd.grad(loss, planes, retain_graph=True)
    want, = torch.autograd.grad(planes, ws, g_planes, retain_graph=True)
    loss.backward()
    assert torch.isfinite(ws.grad).all() and torch.count_nonzero(ws.grad) > 0
    # (the same backward launches; the cotangents meeting at the planes are summed in another order: fp32 agreement, not bits)
    assert SC.rel_l2(ws.grad.cpu().numpy(), want.cpu().numpy()) < 1e-6


def test_fullsize_conditioned_backbone_gradients_vs_float64(P, monkeypatch):
    """The product configuration end to end: the 256^2 backbone (96 channels, channel max 512, conv_clamp 256), batch 1, conditioned
    ('ortho_front.add_shuffle2_4.inj_6b_4'), default operands, differentiated on the HIP path against torch autograd of the float64
    restatement (tests/synthesis_restatement.py) on a CPU copy: relative L2 <= 1e-4 for ws, the conditioning image and every parameter
    tensor.  A noise strength's gradient is ONE sum over a layer's pixels of terms of both signs; its error is gated against the
    magnitude of those terms (the sum's own conditioning) at the same 1e-4.
    The float64 side differentiates the branches (lrelu slope, clamp) the HIP forward took: over 13 layers and ~30 M activations a
    few dozen pre-activations lie within fp32 rounding of zero, and one flipped slope moves that element's gradient by 80 % — ~1e-3
    of a layer's gradient norm, which no fp32 forward avoids (the reference's own fp32 autograd included).  How many branches the
    two forwards take differently is asserted separately (a handful per million)."""
    import synthesis_restatement as R
    cm = "ortho_front.add_shuffle2_4.inj_6b_4"
    net = P.stylegan2.SynthesisNetwork(w_dim=512, img_resolution=256, img_channels=96, cond_mode=cm, channel_base=32768, channel_max=512,
                                       num_fp16_res=0, conv_clamp=256)
    g = torch.Generator().manual_seed(256)
    with torch.no_grad():
        for n, p in sorted(list(net.named_parameters()) + [(n, b) for n, b in net.named_buffers() if n.endswith("noise_const")]):
            if n.endswith("noise_strength"):
                p.fill_(0.1)
            elif n.endswith("affine.bias"):
                p.fill_(1.0)
            elif n.endswith(".bias"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.2)
            else:
                p.copy_(torch.randn(p.shape, generator=g))
    net = net.to(DEV)
    ws = torch.randn(1, net.num_ws, 512, generator=g)
    front = torch.rand(1, 3, 512, 512, generator=g)
    g_out = torch.randn(1, 96, 256, 256, generator=g)
    wsg = ws.to(DEV).requires_grad_(True)
    cond = {"image_ortho_front": front.to(DEV).requires_grad_(True)}
    ys = []
    mc = P.ops.modulated_conv2d

    def recording(*a, **k):  # every SynthesisLayer's fp32 output, in execution order
        y = mc(*a, **k)
        ys.append(y.detach().cpu())
        return y
    monkeypatch.setattr(P.ops, "modulated_conv2d", recording)
    out = net(wsg, cond, noise_mode="const")
    monkeypatch.setattr(P.ops, "modulated_conv2d", mc)
    assert len(ys) == 13
    (out * g_out.to(DEV)).sum().backward()
    pd = {n: t.detach().cpu().double().requires_grad_(t.dtype.is_floating_point) for n, t in list(net.named_parameters()) + list(net.named_buffers())}
    ws64 = ws.double().requires_grad_(True)
    c64 = {"image_ortho_front": front.double().requires_grad_(True)}
    keep = {}
    with torch.no_grad():  # the float64 forward's own branches: how many differ from the HIP forward's
        ys64 = []
        R.synthesis({n: t.detach() for n, t in pd.items()}, ws64.detach(), {k: v.detach() for k, v in c64.items()}, cm, net.block_resolutions,
                    net.b8.resample_filter.cpu(), 256.0, outputs=ys64)
        flips = sum(int(((a > 0) != (b > 0)).sum()) for a, b in zip(ys, ys64))
        total = sum(a.numel() for a in ys)
    assert len(ys64) == len(ys) and flips <= 1e-5 * total, (flips, total)
    ref = R.synthesis(pd, ws64, c64, cm, net.block_resolutions, net.b8.resample_filter.cpu(), 256.0, keep, branches=iter(ys))
    assert SC.rel_l2(out.detach().cpu().numpy(), ref.detach().numpy()) < 1e-5
    (ref * g_out.double()).sum().backward()
    bad = []
    for name, ours, r in [("ws", wsg.grad, ws64.grad), ("image_ortho_front", cond["image_ortho_front"].grad, c64["image_ortho_front"].grad)] + \
            [(n, p.grad, pd[n].grad) for n, p in net.named_parameters()]:
        a, b = ours.detach().cpu().double(), r.detach()
        if name.endswith("noise_strength"):
            layer = name[:-len(".noise_strength")]
            scale = float((keep[layer].grad * pd[layer + ".noise_const"].detach()).abs().sum())
            e = abs(float(a) - float(b)) / max(scale, 1e-30)
        else:
            e = SC.rel_l2(a.numpy(), b.numpy())
        if not e <= 1e-4:
            bad.append((name, e))
    assert not bad, bad


def test_replayed_views_around_backward_calls_give_cold_bits(P):
    """Check 7 through the generator's launch replay: replayed no-grad views, grad-mode views whose backward runs through the synthesis
    network, and replayed views again — every call bit-identical to a cold twin (test_hip_view_replay.Pair), and replays happen."""
    import test_hip_view_replay as VR
    pair = VR.Pair()
    A = VR._subject(1)
    for _ in range(3):
        pair.view(A)
    assert pair.total > 0
    before = pair.total
    for i in range(2):
        assert pair.view(A, grad=True) == 0  # (no replay under autograd)
        torch.manual_seed(77 + i)
        out = pair.G.f(VR._x(A))
        assert out["triplane"].grad_fn is not None
        (out["image_raw"].sum() + out["triplane"].square().mean()).backward()
        pair.G.zero_grad(set_to_none=True)
        for _ in range(2):
            pair.view(A)
    assert pair.total > before
