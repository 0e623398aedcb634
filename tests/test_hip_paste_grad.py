"""GPU (-m gpu): the front-view paste's HIP backward (include/p3d_paste_grad.h, csrc/p3d_paste_grad.hip).

Kernel level: p3d_paste_front_backward_f32 with the forward's own mask against the float64 restatement of
torch.lerp(image, sample_orthofront(tocopy, interpolate(xyz, S)), mask) evaluated at the forward's coordinates
(train_step_cases.paste_backward_ref; tests/test_paste_grad_cpu.py shows that it is float64 torch autograd and that the gate catches
a dropped tap, swapped channels and a missing border zero), element-wise within 8 sqrt(K) 2^-24 of the absolute-value sum.
Generator level: the switch, the bits of the outputs, grad_sample reaching the decoder, and the reference's paste_front under
autograd (tests/golden/train_step.npz)."""
import numpy as np
import pytest
import torch

import p3d_testing as T
import train_step_cases as TC

pytestmark = pytest.mark.gpu
BW = 0.7


@pytest.fixture(scope="module")
def P():
    import panic3d_amd
    panic3d_amd.build()
    panic3d_amd._lib.lib()
    return panic3d_amd


def _forward(P, seed, N, r, S, shared, norm, scale):
    """Inputs with some samples clamped at the illustration's border, and the forward kernel's own mask (fractional where the
    occlusion mask is interpolated, 0 and 1 elsewhere)."""
    g = torch.Generator().manual_seed(seed)
    d = lambda t: t.cuda()
    xyz = torch.randn(N, 3, r, r, generator=g) * scale
    front = torch.rand(1 if shared else N, 3, S, S, generator=g)
    weights, occ = torch.rand(N, 1, r, r, generator=g), torch.rand(N, 1, r, r, generator=g)
    ro, rd = torch.randn(N, 3, r, r, generator=g), torch.nn.functional.normalize(torch.randn(N, 3, r, r, generator=g), dim=1)
    image = torch.randn(N, 3, S, S, generator=g)
    res = P.ops.paste_front(d(weights), d(xyz), d(occ), d(ro), d(rd), d(front), d(image), 0.4, 1e3, 0.5, 1e3, BW, norm)
    g_out, g_paste = torch.randn(N, 3, S, S, generator=g), torch.randn(N, 3, S, S, generator=g)
    return xyz, front, res["mask"], g_out, g_paste


CASES = [(16, 64, 1, False, False, True), (32, 96, 2, False, True, True), (37, 96, 3, True, True, True), (37, 64, 2, True, False, True),
         (32, 512, 2, False, True, True), (16, 512, 3, True, False, True), (16, 512, 1, False, False, False), (37, 96, 2, False, True, False)]


@pytest.mark.parametrize("r,S,N,shared,norm,gs", CASES)
@pytest.mark.parametrize("cot", ["both", "image_only", "paste_only"])
def test_paste_backward_kernel_vs_float64(P, r, S, N, shared, norm, gs, cot):
    xyz, front, mask, g_out, g_paste = _forward(P, 1000 * r + S + N, N, r, S, shared, norm, 0.25)
    m = mask.cpu()
    assert 0.02 < float(m.mean()) < 0.98 and float(((m > 0) & (m < 1)).float().mean()) > 0.01
    go = None if cot == "paste_only" else g_out
    gp = None if cot == "image_only" else g_paste
    if not gs and go is None:
        go = g_out  # without grad_sample the paste's cotangent reaches nothing: a call needs the image's
    d = lambda t: None if t is None else t.cuda()
    gi, gx, gf = P.ops.paste_front_backward(d(go), d(gp), mask, d(xyz), d(front), BW, norm, gs, want_image=True, want_xyz=gs, want_front=gs)
    ref = TC.paste_backward_ref(go, gp, m, xyz, front, BW, norm, gs)
    if not gs:
        assert gx is None and gf is None and "g_xyz" not in ref
    else:
        assert torch.count_nonzero(gx[:, 2]) == 0 and torch.count_nonzero(gx[:, :2]) > 0
        clamped = float((ref["g_xyz"][1][:, :2] == 0).double().mean())
        print(f"texels whose every sample is clamped or unmasked: {clamped:.2%}")
    worst = {}
    for name, ours in (("g_image", gi), ("g_xyz", gx), ("g_front", gf)):
        if ours is None:
            continue
        worst[name] = TC.gate_ratio(ours, *ref[name])
        print(f"gate {name}: worst {worst[name]:.3f} of 8 (K = {ref[name][2]}), rel-L2 {TC.rel_l2(ours, ref[name][0]):.2e}")
    assert all(v <= 8.0 for v in worst.values()), worst


def test_paste_backward_is_reproducible(P):
    """g_image and g_xyz bit for bit over two runs (no atomics); g_front to fp32 rounding (float atomics: the order of the additions)."""
    xyz, front, mask, g_out, g_paste = _forward(P, 77, 3, 32, 512, True, True, 0.25)
    run = lambda: P.ops.paste_front_backward(g_out.cuda(), g_paste.cuda(), mask, xyz.cuda(), front.cuda(), BW, True, True, want_xyz=True, want_front=True)
    a, b = run(), run()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    ref = TC.paste_backward_ref(g_out, g_paste, mask.cpu(), xyz, front, BW, True, True)["g_front"]
    assert TC.gate_ratio(a[2], *ref) <= 8.0 and TC.gate_ratio(b[2], *ref) <= 8.0
    assert TC.rel_l2(a[2], b[2]) < 1e-6


def test_paste_backward_wrapper_rejects_mismatched_shapes(P):
    xyz, front, mask, g_out, g_paste = _forward(P, 5, 2, 16, 64, False, False, 0.25)
    c = lambda t: t.cuda()
    with pytest.raises(RuntimeError):
        P.ops.paste_front_backward(c(g_out)[:1], None, mask, c(xyz), c(front), BW, False, True)
    with pytest.raises(RuntimeError):
        P.ops.paste_front_backward(c(g_out), None, mask[..., :32], c(xyz), c(front), BW, False, True)
    with pytest.raises(RuntimeError):
        P.ops.paste_front_backward(None, None, mask, c(xyz), c(front), BW, False, True)
    with pytest.raises(RuntimeError):
        P.ops.paste_front_backward(c(g_out), None, mask, c(xyz), c(front), BW, False, False, want_xyz=True)
    with pytest.raises(RuntimeError):
        P.ops.paste_front_backward(g_out, None, mask, c(xyz), c(front), BW, False, True)  # a CPU tensor


# ---- the generator -------------------------------------------------------------------------------------------------------------------
def _gen(P):
    from panic3d_amd.generator import TriPlaneGenerator
    g = T.load_golden("syn_triplane_f.npz")
    G = TriPlaneGenerator(**TC.TRI_KW)
    G.load_state_dict({k[3:].replace("__", "."): torch.from_numpy(v) for k, v in g.items() if k.startswith("sd_")}, strict=True)
    G = G.cuda().eval()
    G.set_force_sigmoid(True)
    G.set_render_exact(True)  # (as every grad test of the generator: the grad-mode render dumps its sorted depths and runs the exact final pass)
    G.set_view_replay(False)
    return G


def _draws(seed, N, res):
    gen = torch.Generator().manual_seed(seed)
    return [(torch.rand(N, res * res, 12, 1, generator=gen).cuda(), torch.rand(N * res * res, 12, generator=gen).cuda()) for _ in range(2)]


def _x(ws, front, pp, res=16):
    return dict(ws=ws, cond={"image_ortho_front": front}, elevations=torch.zeros(1, device="cuda"), azimuths=torch.full((1,), 10.0, device="cuda"),
                fovs=torch.full((1,), -1.0, device="cuda"), neural_rendering_resolution=res, noise_mode="const", triplane_crop=0.1, cull_clouds=0.5,
                paste_params=pp)


def test_switch_off_refuses_and_on_records_with_the_same_bits(P):
    G = _gen(P)
    pp = {k: v for k, v in TC.PASTE_PARAMS.items() if k != "grad_sample"}
    front = torch.rand(1, 3, 512, 512, generator=torch.Generator().manual_seed(21)).cuda()
    ws0 = torch.from_numpy(T.load_golden("syn_triplane_f.npz")["ws"])[:1].cuda()
    draws = _draws(31, 1, 16)

    def call(ws, grad, pp=pp):
        G._inject_draws = [tuple(d) for d in draws]
        with torch.enable_grad() if grad else torch.no_grad():
            return G.f(_x(ws, front, pp))
    cold = call(ws0, False)
    assert 0.005 < float(cold["paste"]["mask"].mean()) < 0.995
    # off (the default): a recording image is refused; a non-recording one runs under no_grad, today's bits
    G.set_superresolution_grad(True)
    with pytest.raises(NotImplementedError):
        call(ws0.clone().requires_grad_(True), True)
    G.set_superresolution_grad(False)
    quiet = call(ws0.clone().requires_grad_(True), True)
    for k in ("triplane", "image_raw", "image_xyz", "image_weights", "image_prepaste", "image"):
        assert torch.equal(quiet[k].detach(), cold[k]), k
    assert quiet["image"].grad_fn is None
    # on
    G.set_superresolution_grad(True)
    assert G.set_paste_grad(True) is True and G.__dict__["_view_graphs"] is None
    hot = call(ws0.clone().requires_grad_(True), True)
    assert hot["image"].grad_fn is not None
    for k in ("image", "image_prepaste"):
        assert torch.equal(hot[k].detach(), cold[k]), k
    for k in ("mask", "paste", "mask_weights", "mask_edges", "mask_occ", "mask_dxyz"):
        assert torch.equal(hot["paste"][k].detach(), cold["paste"][k]), k
    assert hot["paste"]["mask"].grad_fn is None and hot["paste"]["paste"].grad_fn is None  # grad_sample off: the paste is a constant
    no_grad_again = call(ws0, False)
    assert torch.equal(no_grad_again["image"], cold["image"]) and no_grad_again["image"].grad_fn is None
    # grad_sample: a loss on `image` alone reaches the decoder through image_xyz only with it
    G.set_superresolution_grad(False)  # the image then depends on the generator through the paste's sampling alone
    grads = {}
    for gs in (False, True):
        G.zero_grad(set_to_none=True)
        out = call(ws0.clone().requires_grad_(True), True, dict(pp, grad_sample=gs))
        if out["image"].grad_fn is not None:
            out["image"].square().sum().backward()
        grads[gs] = [p.grad for p in G.decoder.parameters()]
    assert all(g is None for g in grads[False])
    assert all(g is not None and torch.isfinite(g).all() for g in grads[True]) and any(torch.count_nonzero(g) > 0 for g in grads[True])
    G._inject_draws = None


def test_paste_grad_vs_reference_train_step(P):
    """The reference's image_prepaste / image_xyz / image_weights go into this package's paste (fused kernel, its own occlusion render
    on its own planes with the reference's draws): only the paste is under test."""
    from panic3d_amd import paste
    g = T.load_golden("train_step.npz")
    tt = lambda k: torch.from_numpy(g[k]).cuda()
    G = _gen(P)
    G.set_paste_grad(True)
    x = TC.paste_x("cuda")
    x.update(force_rays={"ray_origins": tt("ray_origins"), "ray_directions": tt("ray_directions")}, normalize_images=False)
    with torch.no_grad():
        planes = G._planes(tt("ws"), x["cond"], noise_mode="const")
    out = {"image": TC.prepaste_from_sub4(g["image_sub4"]).cuda().requires_grad_(True), "image_xyz": tt("image_xyz").requires_grad_(True),
           "image_weights": tt("image_weights").requires_grad_(True), "triplane": planes}
    G._inject_draws = [(tt("draw2"), tt("draw3"))]  # the occlusion pass consumes the reference's draws
    res = paste.paste_front(G, x, out, **TC.PASTE_PARAMS)
    assert G._inject_draws == [] and res["image"].grad_fn is not None and res["paste"].grad_fn is not None
    G._inject_draws = None
    assert float((res["paste"].detach()[..., ::4, ::4].cpu() - torch.from_numpy(g["paste_sub4"])).abs().mean()) < 2e-3
    TC.paste_loss(res["image"], out["image_weights"], out["image_xyz"]).backward()
    assert TC.rel_l2(out["image_weights"].grad, g["g_weights"]) <= 1e-6
    TC.check_paste_against_fixture(g, res["mask"], out["image"].grad, out["image_xyz"].grad)
