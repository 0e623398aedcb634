"""GPU: the training loss's kernels (csrc/p3d_loss.hip) against the float64 restatements of tests/loss_cases.py under the project's gates,
run-to-run bits and grad-mode against no_grad bits; the loss on the device against the reference's own run
(tests/golden/loss_phases.npz); and one real step per phase family through TriPlaneGenerator.f and DualDiscriminator.  On the parent
commit the module, the operators and the symbols do not exist."""
import pytest
import torch

import loss_cases as LC
import p3d_testing as T

pytestmark = pytest.mark.gpu
F = torch.nn.functional


@pytest.fixture(scope="module")
def P():
    import panic3d_amd
    panic3d_amd.build()
    panic3d_amd._lib.lib()
    return panic3d_amd


# ---- the blur ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("taps", LC.BLUR_TAPS)
def test_blur_and_its_adjoint(P, taps):
    """Every shape of the list at NC 1 and 7 (widths 7, 31, 65 and 70: no multiple of 4 but none needed; one pixel more than the tile in
    each direction; images smaller than the filter's half width), an asymmetric filter with mixed signs."""
    tile = P.ops.BLUR_TILE if taps <= 69 else (16, P.ops.BLUR_TILE[1])  # the tile is 16 rows high above 69 taps
    f = LC.blur_filter(taps)
    fd = f.cuda()
    for H, W in LC.blur_shapes(P.ops.BLUR_TILE) + ([(tile[0] + 1, tile[1] + 1)] if tile != P.ops.BLUR_TILE else []):
        for NC in (1, 7):
            x, g = LC.blur_input(NC, H, W)
            xd = x.cuda().requires_grad_(True)
            y = P.ops.blur_fir(xd, fd)
            y.backward(g.cuda())
            with torch.no_grad():
                y0 = P.ops.blur_fir(xd.detach(), fd)
                y1 = P.ops.blur_fir(xd.detach(), fd)
            assert torch.equal(y.detach(), y0) and torch.equal(y0, y1), "grad mode / no_grad / run-to-run bits"
            bad = LC.gate(f"blur {taps} {NC}x{H}x{W}", y0.cpu(), LC.blur_f64(x, f), LC.blur_absref(x, f), 2 * taps)
            bad += LC.gate(f"adjoint {taps} {NC}x{H}x{W}", xd.grad.cpu(), LC.blur_adjoint_f64(g, f), LC.blur_absref(g, f.flip(0)), 2 * taps)
            assert bad == [], bad


def test_blur_of_the_loss_and_batched_planes(P):
    """ops.blur at the trainer's sigma on a [N,C,H,W] tensor: the planes are N*C; against the reference's own convolution pair."""
    x = torch.randn(2, 3, 40, 72, generator=torch.Generator().manual_seed(3))
    f = P.ops.gaussian_filter(10)
    y = P.ops.blur(x.cuda(), 10)
    assert tuple(y.shape) == tuple(x.shape) and P.ops.blur(x.cuda(), 0.2).data_ptr() != y.data_ptr()
    assert LC.gate("blur sigma 10", y.cpu(), LC.blur_f64(x, f), LC.blur_absref(x, f), 2 * 61) == []
    assert LC.rel_l2(y.cpu(), LC.blur_torch(x, f)) < 1e-6
    # differentiable twice: the gradient of <blur(x), g> with respect to g through the recorded backward
    xd, gd = x.cuda().requires_grad_(True), torch.randn(x.shape, generator=torch.Generator().manual_seed(4)).cuda().requires_grad_(True)
    gx, = torch.autograd.grad(P.ops.blur(xd, 1.5), xd, gd, create_graph=True)
    ggy, = torch.autograd.grad(gx, gd, xd.detach())
    assert torch.equal(ggy, P.ops.blur(xd.detach(), 1.5))  # the filter is symmetric: A^T^T x = A x, same launches


# ---- L1 and the view terms --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 1025, 3 * 40 * 41, 1024 * 1024 + 3])
def test_l1(P, n):
    g = torch.Generator().manual_seed(n)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    a[n // 2] = b[n // 2]
    ref = LC.l1_f64(a, b, 1.0 / n)
    ad = a.cuda().requires_grad_(True)
    y = P.ops.l1_mean(ad, b.cuda())
    (y * 1.0).backward()
    with torch.no_grad():
        y0, y1 = P.ops.l1_mean(ad.detach(), b.cuda()), P.ops.l1_mean(ad.detach(), b.cuda())
    assert torch.equal(y.detach(), y0) and torch.equal(y0, y1)
    err, allow = abs(float(y0) * n - float(ref["sum"])), LC.GATE_C * (LC.L1_K + n / (1024 * 256)) ** 0.5 * LC.EPS32 * float(ref["absref"])
    print(f"l1 n={n}: |diff| {err:.3e} allowed {allow:.3e}")
    assert err <= allow
    assert torch.equal(ad.grad.cpu().double(), ref["g_a"]) and ad.grad[n // 2] == 0


@pytest.mark.parametrize("S,r", LC.VT_SHAPES)
@pytest.mark.parametrize("mode", ["z", "x", "norm"])
def test_view_terms(P, S, r, mode):
    for with_q in (False, True):
        c = LC.view_terms_case(S, r, with_q)
        d = {k: (v.cuda() if v is not None else None) for k, v in c.items()}
        count = c["weights"].numel()
        ref = LC.view_terms_f64(c["weights"], c["xyz"], c["gt_alpha"], c["gt_xyz"], mode, c["q"], 1 / count, 1 / count)
        assert float(ref["tight_z"].double().mean()) <= LC.VT_MAX_TIGHT
        sums, gw, gx = P.ops._view_terms_impl(d["weights"], d["xyz"], d["gt_alpha"], d["gt_xyz"], mode, d["q"], True)
        sums2, gw2, gx2 = P.ops._view_terms_impl(d["weights"], d["xyz"], d["gt_alpha"], d["gt_xyz"], mode, d["q"], True)
        plain = P.ops.view_terms(d["weights"], d["xyz"], d["gt_alpha"], d["gt_xyz"], mode, d["q"])
        assert torch.equal(sums, sums2) and torch.equal(gw, gw2) and torch.equal(gx, gx2) and torch.equal(sums, plain)
        assert torch.isfinite(gx).all()
        bad = LC.view_terms_gate(dict(sums=sums.cpu().double() * count, g_w=gw.cpu(), g_x=gx.cpu()), ref, mode)
        assert bad == [], (S, r, mode, with_q, bad)
        w, x = d["weights"].clone().requires_grad_(True), d["xyz"].clone().requires_grad_(True)
        t = P.ops.view_terms(w, x, d["gt_alpha"], d["gt_xyz"], mode, d["q"])
        assert torch.equal(t.detach(), sums)
        (3 * t[0] + 0.5 * t[1]).backward()
        assert torch.equal(w.grad, gw * 3) and torch.equal(x.grad, gx * 0.5)


def test_view_terms_zero_distance_has_zero_gradient(P):
    c = LC.view_terms_case(9, 9, False)  # S == r: the resize is the identity, the distance at xyz == gt_xyz exactly 0
    d = {k: (v.cuda() if v is not None else None) for k, v in c.items()}
    d["xyz"] = d["gt_xyz"].clone()
    d["weights"] = torch.ones_like(d["weights"])
    sums, gw, gx = P.ops._view_terms_impl(d["weights"], d["xyz"], d["gt_alpha"], d["gt_xyz"], "norm", None, True)
    assert float(sums[1]) == 0 and torch.count_nonzero(gx) == 0 and torch.isfinite(gx).all()


# ---- the loss on the device against the reference ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(LC.PHASE_CASES))
def test_phase_against_reference(P, monkeypatch, name):
    golden = T.load_golden("loss_phases.npz")
    case = LC.PHASE_CASES[name]
    LC.draws_on_cpu(monkeypatch)
    reports, grads = LC.run_phase(P.StyleGAN2LossOrthoCondA, case, lambda hook: monkeypatch.setattr(P.loss, "report", hook), device="cuda")
    LC.compare_with_fixture(golden, name, reports, grads)


# ---- one real step per phase family -----------------------------------------------------------------------------------------------------
class _SmallG:
    """The generator of the existing Gmain-shaped test (tests/test_hip_discriminator.py) behind the calls the loss makes.  Its backbone
    is 32^2, so it takes a 32^2 illustration where the trainer's 256^2 backbone takes the 512^2 one: the conditioning dictionary is
    handed on with the illustration resized, and with the small render's options."""

    def __init__(self, G):
        self.G, self.rendering_kwargs, self.cond_mode, self.outs = G, G.rendering_kwargs, G.cond_mode, []

    def _cond(self, cond):
        small = getattr(self, "_small", None)
        if small is None or small[0] is not cond:
            self._small = small = (cond, dict(cond, image_ortho_front=F.interpolate(cond["image_ortho_front"], 32, mode="bilinear", antialias=True)))
        return small[1]

    def mapping(self, z, c, cond, **kw):
        return self.G.mapping(z, c, self._cond(cond), **kw)

    def sample_mixed(self, coordinates, directions, ws, cond, **kw):
        return self.G.sample_mixed(coordinates, directions, ws, self._cond(cond), **kw)

    def f(self, x):
        x = dict(x, cond=self._cond(x["cond"]), noise_mode="const", triplane_crop=0.1, cull_clouds=0.5)
        x.setdefault("neural_rendering_resolution", 16)
        out = self.G.f(x)
        self.outs.append(dict(out))  # (a copy: run_D replaces the image in the dictionary it is given)
        return out


@pytest.fixture(scope="module")
def real_step(P):
    import discriminator_cases as DC
    import p3d_shared_cases as MC
    G = MC.memo_generator("cuda")
    T.fill_generator_params(G, 3)
    G.set_view_replay(False)
    G.set_superresolution_grad(True)
    assert G.rendering_kwargs["superresolution_noise_mode"] == "none"
    G.rendering_kwargs.update(density_reg=0.25, reg_type="l1", density_reg_p_dist=0.004)
    D = DC.fill_discriminator(P.DualDiscriminator(c_dim=25, img_resolution=512, img_channels=3, cond_mode="resnetcond_8", channel_base=2048,
                                                  channel_max=32), 6).cuda()
    gen = torch.Generator().manual_seed(21)
    cam = lambda az: torch.as_tensor(P.cameras.camera_label(0.0, az, 1.0, 30.0), dtype=torch.float32).reshape(1, 25).cuda()
    cond = {"resnet_feats": torch.randn(1, 16, generator=gen).cuda()}
    for i, (key, az) in enumerate((("image_ortho_front", 0.0), ("image", 25.0))):
        cond[key] = torch.rand(1, 3, 512, 512, generator=gen).cuda()
        cond[key + "_alpha"] = LC.blob_alpha(1, 512, 30 + i).cuda()
        cond[key + "_xyz"] = (torch.rand(1, 3, 512, 512, generator=gen).cuda() - 0.5) * 0.5
        cond[key + "_camera"] = cam(az)
    inp = dict(real_img=torch.randn(1, 3, 512, 512, generator=gen).cuda(), real_c=cam(10.0), real_cond=cond,
               gen_z=torch.randn(1, G.backbone.z_dim, generator=gen).cuda(), gen_c=cam(-15.0))
    kw = dict(LC.LAMBDAS, r1_gamma=0, blur_init_sigma=10, blur_fade_kimg=200, neural_rendering_resolution_initial=16, gpc_reg_prob=0.5,
              gpc_reg_fade_kimg=1, dual_discrimination=True)
    small = _SmallG(G)
    loss = P.StyleGAN2LossOrthoCondA(device=torch.device("cuda"), G=small, D=D, augment_pipe=None, lpips_model=LC.lpips_stand_in, **kw)
    return dict(G=G, D=D, small=small, loss=loss, inp=inp)


def _run(P, monkeypatch, rs, phase, seed=5):
    reports = {}
    monkeypatch.setattr(P.loss, "report", lambda name, value: reports.__setitem__(name, value.detach().clone()))
    rs["G"].zero_grad(set_to_none=True)
    rs["D"].zero_grad(set_to_none=True)
    rs["small"].outs.clear()
    torch.manual_seed(seed)
    rs["loss"].accumulate_gradients(phase=phase, gain=1.0, cur_nimg=0, **rs["inp"])  # cur_nimg 0: blur sigma 10, 61 taps
    return reports


def _grad_census(mod):
    """(parameters that require grad, the names of those without a finite gradient, the names of those whose gradient is all zero)."""
    named = [(n, p) for n, p in mod.named_parameters() if p.requires_grad and _takes_part(n)]
    bad = [n for n, p in named if p.grad is None or not torch.isfinite(p.grad).all()]
    zero = [n for n, p in named if p.grad is not None and torch.count_nonzero(p.grad) == 0]
    return named, bad, zero


def _takes_part(name):
    """The super-resolution runs with rendering_kwargs['superresolution_noise_mode'] == 'none' (the trainer's setting as well, triplane.py:233):
    its noise strengths take no part in any phase and get no gradient, in the reference as here."""
    return not (name.startswith("superresolution.") and name.endswith(".noise_strength"))


@pytest.mark.parametrize("phase", ["Gcond", "Gmain", "Greg", "Dmain"])
def test_real_step(P, monkeypatch, real_step, phase):
    rs = real_step
    reports = _run(P, monkeypatch, rs, phase)
    mod = rs["D"] if phase == "Dmain" else rs["G"]
    named, bad, zero = _grad_census(mod)
    if phase == "Greg":  # the density alone: the colour head and the super-resolution are not part of the phase
        named = [(n, p) for n, p in named if p.grad is not None]
        bad = [n for n in bad if any(n == m for m, _ in named)]
        assert any(n.startswith("backbone.synthesis") for n, _ in named) and any(n.startswith("decoder") for n, _ in named)
    print(f"{phase}: {len(named)} parameters, without finite gradient {bad}, all-zero gradient {zero}")
    assert named and bad == []
    assert zero == []
    if phase == "Gcond":
        out, cond = rs["small"].outs[-1], rs["inp"]["real_cond"]
        terms, _, _ = LC.view_terms_impl_torch(out["image_weights"].detach(), out["image_xyz"].detach(), cond["image_ortho_front_alpha"],
                                               cond["image_ortho_front_xyz"], "z", None, False)
        l1 = (out["image"].detach() - cond["image_ortho_front"]).abs().mean()
        lp = LC.lpips_stand_in(out["image"].detach(), cond["image_ortho_front"]).mean()
        lam = [LC.LAMBDAS[f"lambda_Gcond_{t}"] for t in ("lpips", "l1", "alpha_l2", "depth_l2")]
        want = {"Loss/G/cond/lpips": lp, "Loss/G/cond/l1": l1, "Loss/G/cond/alpha_l2": terms[0], "Loss/G/cond/depth_l2": terms[1],
                "Loss/G/cond": lam[0] * lp + lam[1] * l1 + lam[2] * terms[0] + lam[3] * terms[1]}
        key = "Loss/G/cond"
    elif phase in ("Gmain", "Dmain"):
        out = rs["small"].outs[-1]
        with torch.no_grad():
            f = P.ops.gaussian_filter(10, "cuda")
            blurred = LC.blur_torch(out["image"].detach(), f)
            logits = rs["D"]({"image": blurred, "image_raw": out["image_raw"].detach()}, rs["inp"]["gen_c"], rs["small"]._cond(rs["inp"]["real_cond"]))
        want = {"Loss/scores/fake": logits}
        key = "Loss/scores/fake"
    else:
        want, key = {}, None
    assert set(want) <= set(reports), sorted(reports)
    for k, v in want.items():
        err = float((reports[k] - v).abs().max()) / max(float(v.abs().max()), 1e-30)
        print(f"{phase} {k}: reported {reports[k].flatten()[:2].tolist()} recomputed {v.flatten()[:2].tolist()} ({err:.2e})")
        assert err <= 1e-4, (k, err)
    # an Adam step changes the next call's loss
    def scalar():
        if key is not None:
            return reports[key].double().mean().item()
        return sum(float(p.grad.double().abs().sum()) for _, p in named)  # Greg reports nothing: its gradient stands for it
    before = scalar()
    torch.optim.Adam([p for _, p in named], lr=1e-2).step()
    rs["G"].clear_memo()
    reports = _run(P, monkeypatch, rs, phase)
    after = scalar()
    print(f"{phase}: {before!r} -> {after!r}")
    assert after == after and after != before
