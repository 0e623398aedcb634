"""GPU: gradients of the renderer and of run_model (include/p3d_render_grad.h) — against the reference's own autograd
(tests/golden/grad_*.npz, tests/golden/make_golden_grad.py), against an fp64 torch restatement at the HIP forward's own merged
depths, bitwise-unchanged forwards in grad mode, finiteness / masks, lr_multiplier gains, repeatability, argument errors."""
import ctypes as C

import numpy as np
import pytest
import torch

import p3d_testing as T
from render_grad_ref import restate64

pytestmark = pytest.mark.gpu

GRAD_CASES = ["grad_persp_crop_cull", "grad_ortho_binarize", "grad_sf0", "grad_plane_mode0"]
# relative L2 per tensor vs the reference's fp32 CPU autograd: observed <= 2.7e-6 (planes of the cull cases; decoder <= 3.3e-7) on the
# MI355X; the test prints the values
REL_TOL = 2e-5
# vs the float64 restatement at bench scale: observed <= 1.6e-5 (planes; decoder <= 3.3e-6)
REL_TOL_FP64 = 5e-5


@pytest.fixture(scope="module")
def P():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import panic3d_amd
    panic3d_amd._lib.lib()
    return panic3d_amd


DEV = "cuda:0"


def make_decoder(P, raw, force_sigmoid, lr_mul=1.0):
    dec = P.generator.OSGDecoder(32, {"decoder_lr_mul": lr_mul, "decoder_output_dim": 32})
    with torch.no_grad():
        for t, v in zip((dec.net[0].weight, dec.net[0].bias, dec.net[2].weight, dec.net[2].bias), raw):
            t.copy_(torch.from_numpy(np.asarray(v)))
    dec.set_force_sigmoid(bool(force_sigmoid))
    return dec.to(DEV)


def rel_l2(ours, ref):
    ours, ref = np.asarray(ours, np.float64), np.asarray(ref, np.float64)
    fin = np.isfinite(ref)
    return float(np.linalg.norm((ours - ref)[fin]) / max(np.linalg.norm(ref[fin]), 1e-30))


def cotangents(seed, N, R):
    g = torch.Generator().manual_seed(int(seed))
    return [torch.randn(N, R, k, generator=g).to(DEV) for k in (32, 1, 1, 3)]


def grads_of(dec):
    return [t.grad.detach().cpu().numpy() for t in (dec.net[0].weight, dec.net[0].bias, dec.net[2].weight, dec.net[2].bias)]


@pytest.mark.parametrize("name", GRAD_CASES)
def test_render_grad_vs_reference(P, name):
    g = T.load_golden(name + ".npz")
    m = {k[5:]: g[k].item() for k in g if k.startswith("meta_")}
    N, Sc, Sf, seed = int(m["N"]), int(m["Sc"]), int(m["Sf"]), int(m["seed"])
    planes_np = T.make_planes(seed, N, int(m["H"]), int(m["W"]), scale=float(m["plane_scale"]), smooth=int(m["smooth"]))
    assert T.checksum(planes_np) == str(g["planes_checksum"])
    raw = T.make_decoder_params(seed + 1, 1.0, float(m["sigma_gain"]))
    dec = make_decoder(P, raw, m["force_sigmoid"])
    R = g["rays_o"].shape[1]
    jit, u = T.make_random_draws(seed + 2, N, R, Sc, Sf)
    ro = dict(T.RENDERING_KWARGS, depth_resolution=Sc, depth_resolution_importance=Sf, use_triplane=int(m["use_triplane"]),
              white_back=bool(m["white_back"]))
    rend = P.renderer.ImportanceRenderer(use_triplane=bool(m["use_triplane"]))
    planes = torch.from_numpy(planes_np).to(DEV).requires_grad_(True)
    kw = dict(triplane_crop=float(m["crop"]) or None, cull_clouds=float(m["cull"]) or None, binarize_clouds=float(m["binarize"]) or None)
    out = rend(planes, dec, torch.from_numpy(g["rays_o"]).to(DEV), torch.from_numpy(g["rays_d"]).to(DEV), ro,
               jitter=torch.from_numpy(jit).to(DEV), u=torch.from_numpy(u).to(DEV) if Sf else None, exact=True, **kw)
    assert all(o.grad_fn is not None for o in out), "renderer outputs carry no gradient"
    for key, o in zip(("feat", "depth", "wsum", "xyz"), out):
        assert np.allclose(o.detach().cpu().numpy(), g[key], atol=2e-4, rtol=1e-4), key
    loss = sum((o * c).sum() for o, c in zip(out, cotangents(seed + 3, N, R)))
    loss.backward()
    gp = planes.grad.cpu().numpy()
    assert np.isfinite(gp).all() and all(np.isfinite(x).all() for x in grads_of(dec)), "gradient not finite"
    errs = {"planes": rel_l2(gp, g["grad_planes"])}
    for key, x in zip(("g_w0", "g_b0", "g_w1", "g_b1"), grads_of(dec)):
        if np.isfinite(g[key]).all():
            errs[key] = rel_l2(x, g[key])
    print(name, {k: f"{v:.2e}" for k, v in errs.items()})
    assert max(errs.values()) <= REL_TOL, errs


def test_run_model_grad_vs_reference(P):
    g = T.load_golden("grad_run_model.npz")
    m = {k[5:]: g[k].item() for k in g if k.startswith("meta_")}
    N, M, seed = int(m["N"]), int(m["M"]), int(m["seed"])
    planes_np = T.make_planes(seed, N, int(m["H"]), int(m["W"]), smooth=int(m["smooth"]))
    dec = make_decoder(P, T.make_decoder_params(seed + 1, 1.0, 1.0), m["force_sigmoid"])
    coords = torch.from_numpy(T.make_points(seed + 2, N, M)).to(DEV)
    rend = P.renderer.ImportanceRenderer(use_triplane=bool(m["use_triplane"]))
    planes = torch.from_numpy(planes_np).to(DEV).requires_grad_(True)
    ro = dict(T.RENDERING_KWARGS, use_triplane=int(m["use_triplane"]))
    out = rend.run_model(planes, dec, coords, torch.zeros_like(coords), ro)
    gen = torch.Generator().manual_seed(seed + 3)
    gs, gr = torch.randn(N, M, 1, generator=gen).to(DEV), torch.randn(N, M, 32, generator=gen).to(DEV)
    ((out["sigma"] * gs).sum() + (out["rgb"] * gr).sum()).backward()
    errs = {"planes": rel_l2(planes.grad.cpu().numpy(), g["grad_planes"])}
    for key, x in zip(("g_w0", "g_b0", "g_w1", "g_b1"), grads_of(dec)):
        errs[key] = rel_l2(x, g[key])
    print("run_model", {k: f"{v:.2e}" for k, v in errs.items()})
    assert max(errs.values()) <= REL_TOL, errs


BENCH_MODES = [  # (Sc, Sf, exact, views, ro overrides)
    (48, 48, True, 1, {}),
    (48, 48, False, 1, {}),
    (96, 96, False, 1, {}),
    (48, 48, True, 4, {}),
    (32, 32, True, 1, {"disparity_space_sampling": True}),
    (32, 32, False, 1, {"ray_start": "auto", "ray_end": "auto"}),
]


def bench_inputs(P, Sc, Sf, views, over, res=128, odd=False):
    planes_np, raw = T.make_bench_scene("surface")
    ro = dict(T.bench_rendering_kwargs(Sc, Sf), **over)
    rays = []
    for v in range(views):
        o, d = P.cameras.rays_from_label(P.cameras.camera_label(0.0, 20.0 + 40.0 * v, 1.0, 30.0)[None], res)
        rays.append((o, d))
    o = torch.cat([r[0] for r in rays]).to(DEV)
    d = torch.cat([r[1] for r in rays]).to(DEV)
    if odd:
        o, d = o[:, :res * res - 37].contiguous(), d[:, :res * res - 37].contiguous()
    return planes_np, raw, ro, o, d


@pytest.mark.parametrize("mode", range(len(BENCH_MODES)))
def test_render_grad_vs_fp64_restatement(P, mode):
    Sc, Sf, exact, views, over = BENCH_MODES[mode]
    planes_np, raw, ro, o, d = bench_inputs(P, Sc, Sf, views, over, odd=(mode == len(BENCH_MODES) - 1))
    N, R = o.shape[:2]
    torch.manual_seed(1234)
    jitter = torch.rand(N, R, Sc, 1, device=DEV)
    u = torch.rand(N * R, Sf, device=DEV)
    kw = dict(T.BENCH_KW)
    dec = make_decoder(P, raw, kw.pop("force_sigmoid"))
    dec.set_force_sigmoid(True)
    rend = P.renderer.ImportanceRenderer(use_triplane=bool(ro["use_triplane"]))
    base = torch.from_numpy(planes_np).to(DEV).requires_grad_(True)
    planes = base.expand(N, -1, -1, -1, -1) if views > 1 else base
    out = rend(planes, dec, o, d, ro, jitter=jitter, u=u, exact=exact, per_view_clamp=views > 1, **kw)
    cot = cotangents(77, N, R)
    sum((x * c).sum() for x, c in zip(out, cot)).backward()
    # the forward's merged depths and masked densities (exact forward dumps: same depths as the tolerance one)
    opts = rend._opts(ro, dec, fast_color=False, **kw)
    limits = None
    if ro.get("ray_start") == "auto":
        limits = P.cameras.patch_ray_limits(*P.cameras.ray_limits_box(o, d, ro["box_warp"]))
    with torch.no_grad():
        mlp = P.renderer.decoder_params(dec, live=False)
        *_, dm = P.ops.render(P.ops.planes_to_nhwc(base.detach()), o, d, jitter, u, mlp, opts, dumps=("depths_sorted", "sigma_sorted"),
                              per_view_clamp=views > 1, ray_limits=limits)
    gp64, gm64 = restate64(base.detach(), mlp, o, d, dm["depths_sorted"].reshape(N, R, -1), dm["sigma_sorted"], opts, ro,
                           [c.double() for c in cot], views > 1, True)
    gains = [dec.net[0].weight_gain, dec.net[0].bias_gain, dec.net[2].weight_gain, dec.net[2].bias_gain]
    errs = {"planes": rel_l2(base.grad.cpu().numpy(), gp64.cpu().numpy())}
    for k, x, ref, gn in zip(("w0", "b0", "w1", "b1"), grads_of(dec), gm64, gains):
        errs[k] = rel_l2(x, (ref * gn).cpu().numpy())
    print(BENCH_MODES[mode], {k: f"{v:.2e}" for k, v in errs.items()})
    assert max(errs.values()) <= REL_TOL_FP64, errs


@pytest.mark.parametrize("mode", range(len(BENCH_MODES)))
def test_grad_mode_forward_is_bitwise_unchanged(P, mode):
    Sc, Sf, exact, views, over = BENCH_MODES[mode]
    planes_np, raw, ro, o, d = bench_inputs(P, Sc, Sf, views, over, odd=(mode == len(BENCH_MODES) - 1))
    N, R = o.shape[:2]
    torch.manual_seed(99)
    jitter, u = torch.rand(N, R, Sc, 1, device=DEV), torch.rand(N * R, Sf, device=DEV)
    kw = dict(T.BENCH_KW)
    dec = make_decoder(P, raw, kw.pop("force_sigmoid"))
    rend = P.renderer.ImportanceRenderer(use_triplane=True)
    base = torch.from_numpy(planes_np).to(DEV)
    planes = base.expand(N, -1, -1, -1, -1) if views > 1 else base
    with torch.no_grad():
        ref = rend(planes, dec, o, d, ro, jitter=jitter, u=u, exact=exact, per_view_clamp=views > 1, **kw)
    out = rend(planes.detach().requires_grad_(mode % 2 == 0), dec, o, d, ro, jitter=jitter, u=u, exact=exact,
               per_view_clamp=views > 1, **kw)
    assert out[0].grad_fn is not None
    for a, b in zip(out, ref):
        assert torch.equal(a.detach(), b)


def test_masked_densities_get_zero_gradient(P):
    """binarize_clouds overwrites every density: a loss on wsum / depth alone reaches no plane texel and no decoder weight."""
    planes_np, raw, ro, o, d = bench_inputs(P, 16, 16, 1, {}, res=32)
    dec = make_decoder(P, raw, True)
    rend = P.renderer.ImportanceRenderer(use_triplane=True)
    planes = torch.from_numpy(planes_np).to(DEV).requires_grad_(True)
    feat, depth, wsum, xyz = rend(planes, dec, o, d, ro, binarize_clouds=0.5, exact=True)
    (wsum.sum() + depth.sum()).backward()
    assert torch.count_nonzero(planes.grad) == 0
    assert all(not np.any(x) for x in grads_of(dec))


def test_empty_rays_and_clamped_depths_are_finite(P):
    planes_np, raw, ro, o, d = bench_inputs(P, 24, 24, 1, {}, res=32)
    dec = make_decoder(P, raw, True)
    rend = P.renderer.ImportanceRenderer(use_triplane=True)
    planes = torch.from_numpy(planes_np).to(DEV).requires_grad_(True)
    out = rend(planes, dec, o, d, ro, triplane_crop=0.3, cull_clouds=0.5)
    assert int((out[2] == 0).sum()) > 0, "the scene must hold empty rays"
    sum((x * c).sum() for x, c in zip(out, cotangents(5, 1, o.shape[1]))).backward()
    assert torch.isfinite(planes.grad).all() and all(np.isfinite(x).all() for x in grads_of(dec))


def test_raw_parameter_gradients_carry_the_gains(P):
    """The raw net.*.weight / bias receive d(pre-scaled) * gain (lr_multiplier 0.5: every gain differs from 1)."""
    planes_np, raw, ro, o, d = bench_inputs(P, 16, 16, 1, {}, res=32)
    dec = make_decoder(P, raw, True, lr_mul=0.5)
    rend = P.renderer.ImportanceRenderer(use_triplane=True)
    planes = torch.from_numpy(planes_np).to(DEV)
    N, R = o.shape[:2]
    torch.manual_seed(4)
    jitter, u = torch.rand(N, R, 16, 1, device=DEV), torch.rand(N * R, 16, device=DEV)
    out = rend(planes, dec, o, d, ro, jitter=jitter, u=u, exact=True)
    cot = cotangents(6, N, R)
    sum((x * c).sum() for x, c in zip(out, cot)).backward()
    with torch.no_grad():
        mlp = P.renderer.decoder_params(dec, live=False)
        opts = rend._opts(ro, dec, fast_color=False)
        nhwc = P.ops.planes_to_nhwc(planes)
        *_, dm = P.ops.render(nhwc, o, d, jitter, u, mlp, opts, ray_tile_w=32, dumps=("depths_sorted",))
        _, dmlp = P.ops.render_backward(nhwc, o, d, dm["depths_sorted"], mlp, opts, cot)
    l0, l2 = dec.net[0], dec.net[2]
    for t, gm, gain in zip((l0.weight, l0.bias, l2.weight, l2.bias), dmlp, (l0.weight_gain, l0.bias_gain, l2.weight_gain, l2.bias_gain)):
        assert gain != 1
        assert torch.equal(t.grad, gm * gain)


def test_repeatable_backward(P):
    planes_np, raw, ro, o, d = bench_inputs(P, 32, 32, 1, {}, res=64)
    dec = make_decoder(P, raw, True)
    rend = P.renderer.ImportanceRenderer(use_triplane=True)
    N, R = o.shape[:2]
    torch.manual_seed(3)
    jitter, u = torch.rand(N, R, 32, 1, device=DEV), torch.rand(N * R, 32, device=DEV)
    res = []
    for _ in range(2):
        dec.zero_grad(set_to_none=True)
        planes = torch.from_numpy(planes_np).to(DEV).requires_grad_(True)
        out = rend(planes, dec, o, d, ro, jitter=jitter, u=u, **{k: v for k, v in T.BENCH_KW.items() if k != "force_sigmoid"})
        sum((x * c).sum() for x, c in zip(out, cotangents(8, N, R))).backward()
        res.append((planes.grad.clone(), grads_of(dec)))
    for a, b in zip(res[0][1], res[1][1]):
        assert np.array_equal(a, b), "decoder gradients must be bitwise reproducible"
    assert torch.allclose(res[0][0], res[1][0], rtol=1e-5, atol=1e-6 * float(res[0][0].abs().max()))


def test_unsupported_ray_gradients_raise(P):
    planes_np, raw, ro, o, d = bench_inputs(P, 16, 16, 1, {}, res=16)
    dec = make_decoder(P, raw, True)
    rend = P.renderer.ImportanceRenderer(use_triplane=True)
    planes = torch.from_numpy(planes_np).to(DEV)
    with pytest.raises(NotImplementedError, match="ray_origins"):
        rend(planes, dec, o.clone().requires_grad_(True), d, ro)
    with pytest.raises(NotImplementedError, match="ray_directions"):
        rend(planes, dec, o, d.clone().requires_grad_(True), ro)
    with pytest.raises(NotImplementedError, match="sample_coordinates"):
        rend.run_model(planes, dec, o.clone().requires_grad_(True), o, ro)


def test_backward_entry_point_errors(P):
    L = P._lib.lib()
    o = P.ops.make_opts(T.RENDERING_KWARGS)
    fake = C.c_void_p(256)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    wsp = C.c_void_p(ws.data_ptr())
    args = [fake, 1, 8, 8, fake, fake, 16, fake, fake, fake, fake, fake, C.byref(o), None, None, None, None, fake, fake, fake, fake, fake,
            wsp, 1 << 20, None]
    bad = list(args)
    bad[7] = None  # no depths
    assert L.p3d_render_backward_f32(*bad) == -1
    bad = list(args)
    bad[23] = 16  # workspace too small
    assert L.p3d_render_backward_f32(*bad) == -3
    bad = list(args)
    bad[2] = 5000  # H beyond the 32-bit offsets
    assert L.p3d_render_backward_f32(*bad) == -2
    assert L.p3d_triplane_decode_backward_f32(fake, 1, 8, 8, None, 16, fake, fake, fake, fake, C.byref(o), None, None, fake, fake, fake,
                                              fake, fake, wsp, 1 << 20, None) == -1
    with pytest.raises(RuntimeError, match="depths_sorted"):
        P.ops.render_backward(torch.zeros(1, 3, 8, 8, 32, device=DEV), torch.zeros(1, 4, 3, device=DEV), torch.zeros(1, 4, 3, device=DEV),
                              None, P.ops.prescale_mlp(*(torch.zeros(s, device=DEV) for s in ((64, 32), (64,), (33, 64), (33,))), 1, 1, 1, 1),
                              o, (None, None, None, None))


def test_generator_f_outputs_carry_decoder_gradients(P):
    """G.f with grad enabled: image_raw / image_depth / image_weights / image_xyz carry gradients to the decoder; `image`
    (super-resolution) stays inference-only; the outputs are the no-grad call's bits (same draws)."""
    import p3d_shared_cases as MC
    G = MC.memo_generator("cuda")
    T.fill_generator_params(G, 3)
    G.set_view_replay(False)
    gen = torch.Generator().manual_seed(11)
    cond = {"image_ortho_front": torch.rand(1, 3, 32, 32, generator=gen).cuda(), "resnet_feats": torch.randn(1, 16, generator=gen).cuda()}
    x = lambda: dict(seeds=[4], cond=cond, elevations=torch.zeros(1, device="cuda"), azimuths=torch.zeros(1, device="cuda"),
                     neural_rendering_resolution=16, noise_mode="const", triplane_crop=0.1, cull_clouds=0.5)
    keys = ("image_raw", "image_depth", "image_weights", "image_xyz")
    torch.manual_seed(21)
    with torch.no_grad():
        ref = G.f(x())
        ref = {k: ref[k].clone() for k in keys + ("image",)}
    G.clear_memo()
    torch.manual_seed(21)
    out = G.f(x())
    assert out["image"].grad_fn is None
    for k in keys:
        assert out[k].grad_fn is not None, k
        assert torch.equal(out[k].detach(), ref[k]), k
    assert torch.equal(out["image"], ref["image"])
    l0 = G.decoder.net[0]
    l0.weight.grad = None
    sum(out[k].sum() for k in keys).backward()
    assert l0.weight.grad is not None and torch.isfinite(l0.weight.grad).all() and torch.count_nonzero(l0.weight.grad) > 0
