"""GPU (-m gpu): the dual discriminator on the HIP kernels.  Kernel level: p3d_conv2d_act_f32 with its backward (ops.conv2d_act under
autograd) and p3d_mbstd_f32 / p3d_mbstd_backward_f32 against float64 at the smallest shapes that can still go wrong, under the
per-layer gate of tests/discriminator_cases.py (rel-L2 <= 1e-5 per tensor, the long sums to 8 sqrt(K) 2^-24 sum|terms|; the gate's
sensitivity to a dropped tap, an unflipped weight, the mask taken from the wrong tensor and a mean over the wrong axis is shown on CPU in
tests/test_discriminator_cpu.py).  Network level: the small network of tests/golden/discriminator.npz against the reference's fp32
autograd and float64, run-to-run bits, grad-mode against no_grad bits, an optimiser step.  End to end: one Gmain-shaped step through
G.f and D.  Trainer size: one 512^2 forward + backward.  On the parent commit the module, the operators and the symbols do not exist."""
import pytest
import torch

import discriminator_cases as DC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P():
    import panic3d_amd
    panic3d_amd.build()
    panic3d_amd._lib.lib()
    return panic3d_amd


@pytest.mark.parametrize("shape", sorted(DC.CONV_SHAPES))
@pytest.mark.parametrize("variant", sorted(DC.CONV_VARIANTS))
def test_conv2d_act_and_its_backward(P, shape, variant):
    c = DC.conv_case(shape, variant)
    ref = DC.conv_layer_f64(*DC.conv_case_args(c))
    a, b = DC.run_conv_layer(P.ops, c, "cuda"), DC.run_conv_layer(P.ops, c, "cuda")
    assert DC.layer_gate(a, ref) == []
    assert all(torch.equal(a[k], b[k]) for k in a if a[k] is not None), "two runs differ"


def test_conv2d_act_checks_its_arguments(P):
    x, wk = torch.zeros(1, 4, 5, 5, device="cuda"), torch.zeros(9, 4, 3, device="cuda")
    with pytest.raises(RuntimeError):
        P.ops.conv2d_act(x, wk, stride=3, pad=1)
    with pytest.raises(RuntimeError):
        P.ops.conv2d_act(x, wk, pad=3)
    with pytest.raises(RuntimeError):
        P.ops.conv2d_act(x, wk, pad=1, res=torch.zeros(1, 3, 4, 4, device="cuda"))
    with pytest.raises(RuntimeError):
        P.ops.minibatch_std(torch.zeros(6, 4, 4, 4, device="cuda"), 4, 1)  # 4 does not divide 6


@pytest.mark.parametrize("name", sorted(DC.MBSTD_SHAPES))
def test_mbstd_and_its_backward(P, name):
    c = DC.mbstd_case(name)
    ref = DC.mbstd_f64(c)
    runs = []
    for _ in range(2):
        x = c["x"].clone().cuda().requires_grad_(True)
        y = P.ops.minibatch_std(x, c["group"], c["F"])
        with torch.no_grad():
            assert torch.equal(y.detach(), P.ops.minibatch_std(x.detach(), c["group"], c["F"]))
        y.backward(c["gy"].cuda())
        runs.append(dict(y=y.detach().cpu(), gx=x.grad.cpu()))
    assert torch.equal(runs[0]["y"][:, :c["x"].shape[1]], c["x"])
    assert DC.mbstd_gate(runs[0], ref, c) == []
    assert torch.equal(runs[0]["y"], runs[1]["y"]) and torch.equal(runs[0]["gx"], runs[1]["gx"])


def test_discriminator_vs_reference(P):
    DC.discriminator_against_fixture(P, "cuda")


def test_discriminator_bits_and_memo(P):
    """Two runs bitwise equal in the logits, every parameter gradient and the gradient of the concatenated 6-channel input (torch's
    interpolate backward in front of it is not bitwise reproducible); grad-mode logits are the no_grad logits bit for bit; after an
    SGD step the next call of either kind sees the new weights."""
    D = DC.fill_discriminator(P.DualDiscriminator(**DC.D_KW)).cuda()
    inp = {k: v.cuda() for k, v in DC.discriminator_inputs().items()}
    seen = []
    hook = D.b32.register_forward_pre_hook(lambda mod, args: seen.append(args[1]) or (args[1].retain_grad() if args[1].requires_grad else None))

    def run():
        D.zero_grad(set_to_none=True)
        seen.clear()
        image, raw = inp["image"].clone().requires_grad_(True), inp["image_raw"].clone().requires_grad_(True)
        logits = D({"image": image, "image_raw": raw}, inp["c"], {"resnet_feats": inp["feats"]})
        (logits * inp["g"]).sum().backward()
        assert tuple(seen[0].shape) == (DC.BATCH, 6, 32, 32)
        return {"logits": logits.detach().clone(), "g_cat": seen[0].grad.clone(), **{n: p.grad.clone() for n, p in D.named_parameters()}}
    a, b = run(), run()
    hook.remove()
    assert len(a) == 2 + len(list(D.parameters()))
    for k in a:
        assert torch.equal(a[k], b[k]), k
    call = lambda: D({"image": inp["image"], "image_raw": inp["image_raw"]}, inp["c"], {"resnet_feats": inp["feats"]})
    with torch.no_grad():
        cold = call().clone()
    memo = D.b16.conv0._scaled_wb
    assert torch.equal(cold, a["logits"])
    assert call().grad_fn is not None and D.b16.conv0._scaled_wb is memo
    torch.optim.SGD(D.parameters(), lr=1e-3).step()  # (the gradients of run b)
    with torch.no_grad():
        stepped = call().clone()
    assert not torch.equal(stepped, cold) and D.b16.conv0._scaled_wb is not memo
    assert torch.equal(call().detach(), stepped)


def test_gmain_step_reaches_the_generator(P):
    """G.f -> {'image', 'image_raw'} -> D -> softplus(-logits).mean().backward(): finite, non-zero gradients on a backbone, a decoder and
    a super-resolution parameter."""
    import p3d_shared_cases as MC
    import p3d_testing as T
    G = MC.memo_generator("cuda")
    T.fill_generator_params(G, 3)
    G.set_view_replay(False)
    G.set_superresolution_grad(True)
    gen = torch.Generator().manual_seed(11)
    cond = {"image_ortho_front": torch.rand(1, 3, 32, 32, generator=gen).cuda(), "resnet_feats": torch.randn(1, 16, generator=gen).cuda()}
    z = torch.randn(1, G.backbone.z_dim, generator=gen).cuda()
    D = DC.fill_discriminator(P.DualDiscriminator(c_dim=25, img_resolution=512, img_channels=3, cond_mode="resnetcond_8", channel_base=2048,
                                                  channel_max=32), 6).cuda()
    out = G.f(dict(z=z, cond=cond, elevations=torch.zeros(1, device="cuda"), azimuths=torch.zeros(1, device="cuda"),
                   neural_rendering_resolution=16, noise_mode="const", triplane_crop=0.1, cull_clouds=0.5))
    assert out["image"].grad_fn is not None and out["image_raw"].grad_fn is not None
    logits = D({"image": out["image"], "image_raw": out["image_raw"]}, torch.zeros(1, 25, device="cuda"), cond)
    assert tuple(logits.shape) == (1, 1)
    torch.nn.functional.softplus(-logits).mean().backward()
    for name, mod in (("backbone", G.backbone.synthesis), ("decoder", G.decoder), ("superresolution", G.superresolution)):
        gs = [p.grad for p in mod.parameters() if p.grad is not None]
        assert gs and all(torch.isfinite(g).all() for g in gs) and any(torch.count_nonzero(g) > 0 for g in gs), name
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in D.parameters())


def test_trainer_size_forward_backward(P):
    """The trainer's discriminator (512^2, 3 + 3 channels, channel_base 32768, channel_max 512), batch 1: every range check passes."""
    torch.manual_seed(0)
    D = P.DualDiscriminator(c_dim=25, img_resolution=512, img_channels=3, cond_mode="resnetcond_8").cuda()
    image = torch.randn(1, 3, 512, 512, device="cuda", requires_grad=True)
    raw = torch.randn(1, 3, 128, 128, device="cuda", requires_grad=True)
    logits = D({"image": image, "image_raw": raw}, torch.randn(1, 25, device="cuda"), {"resnet_feats": torch.randn(1, 16, device="cuda")})
    torch.nn.functional.softplus(-logits).mean().backward()
    assert tuple(logits.shape) == (1, 1) and torch.isfinite(logits).all()
    assert torch.isfinite(image.grad).all() and torch.isfinite(raw.grad).all() and torch.count_nonzero(image.grad) > 0
    assert all(p.grad is not None and torch.isfinite(p.grad).all() and torch.count_nonzero(p.grad) > 0 for p in D.parameters())
