"""GPU (-m gpu): the R1 penalty on the HIP kernels (include/p3d_r1.h).  Kernel level: p3d_conv2d_mask_f32 at the ragged
shapes of tests/discriminator_cases.py with every activation / clamp variant, bit for bit against the two launches it fuses and under the
layer gate against float64; p3d_mbstd_backward2_f32 against float64 autograd, at most 4x the error of torch's own binary32 double autograd
(the gate's sensitivity to a dropped term is shown on CPU in tests/test_r1_cpu.py); p3d_r1_sumsq_f32; single layers' double backward.
Network level: the small network of tests/golden/r1.npz at two image scales, every gradient against float64 relative to the reference's
own error; a seeded fault; run-to-run bits; one Dreg through the loss on the real discriminator; one trainer-size run.  On the parent
commit the switch, the operators and the symbols do not exist.

Run-to-run bits: everything this package launches is bitwise reproducible.  torch's backward of the antialiased bilinear resize in
front of the discriminator (image_raw -> 2x) adds with atomics, so g_raw — and with it the penalty and whatever is differentiated from
it — is not; the bit tests therefore differentiate with respect to `image` alone (the single-discrimination call), where no torch
kernel with atomics runs, and for the dual call compare what does not pass through that resize."""
import pytest
import torch

import discriminator_cases as DC
import loss_cases as LC
import p3d_testing as T
import r1_cases as RC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P():
    import panic3d_amd
    panic3d_amd.build()
    panic3d_amd._lib.lib()
    return panic3d_amd


@pytest.fixture(scope="module")
def golden():
    return T.load_golden("r1.npz")


# ---- p3d_conv2d_mask_f32 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sorted(DC.CONV_SHAPES))
@pytest.mark.parametrize("variant", sorted(DC.CONV_VARIANTS))
def test_conv2d_mask_is_the_two_launches_and_passes_the_gate(P, shape, variant):
    c = RC.mask_case(shape, variant)
    h, wk, pre = c["h"].cuda(), c["wk"].cuda(), c["pre"].cuda()
    args = (c["act"], c["gain_value"], c["clamp"], c["stride"], c["pad"])
    got = P.ops._conv2d_mask_impl(h, wk, pre, *args)
    z = P.ops.conv2d_act(h, wk, None, act="linear", gain=1.0, clamp=None, stride=c["stride"], pad=c["pad"])
    two, _ = P.ops._bias_act_backward_meta(pre, z, args[:3])
    assert torch.equal(got, two), "the fused launch differs from conv2d_act + bias_act_backward"
    assert torch.equal(got, P.ops._conv2d_mask_impl(h, wk, pre, *args)), "two runs differ"
    ref, absref, K = RC.conv2d_mask_f64(c["h"], c["wk"], c["pre"], *args)
    q, e = DC.R.gate_ratio(got.cpu(), ref, absref, K), DC.rel_l2(got.cpu(), ref)
    print(f"{shape}/{variant}: gate ratio {q:.3f} of {DC.R.GATE_C:g}, rel-L2 {e:.2e}, zeros {float((ref == 0).double().mean()):.2f}")
    assert q <= DC.R.GATE_C and e <= DC.R.REL_L2
    buf = pre.clone()  # out may alias pre
    rc = P._lib.lib().p3d_conv2d_mask_f32(h.data_ptr(), h.shape[0], h.shape[1], h.shape[2], h.shape[3], wk.data_ptr(), wk.shape[0], wk.shape[2],
                                          pre.shape[2], pre.shape[3], c["stride"], c["pad"], buf.data_ptr(), 1 if c["act"] == "lrelu" else 0, 0.2,
                                          float(c["gain_value"]), float(c["clamp"] if c["clamp"] is not None else -1), buf.data_ptr(),
                                          torch.cuda.current_stream().cuda_stream)
    assert rc == 0 and torch.equal(buf, got)


# ---- p3d_mbstd_backward2_f32 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(RC.MBSTD2_SHAPES))
def test_mbstd_double_backward(P, name):
    c = RC.mbstd2_case(name)
    a, b = RC.run_mbstd2(P.ops, c, "cuda"), RC.run_mbstd2(P.ops, c, "cuda")
    assert all(torch.equal(a[k], b[k]) for k in a), "two runs differ"
    gy0 = c["gy"].clone()
    gy0[:, :c["x"].shape[1]] = 0
    x = c["x"].clone().cuda().requires_grad_(True)
    P.ops.minibatch_std(x, c["group"], c["F"]).backward(gy0.cuda())
    assert torch.equal(a["first"], x.grad.cpu()), "the recorded first gradient differs from the plain one"
    bad, ratios = RC.mbstd2_gate(a, c, verbose=f"{name}: ")
    assert bad == [], ratios
    M = c["x"].shape[0] // min(c["group"], c["x"].shape[0])
    ge = a["g_extra"].reshape(-1, M, c["F"], a["g_extra"].shape[2] * a["g_extra"].shape[3])
    assert torch.equal(ge, ge[:1, :, :, :1].expand_as(ge)), "one value per (group, statistic), broadcast"


# ---- p3d_r1_sumsq_f32 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shapes", [((3, 3, 9, 7), (3, 3, 5, 3)), ((2, 3, 33, 31), None), ((1, 1, 1, 1), (1, 2, 1, 1))])
def test_r1_penalty_kernel(P, shapes):
    g = torch.Generator().manual_seed(7)
    a = torch.randn(shapes[0], generator=g)
    b = torch.randn(shapes[1], generator=g) if shapes[1] is not None else None
    ref = RC.sumsq_torch(a.double(), b.double() if b is not None else None)
    ad, bd = a.cuda().requires_grad_(True), (b.cuda().requires_grad_(True) if b is not None else None)
    pen = P.ops.r1_penalty(ad, bd)
    assert torch.equal(pen.detach(), P.ops.r1_penalty(ad.detach(), bd.detach() if bd is not None else None))
    # binary64 sums, one rounding: half an ulp of the result
    assert float(((pen.detach().cpu().double() - ref).abs() / ref).max()) <= 2.0 ** -24
    cot = torch.randn(shapes[0][0], generator=g)
    pen.backward(cot.cuda())
    assert torch.equal(ad.grad.cpu(), 2 * cot.view(-1, 1, 1, 1) * a)
    assert bd is None or torch.equal(bd.grad.cpu(), 2 * cot.view(-1, 1, 1, 1) * b)


# ---- single layers ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,variant", [("conv0", "clamp"), ("conv1", "residual"), ("fromrgb", "bias_lrelu")])
def test_conv_layer_double_backward(P, shape, variant):
    c = DC.conv_case(shape, variant)
    h = torch.randn(c["x"].shape, generator=torch.Generator().manual_seed(9))
    ref = RC.conv_layer2_f64(c, h)
    a, b = RC.run_conv_layer2(P.ops, c, h, "cuda"), RC.run_conv_layer2(P.ops, c, h, "cuda")
    assert all(torch.equal(a[k], b[k]) for k in a if a[k] is not None), "two runs differ"
    assert torch.equal(a["gx"], DC.run_conv_layer(P.ops, c, "cuda")["gx"]), "the recorded first gradient differs from the plain one"
    for k in ("gx", "g_gy", "g_wk"):
        e = DC.rel_l2(a[k], ref[k])
        print(f"{shape}/{variant} {k}: rel-L2 {e:.2e}")
        assert e <= DC.R.REL_L2, k
    assert a["g_bias"] is not None and not a["g_bias"].any() and not ref["g_bias"].any()


# ---- the network ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", sorted(RC.SCALES))
def test_network_vs_reference(P, golden, tag):
    ratios = RC.network_against_fixture(P, "cuda", tag, golden)
    print(f"{tag}: worst ratio {max(ratios.values()):.3f} ({max(ratios, key=ratios.get)}) of {RC.MARGIN:g}")
    assert ratios["b4.conv.bias"] == 0.0 and ratios["b4.fc.bias"] == 0.0


def test_network_gate_fails_without_the_mbstd_second_order_path(P, golden, monkeypatch):
    monkeypatch.setattr(P.ops, "mbstd_backward2", lambda x, gy, h, G, Fc: (torch.zeros_like(gy[:, x.shape[1]:]), torch.zeros_like(x)))
    with pytest.raises(AssertionError, match="bias"):
        RC.network_against_fixture(P, "cuda", "s1", golden)


def _image_only(P, D, inp, size=None):
    """Dreg with respect to `image` alone (single discrimination): no torch kernel with atomics runs."""
    image = inp["image"].cuda().requires_grad_(True)
    for p in D.parameters():
        p.grad = None
    logits = D({"image": image, "image_raw": inp["image_raw"].cuda()}, inp["c"].cuda().clone(), {"resnet_feats": inp["feats"].cuda()})
    with P.ops.no_weight_gradients():
        g_image, = torch.autograd.grad([logits.sum()], [image], create_graph=True, only_inputs=True)
    pen = P.ops.r1_penalty(g_image)
    (pen * (RC.GAMMA / 2)).mean().mul(RC.GAIN).backward()
    return {"penalty": pen.detach().clone(), "g_image": g_image.detach().clone(), **{n: p.grad.clone() for n, p in D.named_parameters() if p.grad is not None}}


def test_network_bits_run_to_run(P):
    D = DC.fill_discriminator(P.DualDiscriminator(**DC.D_KW)).cuda()
    D.set_r1_grad(True)
    inp = RC.r1_inputs(1.0)
    a, b = _image_only(P, D, inp), _image_only(P, D, inp)
    assert len(a) == 2 + len(list(D.parameters())) - 1 and "b4.out.bias" not in a
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert all(torch.isfinite(v).all() for v in a.values()) and torch.count_nonzero(a["b32.fromrgb.bias"]) > 0
    # the dual call: the first backward's image gradient does not pass through torch's resize backward
    r1, r2 = (RC.run_module(D, inp, "cuda", penalty=P.ops.r1_penalty, guard=P.ops.no_weight_gradients()) for _ in range(2))
    assert torch.equal(r1["g_image"], r2["g_image"])


def test_dreg_through_the_loss_on_the_real_discriminator(P, monkeypatch):
    """One Dreg of StyleGAN2LossOrthoCondA.accumulate_gradients on DualDiscriminator at 32^2 with a blur of sigma 1.5 in front (ops.blur's
    double backward), against the same phase in float64 on CPU (DC.discriminator_f64, LC.blur_torch): the reported penalty to 1e-5
    relative, every weight's gradient to rel-L2 1e-4 (the first-order network test's bound; the reference's own binary32 error on these
    tensors is 4e-7 .. 2.4e-6), every gradient finite, the set of parameters with a gradient the reference's."""
    D = DC.fill_discriminator(P.DualDiscriminator(**DC.D_KW)).cuda()
    D.set_r1_grad(True)
    G = LC.StandInG(LC.RK).cuda()
    inp = LC.loss_inputs(device="cuda")
    feats = torch.randn(LC.N, 16, generator=torch.Generator().manual_seed(12))
    inp["real_cond"]["resnet_feats"] = feats.cuda()
    reports = {}
    monkeypatch.setattr(P.loss, "report", lambda name, value: reports.__setitem__(name, torch.as_tensor(value).detach().cpu()))
    loss = P.StyleGAN2LossOrthoCondA(device=torch.device("cuda"), G=G, D=D, augment_pipe=None, lpips_model=LC.lpips_stand_in, **LC.LOSS_KW)
    loss.accumulate_gradients(phase="Dreg", gain=LC.GAIN, cur_nimg=LC.NIMG["s1.5"], **inp)
    assert set(reports) == {"Loss/scores/real", "Loss/signs/real", "Loss/r1_penalty", "Loss/D/reg"}
    # float64 on CPU
    d = torch.float64
    real = inp["real_img"].cpu().to(d)
    raw = torch.nn.functional.interpolate(real, size=(LC.RES, LC.RES), mode="bilinear", align_corners=False, antialias=True)
    f = P.ops.gaussian_filter(1.5).to(d)
    image, raw = (LC.blur_torch(t, f).requires_grad_(True) for t in (real, raw))
    p64 = {n: p.detach().cpu().to(d).requires_grad_(True) for n, p in D.named_parameters()}
    logits = DC.discriminator_f64(p64, image, raw, inp["real_c"].cpu().to(d), feats.to(d))
    g_image, g_raw = torch.autograd.grad([logits.sum()], [image, raw], create_graph=True)
    pen = RC.sumsq_torch(g_image, g_raw)
    (pen * (LC.LOSS_KW["r1_gamma"] / 2)).mean().mul(LC.GAIN).backward()
    e = float((reports["Loss/r1_penalty"].double() - pen.detach()).abs().max() / pen.detach().abs().max())
    print(f"penalty {pen.detach().tolist()}: relative error {e:.2e}")
    assert e <= 1e-5
    assert {n for n, p in D.named_parameters() if p.grad is not None} == {n for n, p in p64.items() if p.grad is not None}
    for n, p in D.named_parameters():
        if p.grad is None:
            continue
        assert torch.isfinite(p.grad).all(), n
        if n.endswith(".weight"):
            err = DC.rel_l2(p.grad.cpu(), p64[n].grad)
            print(f"{n}: rel-L2 {err:.2e}")
            assert err <= 1e-4, n
    assert all(p.grad is None for p in G.parameters())


def test_trainer_size_dreg(P):
    """The trainer's discriminator (512^2, channel_base 32768, channel_max 512), batch 2 = one group of two, image alone: every range
    check passes, the penalty and every gradient are finite, every parameter the reference gives a non-zero gradient gets one, and two
    runs agree bit for bit."""
    torch.manual_seed(0)
    D = P.DualDiscriminator(c_dim=25, img_resolution=512, img_channels=3, cond_mode="resnetcond_8").cuda()
    D.set_r1_grad(True)
    g = torch.Generator().manual_seed(1)
    inp = dict(image=torch.randn(2, 3, 512, 512, generator=g), image_raw=torch.randn(2, 3, 128, 128, generator=g), c=torch.randn(2, 25, generator=g),
               feats=torch.randn(2, 16, generator=g))
    a, b = _image_only(P, D, inp), _image_only(P, D, inp)
    assert set(a) == {"penalty", "g_image"} | {n for n, _ in D.named_parameters() if n != "b4.out.bias"}
    for k in a:
        assert torch.isfinite(a[k]).all(), k
        assert torch.equal(a[k], b[k]), k
        if k not in ("b4.conv.bias", "b4.fc.bias"):
            assert torch.count_nonzero(a[k]) > 0, k
    assert not a["b4.conv.bias"].any() and not a["b4.fc.bias"].any()
