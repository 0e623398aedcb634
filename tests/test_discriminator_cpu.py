"""CPU (-m "not gpu"): the dual discriminator's host wiring (discriminator.py, ops.conv2d_act / ops.minibatch_std / ops.fir under
autograd) with the device operators replaced by torch stand-ins (tests/discriminator_cases.py), against the reference's own fp32
autograd (tests/golden/discriminator.npz) and a float64 restatement; the reference's state_dict names; and the layer gates of
tests/test_hip_discriminator.py checked against seeded faults.  On the parent commit the module, the operators and the exported
class do not exist."""
import pytest
import torch

import discriminator_cases as DC
import p3d_testing as T


@pytest.fixture(scope="module")
def P():
    import panic3d_amd
    panic3d_amd.build()
    return panic3d_amd


def test_discriminator_vs_reference(P, monkeypatch):
    DC.install_ops(monkeypatch, P.ops)
    DC.discriminator_against_fixture(P, "cpu")


def test_state_dict_is_the_reference(P):
    g = T.load_golden("discriminator.npz")
    D = P.DualDiscriminator(**DC.D_KW)
    sd = D.state_dict()
    want = dict(zip(g["state_names"].tolist(), g["state_shapes"].tolist()))
    assert {k: ",".join(str(d) for d in v.shape) for k, v in sd.items()} == want
    D2 = DC.fill_discriminator(P.DualDiscriminator(**DC.D_KW), 5)
    D.load_state_dict(D2.state_dict(), strict=True)
    assert all(torch.equal(a, b) for a, b in zip(D.state_dict().values(), D2.state_dict().values()))
    Df = P.DualDiscriminator(**dict(DC.D_KW, block_kwargs={"freeze_layers": 2}))
    assert [n for n, _ in Df.named_parameters()] == g["frozen2_parameters"].tolist()
    frozen = {n.rsplit(".", 1)[0] for n, _ in Df.named_buffers() if n.endswith(".weight")}
    assert frozen == {"b32.fromrgb", "b32.conv0"}
    assert set(Df.state_dict()) == set(sd)
    Df.load_state_dict(D2.state_dict(), strict=True)  # parameters into buffers: the same keys
    assert P.discriminator.DualDiscriminator is P.DualDiscriminator


def test_unused_architectures_raise(P):
    for arch in ("skip", "orig"):
        with pytest.raises(NotImplementedError, match="networks_stylegan2.py"):
            P.DualDiscriminator(**dict(DC.D_KW, architecture=arch))


def test_double_backward_names_r1(P, monkeypatch):
    DC.install_ops(monkeypatch, P.ops)
    D = DC.fill_discriminator(P.DualDiscriminator(**DC.D_KW))
    inp = DC.discriminator_inputs()
    image, raw = (inp[k].clone().requires_grad_(True) for k in ("image", "image_raw"))
    logits = D({"image": image, "image_raw": raw}, inp["c"], {"resnet_feats": inp["feats"]})
    with pytest.raises(RuntimeError, match="R1"):
        torch.autograd.grad([logits.sum()], [image, raw], create_graph=True, only_inputs=True)  # loss_orthocondA.py's R1 call


def test_frozen_layers_and_memo(P, monkeypatch):
    """freeze_layers: the frozen layers get no gradient and keep the memoised operand under autograd; a trainable layer records its
    multiplication live (same bits), and an optimiser step is seen by the next call of either kind."""
    DC.install_ops(monkeypatch, P.ops)
    D = DC.fill_discriminator(P.DualDiscriminator(**dict(DC.D_KW, block_kwargs={"freeze_layers": 2})))
    inp = DC.discriminator_inputs()
    call = lambda: D({"image": inp["image"], "image_raw": inp["image_raw"]}, inp["c"], {"resnet_feats": inp["feats"]})
    with torch.no_grad():
        cold = call().clone()
    memo = D.b16.conv0._scaled_wb
    hot = call()
    assert hot.grad_fn is not None and torch.equal(hot.detach(), cold)
    assert D.b16.conv0._scaled_wb is memo and not memo.requires_grad
    (hot * inp["g"]).sum().backward()
    assert D.b32.conv1.weight.grad is not None and not D.b32.conv0.weight.requires_grad
    torch.optim.SGD(D.parameters(), lr=1e-3).step()
    with torch.no_grad():
        stepped = call()
    assert not torch.equal(stepped, cold) and D.b16.conv0._scaled_wb is not memo
    assert torch.equal(call().detach(), stepped)


@pytest.mark.parametrize("mode", ["antialiased", "classic", "none", 0.5])
def test_filtered_resizing(P, monkeypatch, mode):
    DC.install_ops(monkeypatch, P.ops)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 3, 10, 10, generator=g, requires_grad=True)
    f = P.ops.setup_filter([1, 3, 3, 1])
    y = P.discriminator.filtered_resizing(x, 16, f, filter_mode=mode)
    x64 = x.detach().double().requires_grad_(True)
    y64 = DC.filtered_resizing_any(x64, 16, f.double(), mode)
    assert tuple(y.shape) == (2, 3, 16, 16) and DC.rel_l2(y.detach(), y64.detach()) < 1e-6
    gy = torch.randn(y.shape, generator=g)
    y.backward(gy)
    y64.backward(gy.double())
    assert DC.rel_l2(x.grad, x64.grad) < 1e-6


def test_fir_adjoint_of_the_down_sampling_layers(P, monkeypatch):
    """ops.fir's backward (ops._upfirdn2d_adjoint) against autograd: first the two FIR calls of a down-sampling layer at 8 x 8, on
    seeded draws, against binary32 autograd of the stand-in; then every case of tests/resample_cases.py — asymmetric and non-square
    filters, odd sizes, up and down together, unequal and negative padding, flip_filter — on the case's own inputs against float64
    autograd under the project's gate (its scale is the sum of the |terms|, so a one-element gradient whose terms cancel is judged by
    what binary32 can deliver, which a relative L2 bound is not)."""
    import resample_cases as RC
    from synthesis_grad_ref import gate
    DC.install_ops(monkeypatch, P.ops)
    f = P.ops.setup_filter([1, 3, 3, 1])
    gen = torch.Generator().manual_seed(4)
    for kw in (dict(padding=[2, 2, 2, 2]), dict(down=2, padding=[1, 1, 1, 1])):
        x = torch.randn(2, 3, 8, 8, generator=gen, requires_grad=True)
        y = P.ops.fir(x, f, **kw)
        g = torch.randn(y.shape, generator=gen)
        y.backward(g)
        x2 = x.detach().clone().requires_grad_(True)
        DC.upfirdn2d_torch(x2, f, **kw).backward(g)
        assert DC.rel_l2(x.grad, x2.grad) < 1e-6, kw
    for c in RC.CASES:
        x, fc, g = RC.make_inputs(c)
        ref = RC.case_ref(c)
        xg = x.clone().requires_grad_(True)
        P.ops.fir(xg, fc, **RC.kwargs(c)).backward(g)
        assert xg.grad.shape == ref["gx"].shape, c.id
        gate(f"{c.id} ops.fir backward", xg.grad, ref["gx"], ref["gx_absref"], ref["K"])


# ---- the layer gates and their sensitivity --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sorted(DC.CONV_SHAPES))
@pytest.mark.parametrize("variant", sorted(DC.CONV_VARIANTS))
def test_conv_layer_wiring_passes_the_gate(P, monkeypatch, shape, variant):
    """ops.conv2d_act under autograd on the stand-ins: what the GPU test runs on the kernels."""
    DC.install_ops(monkeypatch, P.ops)
    c = DC.conv_case(shape, variant)
    ref = DC.conv_layer_f64(*DC.conv_case_args(c))
    assert DC.layer_gate(DC.run_conv_layer(P.ops, c, "cpu"), ref) == []
    if c["clamp"] is not None:
        assert float((ref["pre"].abs() >= DC.R.f32(c["clamp"]) - 1e-12).double().mean()) > 0.05, "the clamp does not bite"


def test_layer_gate_fails_seeded_faults():
    for shape, variant, fault, where in (("conv0", "bias_lrelu", "tap", "out"), ("fromrgb", "plain", "tap", "out"), ("conv0", "clamp", "unflipped", "gx"),
                                         ("conv1", "residual", "unflipped", "gx"), ("conv0", "residual", "mask", "gx"), ("conv1", "residual", "mask", "gwk")):
        c = DC.conv_case(shape, variant)
        ref = DC.conv_layer_f64(*DC.conv_case_args(c))
        assert DC.layer_gate(DC.conv_layer_f32(*DC.conv_case_args(c)), ref) == [], (shape, variant)
        bad = DC.layer_gate(DC.conv_layer_f32(*DC.conv_case_args(c), fault=fault), ref, verbose=f"[{fault}] ")
        assert where in bad, (shape, variant, fault, bad)


@pytest.mark.parametrize("name", sorted(DC.MBSTD_SHAPES))
def test_mbstd_wiring_and_gate(P, monkeypatch, name):
    DC.install_ops(monkeypatch, P.ops)
    c = DC.mbstd_case(name)
    ref = DC.mbstd_f64(c)
    x = c["x"].clone().requires_grad_(True)
    y = P.ops.minibatch_std(x, c["group"], c["F"])
    with torch.no_grad():
        assert torch.equal(y.detach(), P.ops.minibatch_std(x.detach(), c["group"], c["F"]))
    y.backward(c["gy"])
    assert DC.mbstd_gate(dict(y=y.detach(), gx=x.grad), ref, c) == []
    assert DC.mbstd_gate(DC.mbstd_f32(c), ref, c) == []
    if c["x"].shape[0] > min(c["group"], c["x"].shape[0]):  # more than one group: the mean over the wrong axis is another number
        assert DC.mbstd_gate(DC.mbstd_f32(c, fault="axis"), ref, c) != []
