"""CPU (-m "not gpu"): the R1 penalty without a device — the C ABI (include/p3d_r1.h, _lib.R1_SIGNATURES and the library's exports;
argument errors come back before any launch); the recorded backward of the dual discriminator (DualDiscriminator.set_r1_grad, ops.py's
_R1* Functions) and the loss's Dreg / Dboth on torch stand-ins of the device operators (tests/r1_cases.py) against the reference's own
run (tests/golden/r1.npz) and float64; the switch's default, the third differentiation, the recorded first gradient's bits; and the gates
that tests/test_hip_r1.py holds the kernels to, checked against seeded faults.  On the parent commit the switch, the operators and the
symbols do not exist."""
import os
import re

import pytest
import torch

import discriminator_cases as DC
import loss_cases as LC
import p3d_testing as T
import r1_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def P():
    import panic3d_amd
    panic3d_amd.build()
    return panic3d_amd


@pytest.fixture(scope="module")
def golden():
    return T.load_golden("r1.npz")


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_r1_header_table_and_exports_agree(P):
    hdr = open(os.path.join(ROOT, "include", "p3d_r1.h")).read()
    declared = set(re.findall(r"\b(p3d_[a-z0-9_]+)\s*\(", hdr))
    lib = P._lib
    assert declared == set(lib.R1_SIGNATURES) and len(declared) == 3
    for name in dir(lib):
        if name.endswith("SIGNATURES") and name != "R1_SIGNATURES":
            assert not declared & set(getattr(lib, name)), name
    L = lib.lib()
    for name in declared:
        assert hasattr(L, name)
    assert "p3d_r1.hip" in P._build.SOURCES and os.path.join("..", "..", "include", "p3d_r1.h") in P._build.HEADERS
    assert "p3d_r1.hip" not in P._build.SYNTHESIS_UNIT and "p3d_r1.hip" not in P._build.RENDER_UNIT
    disc = open(os.path.join(ROOT, "include", "p3d_discriminator.h")).read()
    assert not any(name in disc for name in declared), "the R1 symbols belong to p3d_r1.h alone"


def test_r1_argument_errors_without_gpu(P):
    L = P._lib.lib()
    p = 256  # never dereferenced: the checks come first
    mask = lambda h=p, wk=p, pre=p, out=p, N=1, Ci=4, Hi=5, Wi=5, taps=9, Co=3, Ho=5, Wo=5, stride=1, pad=1, act=1: \
        L.p3d_conv2d_mask_f32(h, N, Ci, Hi, Wi, wk, taps, Co, Ho, Wo, stride, pad, pre, act, 0.2, 1.0, -1.0, out, None)
    assert mask(h=None) == -1 and mask(wk=None) == -1 and mask(pre=None) == -1 and mask(out=None) == -1 and mask(N=0) == -1 and mask(Co=0) == -1
    assert mask(taps=4) == -2 and mask(stride=3) == -2 and mask(pad=3) == -2 and mask(act=2) == -2 and mask(Ho=4) == -2
    assert mask(stride=2, pad=0, Ho=3, Wo=3) == -2  # (5 - 3) / 2 + 1 = 2
    mb = lambda x=p, ge=p, h=p, gg=p, gx=p, N=4, C=4, HW=16, group=2, F=1, stride=16: \
        L.p3d_mbstd_backward2_f32(x, ge, stride, h, N, C, HW, group, F, gg, gx, None)
    assert mb(x=None) == -1 and mb(ge=None) == -1 and mb(h=None) == -1 and mb(gg=None) == -1 and mb(gx=None) == -1 and mb(N=0) == -1 and mb(F=0) == -1
    assert mb(N=6, group=4) == -2 and mb(C=5, F=2) == -2 and mb(stride=15) == -2 and mb(HW=1 << 40) == -2
    ss = lambda a=p, b=p, out=p, Ea=10, Eb=10, N=2: L.p3d_r1_sumsq_f32(a, Ea, b, Eb, N, out, None)
    assert ss(a=None) == -1 and ss(out=None) == -1 and ss(N=0) == -1 and ss(Ea=0) == -1 and ss(b=None) == -1 and ss(Eb=0) == -1 and ss(Eb=-1) == -1
    assert ss(Ea=1 << 40) == -2 and ss(Eb=1 << 40) == -2


# ---- the switch -------------------------------------------------------------------------------------------------------------------------
def _grad_call(D, inp):
    image, raw = (inp[k].clone().requires_grad_(True) for k in ("image", "image_raw"))
    logits = D({"image": image, "image_raw": raw}, inp["c"].clone(), {"resnet_feats": inp["feats"]})
    return logits, image, raw


def test_switch_reaches_every_layer_and_defaults_off(P, monkeypatch):
    RC.install_ops(monkeypatch, P.ops)
    D = DC.fill_discriminator(P.DualDiscriminator(**DC.D_KW))
    layers = [m for m in D.modules() if isinstance(m, (P.discriminator.Conv2dLayer, P.discriminator.MinibatchStdLayer))]
    assert len(layers) == 3 * 3 + 1 + 1 + 1 and D.r1_grad is False and not any(m.r1_grad for m in layers)
    inp = DC.discriminator_inputs()
    logits, image, raw = _grad_call(D, inp)
    with pytest.raises(RuntimeError) as e:
        torch.autograd.grad([logits.sum()], [image, raw], create_graph=True, only_inputs=True)
    assert str(e.value) == P.ops.R1_MESSAGE
    assert D.set_r1_grad() is True and D.r1_grad is True and all(m.r1_grad for m in layers) and D.b4.fc.r1_grad is True
    assert set(D.state_dict()) == set(DC.fill_discriminator(P.DualDiscriminator(**DC.D_KW)).state_dict())
    logits2, image, raw = _grad_call(D, inp)
    assert torch.equal(logits2.detach(), logits.detach())
    g = torch.autograd.grad([logits2.sum()], [image, raw], create_graph=True, only_inputs=True)
    assert all(t.grad_fn is not None for t in g)
    assert D.set_r1_grad(False) is False and not any(m.r1_grad for m in layers) and D.b4.fc.r1_grad is False
    logits3, image, raw = _grad_call(D, inp)
    with pytest.raises(RuntimeError, match="R1"):
        torch.autograd.grad([logits3.sum()], [image, raw], create_graph=True, only_inputs=True)


def test_recorded_first_gradient_is_the_plain_one_bit_for_bit(P, monkeypatch):
    """Images and every parameter: the recorded pass (outside no_weight_gradients it also returns the parameters' first-order
    gradients) against logits.sum().backward() with the switch off."""
    RC.install_ops(monkeypatch, P.ops)
    D = DC.fill_discriminator(P.DualDiscriminator(**DC.D_KW))
    inp = DC.discriminator_inputs()
    logits, image, raw = _grad_call(D, inp)
    logits.sum().backward()
    plain = [image.grad, raw.grad] + [p.grad for p in D.parameters()]
    D.set_r1_grad(True)
    logits, image, raw = _grad_call(D, inp)
    rec = torch.autograd.grad([logits.sum()], [image, raw] + list(D.parameters()), create_graph=True)
    assert len(plain) == len(rec) and all(torch.equal(a, b.detach()) for a, b in zip(plain, rec))
    logits, image, raw = _grad_call(D, inp)  # and a plain backward with the switch on is today's code
    logits.sum().backward()
    assert torch.equal(image.grad, plain[0]) and torch.equal(raw.grad, plain[1])


def test_third_differentiation_raises(P, monkeypatch):
    RC.install_ops(monkeypatch, P.ops)
    D = DC.fill_discriminator(P.DualDiscriminator(**DC.D_KW))
    D.set_r1_grad(True)
    logits, image, raw = _grad_call(D, DC.discriminator_inputs())
    g_image, g_raw = torch.autograd.grad([logits.sum()], [image, raw], create_graph=True, only_inputs=True)
    pen = P.ops.r1_penalty(g_image, g_raw).sum()
    with pytest.raises(RuntimeError) as e:
        torch.autograd.grad([pen], [D.b16.conv0.weight], create_graph=True)
    assert str(e.value) == P.ops.R1_THIRD_ORDER_MESSAGE and "third" in str(e.value)
    for c in (RC.mbstd2_case("two_stats"),):
        x = c["x"].clone().requires_grad_(True)
        y = P.ops.minibatch_std(x, c["group"], c["F"], r1=True)
        gx, = torch.autograd.grad([y], [x], [c["gy"]], create_graph=True)
        with pytest.raises(RuntimeError, match="third"):
            torch.autograd.grad([(gx * c["h"]).sum()], [x], create_graph=True)


# ---- the network against the reference's own run -------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", sorted(RC.SCALES))
def test_network_vs_reference(P, monkeypatch, golden, tag):
    RC.install_ops(monkeypatch, P.ops)
    ratios = RC.network_against_fixture(P, "cpu", tag, golden)
    names = golden[f"{tag}|names"].tolist()
    assert "b4.out.bias" not in names and {"b4.conv.bias", "b4.fc.bias"} <= set(names)
    assert ratios["b4.conv.bias"] == 0.0 and ratios["b4.fc.bias"] == 0.0
    assert float(golden[f"{tag}|n|b4.conv.bias"]) == 0.0 and float(golden[f"{tag}|n|b4.fc.bias"]) == 0.0


def test_network_gate_fails_without_the_mbstd_second_order_path(P, monkeypatch, golden):
    """Seeded fault: mbstd_backward2 returns zeros.  The biases below the layer then get no R1 gradient at all, which the gate relative
    to the reference's own error notices at scale 1."""
    RC.install_ops(monkeypatch, P.ops)
    monkeypatch.setattr(P.ops, "mbstd_backward2", lambda x, gy, h, G, Fc: (torch.zeros_like(gy[:, x.shape[1]:]), torch.zeros_like(x)))
    with pytest.raises(AssertionError, match="bias"):
        RC.network_against_fixture(P, "cpu", "s1", golden)


# ---- the loss ---------------------------------------------------------------------------------------------------------------------------
def _capture(P):
    def capture(hook):
        P.loss.report = hook
    return capture


@pytest.mark.parametrize("name", sorted(RC.PHASE_CASES))
def test_loss_phase_vs_reference(P, monkeypatch, golden, name):
    """Dreg / Dboth of this package's loss on LC's stand-ins (StandInD carrying r1_grad = True) against the reference's own run."""
    LC.install_ops(monkeypatch, P.ops)
    RC.install_ops(monkeypatch, P.ops)
    monkeypatch.setattr(LC.StandInD, "r1_grad", True, raising=False)
    monkeypatch.setattr(P.loss, "report", P.loss.report)
    reports, grads = LC.run_phase(P.StyleGAN2LossOrthoCondA, RC.PHASE_CASES[name], _capture(P))
    assert "Loss/r1_penalty" in reports and "Loss/D/reg" in reports
    LC.compare_with_fixture(golden, name, reports, grads)


def test_loss_still_raises_with_the_switch_off(P, monkeypatch, golden):
    LC.install_ops(monkeypatch, P.ops)
    RC.install_ops(monkeypatch, P.ops)
    monkeypatch.setattr(P.loss, "report", P.loss.report)
    assert not hasattr(LC.StandInD, "r1_grad")
    for name in ("Dreg-s10", "Dboth-s1.5"):
        with pytest.raises(RuntimeError) as e:
            LC.run_phase(P.StyleGAN2LossOrthoCondA, RC.PHASE_CASES[name], _capture(P))
        assert str(e.value) == P.ops.R1_MESSAGE
    assert "R1" in P.StyleGAN2LossOrthoCondA.__doc__ and "set_r1_grad" in P.StyleGAN2LossOrthoCondA.__doc__


def test_r1_penalty_and_its_gradient(P, monkeypatch):
    RC.install_ops(monkeypatch, P.ops)
    g = torch.Generator().manual_seed(5)
    a, b = torch.randn(3, 2, 5, 7, generator=g, requires_grad=True), torch.randn(3, 2, 3, 3, generator=g, requires_grad=True)
    cot = torch.randn(3, generator=g)
    for args in ((a, b), (a,)):
        a.grad = b.grad = None
        pen = P.ops.r1_penalty(*args)
        assert tuple(pen.shape) == (3,) and torch.allclose(pen, RC.sumsq_torch(*(t.detach() for t in args)))
        pen.backward(cot)
        assert torch.equal(a.grad, 2 * cot.view(3, 1, 1, 1) * a.detach())
        assert (b.grad is None) if len(args) == 1 else torch.equal(b.grad, 2 * cot.view(3, 1, 1, 1) * b.detach())
    with torch.no_grad():
        assert P.ops.r1_penalty(a, b).grad_fn is None


# ---- the single operators: wiring on the stand-ins, and the gates against seeded faults ------------------------------------------------
@pytest.mark.parametrize("name", sorted(RC.MBSTD2_SHAPES))
def test_mbstd_double_backward_wiring_and_gate(P, monkeypatch, name):
    RC.install_ops(monkeypatch, P.ops)
    c = RC.mbstd2_case(name)
    got = RC.run_mbstd2(P.ops, c, "cpu")
    gy0 = c["gy"].clone()
    gy0[:, :c["x"].shape[1]] = 0
    x = c["x"].clone().requires_grad_(True)
    P.ops.minibatch_std(x, c["group"], c["F"]).backward(gy0)
    assert torch.equal(got["first"], x.grad), "the recorded first gradient differs from the plain one"
    bad, _ = RC.mbstd2_gate(got, c)
    assert bad == []
    G = min(c["group"], c["x"].shape[0])
    fault = dict(zip(("g_extra", "gx"), RC.mbstd_backward2_torch(c["x"], gy0, c["h"], G, c["F"], fault="no_d_term")))
    bad, _ = RC.mbstd2_gate(fault, c, verbose="[no_d_term] ")
    assert "gx" in bad


@pytest.mark.parametrize("shape,variant", [("conv0", "clamp"), ("conv1", "residual"), ("fromrgb", "bias_lrelu"), ("epilogue", "linear_residual")])
def test_conv_layer_double_backward_wiring(P, monkeypatch, shape, variant):
    RC.install_ops(monkeypatch, P.ops)
    c = DC.conv_case(shape, variant)
    h = torch.randn(c["x"].shape, generator=torch.Generator().manual_seed(9))
    ref = RC.conv_layer2_f64(c, h)
    got = RC.run_conv_layer2(P.ops, c, h, "cpu")
    plain = DC.run_conv_layer(P.ops, c, "cpu")
    assert torch.equal(got["gx"], plain["gx"]), "the recorded first gradient differs from the plain one"
    for k in ("gx", "g_gy", "g_wk"):
        e = DC.rel_l2(got[k], ref[k])
        print(f"{shape}/{variant} {k}: rel-L2 {e:.2e}")
        assert e <= DC.R.REL_L2, k
    assert (got["g_bias"] is None) == (c["bias"] is None)
    if c["bias"] is not None:
        assert not got["g_bias"].any() and not ref["g_bias"].any()


def test_mask_gate_fails_a_missing_mask():
    c = RC.mask_case("conv0", "clamp")
    args = (c["h"], c["wk"], c["pre"], c["act"], c["gain_value"], c["clamp"], c["stride"], c["pad"])
    ref, absref, K = RC.conv2d_mask_f64(*args)
    assert DC.R.gate_ratio(RC.conv2d_mask_impl_torch(*args), ref, absref, K) <= DC.R.GATE_C
    assert DC.R.gate_ratio(RC.conv2d_mask_impl_torch(*args, fault="nomask"), ref, absref, K) > DC.R.GATE_C
    assert float((ref == 0).double().mean()) > 0.05, "the clamp does not bite"


def test_fir_recorded_backward_is_linear_to_any_order(P, monkeypatch):
    """ops.fir(r1=True): the gradient of <fir'(g), h> with respect to g is fir(h) — the operator itself — for the down-sampling layers'
    two calls and the 'classic' resize's up-sampling call, and that gradient can be recorded once more."""
    RC.install_ops(monkeypatch, P.ops)
    f = P.ops.setup_filter([1, 3, 3, 1])
    gen = torch.Generator().manual_seed(4)
    for kw in (dict(padding=[2, 2, 2, 2]), dict(down=2, padding=[1, 1, 1, 1]), dict(up=2, padding=[2, 1, 2, 1], gain=4)):
        x = torch.randn(2, 3, 8, 8, generator=gen, requires_grad=True)
        y = P.ops.fir(x, f, r1=True, **kw)
        g = torch.randn(y.shape, generator=gen, requires_grad=True)
        h = torch.randn(x.shape, generator=gen, requires_grad=True)
        gx, = torch.autograd.grad([y], [x], [g], create_graph=True)
        gg, = torch.autograd.grad([(gx * h).sum()], [g], create_graph=True)
        assert DC.rel_l2(gg.detach(), DC.upfirdn2d_torch(h.detach().double(), f.double(), **kw)) < 1e-6, kw
        gh, = torch.autograd.grad([(gg * y.detach()).sum()], [h])
        assert DC.rel_l2(gh, gx.detach() * 0 + torch.autograd.grad([P.ops.fir(x, f, **kw)], [x], [y.detach()])[0]) < 1e-6, kw
