"""CPU (-m "not gpu"): the mapping network under autograd with the device operators replaced by torch stand-ins
(tests/train_step_cases.py) — the host wiring of FullyConnectedLayer / MappingNetwork / TriPlaneGenerator.mapping_zplus against the
reference's own fp32 autograd (tests/golden/mapping_grad.npz) and a float64 restatement, update_emas, and the memo layer around it.
On the parent commit MappingNetwork.forward asserts `not update_emas` and every mapping parameter's gradient is None."""
import pytest
import torch

import train_step_cases as TC


@pytest.fixture(scope="module")
def P():
    import panic3d_amd
    panic3d_amd.build()
    return panic3d_amd


@pytest.mark.parametrize("L", TC.MAPPING_LAYERS)
def test_mapping_grad_vs_reference(P, monkeypatch, L):
    TC.install_mapping_ops(monkeypatch, P.ops)
    TC.mapping_against_fixture(P, "cpu", L)


def test_mapping_grad_bits_and_memo(P, monkeypatch):
    TC.install_mapping_ops(monkeypatch, P.ops)
    TC.mapping_bits_and_memo(P, "cpu")


def test_update_emas_reaches_the_backbone_through_every_entry(P, monkeypatch):
    """mapping / mapping_zplus / backbone.forward hand update_emas on: w_avg moves by exactly the reference's expression; without
    update_emas, or with w_avg_beta None, it stays."""
    TC.install_mapping_ops(monkeypatch, P.ops)
    from panic3d_amd.generator import TriPlaneGenerator
    G = TC.fill_mapping(TriPlaneGenerator(**TC.mapping_kw(2)).eval(), 9)
    mp = G.backbone.mapping
    inp = TC.mapping_inputs(G.backbone.num_ws, 10)
    cond = {"resnet_feats": inp["feats"]}
    before = mp.w_avg.clone()
    G.mapping(inp["zs"][:, 0], inp["c"], cond)
    assert torch.equal(mp.w_avg, before)
    with torch.no_grad():
        x = mp(inp["zs"][:, 0], inp["c"], cond)[:, 0]
    want = x.mean(0).lerp(before, mp.w_avg_beta)
    G.mapping(inp["zs"][:, 0], inp["c"], cond, update_emas=True)
    assert torch.equal(mp.w_avg, want) and not torch.equal(want, before)
    mp.w_avg_beta = None
    G.mapping(inp["zs"][:, 0], inp["c"], cond, update_emas=True)
    assert torch.equal(mp.w_avg, want)


def test_fully_connected_lrelu_backward_mask_comes_from_the_output(P, monkeypatch):
    """The lrelu layer's Function against torch autograd of the same formula, bias gradient = column sums; a 2-D input."""
    TC.install_mapping_ops(monkeypatch, P.ops)
    torch.manual_seed(3)
    fc = P.stylegan2.FullyConnectedLayer(24, 40, activation="lrelu", lr_multiplier=0.01)
    with torch.no_grad():
        fc.bias.copy_(torch.randn(40) * 20)
    x = torch.randn(5, 24, requires_grad=True)
    g = torch.randn(5, 40)
    y = fc(x)
    with torch.no_grad():
        assert torch.equal(y.detach(), fc(x.detach()))
    y.backward(g)
    x2 = x.detach().clone().requires_grad_(True)
    w, b = fc.weight.detach().clone().requires_grad_(True), fc.bias.detach().clone().requires_grad_(True)
    y2 = torch.nn.functional.leaky_relu(x2 @ (w * fc.weight_gain).t() + b * fc.bias_gain, 0.2) * (2 ** 0.5)
    y2.backward(g)
    for a, r in ((x.grad, x2.grad), (fc.weight.grad, w.grad), (fc.bias.grad, b.grad)):
        assert TC.rel_l2(a, r) < 1e-6
