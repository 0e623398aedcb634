"""CPU (-m "not gpu"): the grad-mode HOST wiring of the 512^2 super-resolution (SuperresolutionHybrid8XDC with record_grad: the
StylePlan under autograd, both blocks with the ToRGB layer riding on conv1, ops.torgb_combine given the layer's own inputs) with the
device operators replaced by their torch restatements (tests/p3d_torch_ops.py, extended here by the riding ToRGB), against the
reference's own fp32 autograd (tests/golden/sr_grad.npz, tests/golden/make_golden_superres_grad.py)."""
import pytest
import torch
import torch.nn.functional as F

import p3d_testing as T
import superres_grad_cases as SRC


@pytest.fixture(scope="module")
def P():
    import panic3d_amd
    panic3d_amd.build()
    return panic3d_amd


def _install(monkeypatch, ops, seen):
    import p3d_torch_ops
    p3d_torch_ops.install(monkeypatch, ops)
    base = ops.modulated_conv2d

    def modulated_conv2d(x, weight, styles, *a, rgb_weight=None, rgb_styles=None, want_y=True, **k):
        y = base(x, weight, styles, *a, **k)
        if rgb_weight is None:
            return y
        part = torch.einsum("ro,nohw->nrhw", rgb_weight, (y * rgb_styles[:, :, None, None]).detach())[None]
        return y, None, part

    def torgb_combine(partial, bias=None, clamp=None, skip=None, skip_filter=None, x=None, weight=None, styles=None):
        """networks_stylegan2.py:366-380 + :476-478 from the layer's own inputs when they are given, else from the shares."""
        seen.append(x is not None)
        v = F.conv2d(x * styles[:, :, None, None], weight) if x is not None else partial.sum(0)
        y = p3d_torch_ops.bias_act(v, bias, clamp=clamp)
        return y if skip is None else p3d_torch_ops.upsample2d(skip, skip_filter) + y
    monkeypatch.setattr(ops, "modulated_conv2d", modulated_conv2d)
    monkeypatch.setattr(ops, "torgb_combine", torgb_combine)


def test_superres_grad_host_logic_vs_reference(P, monkeypatch):
    """Every gradient — rgb, the feature image, ws, every parameter of both blocks incl. the affine layers, the ToRGB layers that ride
    on conv1 and the noise strengths — against the reference's fp32 autograd at relative L2 1e-4.  Without the recorded backward the
    module returns an image without grad_fn and no parameter gets a gradient."""
    seen = []
    _install(monkeypatch, P.ops, seen)
    g = T.load_golden("sr_grad.npz")
    sr = SRC.fill(P.generator.SuperresolutionHybrid8XDC(**SRC.SR_KW)).eval()
    rgb, x, ws, g_out, chk = SRC.draws()
    assert abs(chk - float(g["draw_checksum"][0])) < 1e-6 * abs(chk), "the fixture's draws could not be reproduced"
    for t in (rgb, x, ws):
        t.requires_grad_(True)
    sr.record_grad = True
    out = sr(rgb, x, ws, noise_mode="const")
    assert out.grad_fn is not None
    assert seen == [True, True]  # both ToRGB layers rode on conv1 and were recorded from their own inputs
    assert SRC.rel_l2(out.detach()[:, :, ::8, ::8].numpy(), g["out_sub"]) < 1e-4
    (out * g_out).sum().backward()
    SRC.check_against_fixture(sr, rgb, x, ws, g)


def test_superres_records_only_when_switched_on_and_autograd_records(P):
    """The default stays inference-only: the module records a backward only with record_grad set, grad enabled and an input or
    parameter requiring grad."""
    sr = P.generator.SuperresolutionHybrid8XDC(**dict(SRC.SR_KW, channels_hidden=64))
    rgb, x, ws, _, _ = SRC.draws()
    assert not sr._records_grad(rgb, x.requires_grad_(True), ws)
    sr.record_grad = True
    assert sr._records_grad(rgb, x, ws)
    with torch.no_grad():
        assert not sr._records_grad(rgb, x, ws)
    x.requires_grad_(False)
    for p in sr.parameters():
        p.requires_grad_(False)
    assert not sr._records_grad(rgb, x, ws) and sr._records_grad(rgb, x, ws.requires_grad_(True))
