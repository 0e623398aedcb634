"""CPU (-m "not gpu"): the synthesis backward's C ABI (include/p3d_synthesis_grad.h, _lib.SYN_GRAD_SIGNATURES and the library's
exports agree; argument errors come back before any launch), and the grad-mode HOST wiring of the synthesis network (StylePlan's
recorded styles / demodulation, noise, out-of-place conditioning, injections, stop_level) with the operators replaced by their torch
restatements (tests/p3d_torch_ops.py), against the reference's own autograd (tests/golden/syn_grad_*.npz)."""
import ctypes as C
import os
import re

import pytest
import torch

import synthesis_grad_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def P():
    import panic3d_amd
    panic3d_amd.build()
    return panic3d_amd


def test_syn_grad_header_table_and_exports_agree(P):
    hdr = open(os.path.join(ROOT, "include", "p3d_synthesis_grad.h")).read()
    declared = set(re.findall(r"\b(p3d_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(P._lib.SYN_GRAD_SIGNATURES), "include/p3d_synthesis_grad.h and _lib.SYN_GRAD_SIGNATURES disagree"
    assert not declared & (set(P._lib.SIGNATURES) | set(P._lib.GRAD_SIGNATURES))
    L = P._lib.lib()
    for name in declared:
        assert hasattr(L, name)
    assert "p3d_synthesis_grad.hip" in P._build.SOURCES
    # the forward's translation units are not touched by the backward
    assert "p3d_synthesis_grad.hip" not in P._build.SYNTHESIS_UNIT and "p3d_synthesis_grad.hip" not in P._build.RENDER_UNIT


def test_syn_grad_argument_errors_without_gpu(P):
    L = P._lib.lib()
    f = C.c_void_p(256)  # never dereferenced: the checks come first
    assert L.p3d_bias_act_backward_f32(None, f, 1, 8, 16, 1, 0.2, 1.4, -1.0, None, f, None, None, None) == -1
    assert L.p3d_bias_act_backward_f32(f, f, 1, 0, 16, 1, 0.2, 1.4, -1.0, None, f, None, None, None) == -1
    assert L.p3d_bias_act_backward_f32(f, f, 1, 8, 16, 2, 0.2, 1.4, -1.0, None, f, None, None, None) == -2  # unknown activation
    assert L.p3d_conv_dgrad_f32(f, 1, 8, 4, 4, None, 9, 8, 4, 4, 1, 1, f, None) == -1
    assert L.p3d_conv_dgrad_f32(f, 1, 8, 4, 4, f, 4, 8, 4, 4, 1, 1, f, None) == -2  # taps
    assert L.p3d_conv_dgrad_f32(f, 1, 8, 4, 4, f, 9, 8, 4, 4, 3, 1, f, None) == -2  # stride
    assert L.p3d_mod_backward_f32(f, None, 1, 8, 16, f, f, None) == -1
    assert L.p3d_conv_wgrad_workspace_bytes(0, 8, 8, 9, 4, 4) == 0
    assert L.p3d_conv_wgrad_workspace_bytes(1, 8, 8, 4, 4, 4) == 0
    wsb = L.p3d_conv_wgrad_workspace_bytes(2, 64, 64, 9, 16, 16)
    assert wsb >= 2 * 9 * 64 * 64 * 4 * 2 and wsb % 256 == 0
    ws = C.c_void_p(4096)
    args = [f, 16, 16, 1, 0, 0, f, f, 16, 16, 1, 1, 1, 2, 64, 64, 9, 16, 16, f, None, None, None, ws, wsb, None]

    def call(**kw):
        a = list(args)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return L.p3d_conv_wgrad_f32(*a)
    assert call(a0=None) == -1           # g
    assert call(a19=None) == -1          # dw
    assert call(a22=f) == -1             # g_d without wk / dscale
    assert call(a23=None) == -1          # workspace
    assert call(a23=C.c_void_p(4100)) == -1  # unaligned workspace
    assert call(a24=16) == -3            # workspace too small
    assert call(a16=4) == -2             # taps
    assert call(a3=3) == -2              # stride


@pytest.mark.parametrize("tag", ["none", "cond"])
def test_synthesis_grad_host_logic_vs_reference(P, monkeypatch, tag):
    """SynthesisNetwork.forward under autograd on CPU with the torch restatements of the operators: every gradient (ws, every
    synthesis parameter incl. the affine layers and noise strengths, the injections, the conditioning images) against the reference's
    fp32 autograd.  Without the recorded StylePlan / noise / conditioning, the affine and noise-strength gradients are missing."""
    import p3d_torch_ops
    p3d_torch_ops.install(monkeypatch, P.ops)
    G, net, ws, cond, inj, g_out, sl, g = SC.build(P, tag, "cpu")
    out = net(ws, cond, latent_injection=inj, stop_level=sl, noise_mode="const")
    assert out.grad_fn is not None
    assert SC.rel_l2(out.detach()[:, ::8, ::4, ::4].numpy(), g["out_sub"]) < 1e-4
    (out * g_out).sum().backward()
    SC.check_against_fixture(net, ws, cond, inj, g)


def test_synthesis_no_grad_call_unchanged_after_grad_call(P, monkeypatch):
    """A grad-mode call leaves no recorded tensor in the caches a no-grad call reads: the no-grad call after it gives the cold bits."""
    import p3d_torch_ops
    p3d_torch_ops.install(monkeypatch, P.ops)
    G, net, ws, cond, inj, g_out, sl, g = SC.build(P, "cond", "cpu")
    with torch.no_grad():
        cold = net(ws.detach(), cond, noise_mode="const").clone()
    out = net(ws, cond, noise_mode="const")
    assert torch.equal(out.detach(), cold)
    (out * g_out).sum().backward()
    with torch.no_grad():
        again = net(ws.detach(), cond, noise_mode="const")
    assert torch.equal(again, cold) and again.grad_fn is None
