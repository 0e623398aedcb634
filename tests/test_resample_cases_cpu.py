"""CPU (-m "not gpu"): the designed cases of the generic resampler and its adjoint (tests/resample_cases.py).  ops._upfirdn2d_adjoint —
the padding, the exchanged factors and the `not flip_filter` of the backward of ops.fir, ops.upsample2d and the ToRGB skip — on the
float64 stand-in against float64 autograd at every case; binary32 torch passes the gate; six seeded faults fail the case named for each.
tests/test_hip_resample_edges.py applies the same reference and gate to k_upfirdn2d."""
import pytest
import torch

import discriminator_cases as DC
import resample_cases as RC
from synthesis_grad_ref import GATE_C, gate, gate_passes, gate_ratio


@pytest.fixture(scope="module")
def P():
    import panic3d_amd
    panic3d_amd.build()
    return panic3d_amd


def test_cases_keep_their_coverage():
    C = RC.CASES
    assert len(C) >= 15 and len(set(RC.CASE_IDS)) == len(C)
    assert {c.filt for c in C} == {"sym", "asym", "f3x5"}
    for filt in ("asym", "f3x5"):
        mine = [c for c in C if c.filt == filt]
        assert any(c.up > 1 for c in mine) and any(c.down > 1 for c in mine) and any(c.flip for c in mine), filt
        f = RC.make_filter(filt)
        assert not torch.equal(f, f.flip([0])) and not torch.equal(f, f.flip([1])) and not torch.equal(f, f.flip([0, 1]))
        assert tuple(f.shape) != (4, 4) or not torch.equal(f, f.t())
    assert any(min(DC._pad4(c.padding)) < 0 for c in C)
    assert any(DC._pad4(c.padding)[:2] != DC._pad4(c.padding)[2:] for c in C)
    assert any(c.up > 1 and c.down > 1 and c.up != c.down for c in C)
    n = [c.shape[0] * c.shape[1] * RC.out_hw(c)[0] * RC.out_hw(c)[1] for c in C]
    assert any(v > 256 and v % 256 for v in n) and 1 in n
    assert all(min(RC.out_hw(c)) >= 1 for c in C)
    assert set(RC.FAULT_CASE) == set(RC.FAULTS) and set(RC.FAULT_CASE.values()) <= set(RC.CASE_IDS)


@pytest.mark.parametrize("ci", range(len(RC.CASES)), ids=RC.CASE_IDS)
def test_adjoint_formula_and_binary32_gate(P, monkeypatch, ci):
    DC.install_ops(monkeypatch, P.ops)
    c = RC.CASES[ci]
    x, f, g = RC.make_inputs(c)
    ref = RC.case_ref(c)
    assert tuple(ref["y"].shape[2:]) == RC.out_hw(c)
    # float64 on the stand-in: the formula itself, to rounding (16 to 15 float64 terms per value)
    gx64 = P.ops._upfirdn2d_adjoint(g.double(), f.double(), c.up, c.down, c.padding, c.flip, c.gain, tuple(c.shape[2:]))
    assert gx64.shape == ref["gx"].shape
    assert float((gx64 - ref["gx"]).abs().max()) <= 1e-13 * max(1.0, float(ref["gx_absref"].max())), c.id
    # binary32: the forward and the adjoint pass the gate
    gate(f"{c.id} forward binary32", RC.forward_f32(c), ref["y"], ref["absref"], ref["K"])
    gate(f"{c.id} adjoint binary32", RC.adjoint_f32(P.ops, c), ref["gx"], ref["gx_absref"], ref["K"])
    # ... and ops.fir under autograd is that adjoint
    xg = x.clone().requires_grad_(True)
    P.ops.fir(xg, f, **RC.kwargs(c)).backward(g)
    assert torch.equal(xg.grad, RC.adjoint_f32(P.ops, c))


@pytest.mark.parametrize("fault", RC.FAULTS)
def test_gate_fails_seeded_faults(P, monkeypatch, fault):
    DC.install_ops(monkeypatch, P.ops)
    c = RC.BY_ID[RC.FAULT_CASE[fault]]
    ref = RC.case_ref(c)
    if fault == "adjoint_up_down_swapped":
        bad, want, ab = RC.overlap(RC.adjoint_f32(P.ops, c, fault), ref["gx"]), ref["gx"], ref["gx_absref"]
    else:
        bad, want, ab = RC.overlap(RC.forward_f32(c, fault), ref["y"]), ref["y"], ref["absref"]
    r = gate_ratio(bad, want, ab, ref["K"])
    print(f"{fault} on {c.id}: worst ratio {r:.3g} against {GATE_C:g}")
    assert r > GATE_C and not gate_passes(bad, want, ab, ref["K"])
    if fault in ("no_flip", "flip_one_axis", "pad_xy_swapped"):
        # what the symmetric [1,3,3,1] filter and equal x / y padding cannot show: the same fault is invisible there
        s = RC.BY_ID["16-sym-down2"]
        assert gate_passes(RC.forward_f32(s, fault), RC.case_ref(s)["y"], RC.case_ref(s)["absref"], RC.case_ref(s)["K"])
