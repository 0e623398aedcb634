"""CPU (-m "not gpu"): the designed cases of the stand-alone ToRGB GEMM (tests/torgb_cases.py) and the host-side plan of its launch
(csrc/p3d_torgb_plan.hpp, compiled alone into tests/torgb_plan_host.cpp).  (1) The plan reproduces the launches recorded from
p3d_torgb_f32's own dispatch before the plan existed (tests/golden/torgb_plans.json, written by tests/golden/make_golden_torgb_plans.py:
N, I, O, H, W, then the P3D_E_* code or the instantiation, the grid and the dynamic LDS bytes).  (2) Every case reaches the instantiation it names and the list keeps its coverage
conditions.  (3) The float64 reference equals float64 torch; binary32 torch passes the gate in three summation orders; every seeded
fault fails the case named for it.  tests/test_hip_torgb_edges.py applies the same reference and gate to the kernels."""
import json
import os
import subprocess

import pytest
import torch

import discriminator_cases as DC
import torgb_cases as TC
from host_build import ROOT, compile_host
from synthesis_grad_ref import GATE_C, gate, gate_passes, gate_ratio


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return compile_host(tmp_path_factory.mktemp("torgb_plan"), "torgb_plan_host.cpp")


def _plans(exe, shapes):
    res = subprocess.run([exe], input="".join("p %d %d %d %d %d\n" % tuple(s) for s in shapes), capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-4000:]
    out = [l.split() for l in res.stdout.splitlines()]
    assert len(out) == len(shapes)
    return [[int(f[1])] if f[0] == "err" else [f[0]] + [int(v) for v in f[1:]] for f in out]


def test_plan_reproduces_the_recorded_launches(host):
    with open(os.path.join(ROOT, "tests", "golden", "torgb_plans.json")) as f:
        rows = json.load(f)
    assert len(rows) > 5000 and {r[5] for r in rows if len(r) == 6} == {-1, -2}
    assert {r[5] for r in rows if len(r) > 6} == set(TC.KERNELS)
    for r, got in zip(rows, _plans(host, [r[:5] for r in rows])):
        assert got == r[5:], r[:5]


def test_every_case_reaches_the_instantiation_it_names(host):
    assert len(set(TC.CASE_IDS)) == len(TC.CASES)
    for c, got in zip(TC.CASES, _plans(host, [(c.N, c.I, c.O, c.H, c.W) for c in TC.CASES])):
        assert got[0] == c.kernel, (c.id, got)
        px, ks = TC.tiles(c)
        # the rule as the issue states it, next to the plan
        want = (TC.PX1 if px >= 512 else TC.KS1) if c.O <= 32 else TC.PX3 if px >= 512 else TC.KS3 if 3 * ks > 1024 else TC.MS if c.I > 512 else TC.PRE
        assert want == c.kernel, c.id
        assert c.filt is None or (c.H % 2 == 0 and c.W % 2 == 0), c.id
        assert c.N * c.I * c.H * c.W * 4 <= 36 << 20, c.id  # the largest x: about 35 MB


def test_cases_keep_their_coverage():
    C = TC.CASES
    for k in TC.KERNELS:
        mine = [c for c in C if c.kernel == k]
        assert {c.filt is not None for c in mine} == {True, False}, k
        assert {c.bias for c in mine} == {True, False}, k
        assert {c.clamp is not None for c in mine} == {True, False}, k
        assert any(c.clamp is not None and TC.case_ref(c)["clipped"] > 0.10 for c in mine), k
    Is, Os = {c.I for c in C}, {c.O for c in C}
    assert {1, 64, 65, 512, 513, 1024} <= Is and any(i % 2 for i in Is)
    chunks = {-(-i // 64) for i in Is}
    assert any(n >= 3 and n % 2 for n in chunks) and any(n >= 3 and n % 2 == 0 for n in chunks)
    assert {1, 3, 32, 33, 40, 96} <= Os
    assert any(c.H != c.W for c in C)
    ks = [c for c in C if c.kernel not in (TC.PX1, TC.PX3)]
    assert any((c.H * c.W) % 32 for c in ks)
    for k in (TC.PX1, TC.PX3):
        px = [c for c in C if c.kernel == k]
        assert all((c.H * c.W) % 128 for c in px), k
        assert any(c.filt for c in px) and any(TC.tiles(c)[0] == 512 for c in px), k
    assert sum(c.N == 1 for c in C) == 1
    assert {511, 512} <= {TC.tiles(c)[0] for c in C}
    assert {1023, 1026} <= {3 * TC.tiles(c)[1] for c in C if c.O > 32}  # 3 * KS tiles is a multiple of 3: the two sides of 1024
    assert set(TC.FAULT_CASE) == set(TC.FAULTS) and set(TC.FAULT_CASE.values()) <= set(TC.CASE_IDS)
    assert {"sym", "asym"} <= {c.filt for c in C}


@pytest.mark.parametrize("ci", range(len(TC.CASES)), ids=TC.CASE_IDS)
def test_reference_is_float64_torch_and_binary32_passes_the_gate(ci):
    c = TC.CASES[ci]
    t, ref = TC.make_inputs(c), TC.case_ref(c)
    # float64: per-sample weights through torch's conv2d, the skip image through the restated upfirdn2d (no code shared with the reference)
    ww = t["w"].double()[None] * t["s"].double()[:, None, :]
    v = torch.cat([torch.nn.functional.conv2d(t["x"][n:n + 1].double(), ww[n][:, :, None, None]) for n in range(c.N)])
    if c.bias:
        v = v + t["bias"].double()[None, :, None, None]
    if c.clamp is not None:
        v = v.clamp(-TC.f32(c.clamp), TC.f32(c.clamp))
    if c.filt:
        v = DC.upfirdn2d_torch(t["skip"].double(), t["f"].double(), up=2, padding=[2, 1, 2, 1], gain=4) + v
    assert float((v - ref["y"]).abs().max()) <= 1e-12, c.id
    assert float((TC.case_torch(c, torch.float64) - ref["y"]).abs().max()) <= 1e-12, c.id
    assert float(ref["absref"].min()) > 0 and bool((ref["absref"] >= ref["y"].abs() - 1e-12).all())
    # binary32 in three orders: none of them the kernel's, all of them legitimate
    for order in ("plain", "modx", "quarters"):
        gate(f"{c.id} binary32 {order}", TC.case_torch(c, torch.float32, order), ref["y"], ref["absref"], ref["K"])


@pytest.mark.parametrize("fault", TC.FAULTS)
def test_gate_fails_seeded_faults(fault):
    c = TC.BY_ID[TC.FAULT_CASE[fault]]
    ref = TC.case_ref(c)
    for order in ("modx", "quarters"):
        bad = TC.case_torch(c, torch.float32, order, fault)
        r = gate_ratio(bad, ref["y"], ref["absref"], ref["K"])
        print(f"{fault} on {c.id} ({order}): worst ratio {r:.3g} against {GATE_C:g}")
        assert r > GATE_C and not gate_passes(bad, ref["y"], ref["absref"], ref["K"]), (fault, c.id, order)


def test_exact_where_the_scale_is_zero():
    """An element whose terms are all zero must be exact: a zero image with no bias passes, the smallest non-zero value there fails."""
    x, w, s = torch.zeros(2, 3, 2, 2), torch.randn(4, 3), torch.ones(2, 3)
    ref = TC.torgb_ref(x, w, s)
    assert float(ref["absref"].max()) == 0 and gate_passes(torch.zeros(2, 4, 2, 2), ref["y"], ref["absref"], ref["K"])
    bad = torch.zeros(2, 4, 2, 2)
    bad[1, 2, 1, 0] = 1e-30
    assert not gate_passes(bad, ref["y"], ref["absref"], ref["K"])
