"""CPU (-m "not gpu"): the front-view paste's backward without a device — its C ABI (include/p3d_paste_grad.h, _lib.PASTE_GRAD_SIGNATURES
and the library's exports agree; argument errors come back before any launch; the unit's ISA holds no compare-and-swap loop), the
float64 restatement the GPU test measures the kernel against (tests/train_step_cases.paste_backward_ref) checked against float64 torch
autograd of the reference's own composition, the gate's power to catch a dropped tap, swapped x / y channels and a missing border
zero, and the torch formulation (paste.paste_front_torch, the path of front_weight_erosion / force_image) against the reference's
paste_front under autograd (tests/golden/train_step.npz)."""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import p3d_testing as T
import train_step_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def P():
    import panic3d_amd
    panic3d_amd.build()
    return panic3d_amd


def test_paste_grad_header_table_and_exports_agree(P):
    hdr = open(os.path.join(ROOT, "include", "p3d_paste_grad.h")).read()
    declared = set(re.findall(r"\b(p3d_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(P._lib.PASTE_GRAD_SIGNATURES)
    assert not declared & (set(P._lib.SIGNATURES) | set(P._lib.GRAD_SIGNATURES) | set(P._lib.SYN_GRAD_SIGNATURES))
    L = P._lib.lib()
    for name in declared:
        assert hasattr(L, name)
    assert "p3d_paste_grad.hip" in P._build.SOURCES and os.path.join("..", "..", "include", "p3d_paste_grad.h") in P._build.HEADERS
    assert "p3d_paste_grad.hip" not in P._build.SYNTHESIS_UNIT and "p3d_paste_grad.hip" not in P._build.RENDER_UNIT
    fields = re.search(r"typedef struct p3d_paste_grad_args \{(.*?)\}", hdr, re.S).group(1)
    names = [n for line in fields.split("\n") for n in re.findall(r"(\w+)\s*[,;]", line.split("/*")[0])]
    assert names == [n for n, _ in P._lib.PasteGradArgs._fields_] and C.sizeof(P._lib.PasteGradArgs) == 112


def test_paste_grad_argument_errors_without_gpu(P):
    L = P._lib.lib()
    f = 256  # never dereferenced: the checks come first
    base = dict(g_out=f, g_paste=f, mask=f, xyz=f, front=f, g_image=f, g_xyz=f, g_front=f, workspace=4096, workspace_bytes=1 << 30, N=1, r=16, S=64,
                front_shared=0, normalize_images=0, grad_sample=1, box_warp=0.7)

    def call(**kw):
        return L.p3d_paste_front_backward_f32(C.byref(P._lib.PasteGradArgs(**dict(base, **kw))), None)
    assert L.p3d_paste_front_backward_f32(None, None) == -1
    assert call(mask=None) == -1 and call(g_out=None, g_paste=None) == -1
    assert call(g_image=None, g_xyz=None, g_front=None) == -1
    assert call(N=0) == -1 and call(r=0) == -1 and call(S=-4) == -1
    assert call(grad_sample=0) == -1 and call(xyz=None) == -1 and call(front=None, g_xyz=None) == -1
    assert call(workspace=None) == -1 and call(workspace=4100) == -1
    assert call(r=4097) == -2 and call(S=8193) == -2
    assert call(workspace_bytes=64) == -3
    assert L.p3d_paste_front_backward_workspace_bytes(0, 64) == 0 and L.p3d_paste_front_backward_workspace_bytes(2, 0) == 0
    w = L.p3d_paste_front_backward_workspace_bytes(3, 96)
    assert w >= 3 * 2 * 96 * 96 * 4 and w % 256 == 0


def test_paste_grad_unit_has_no_cas_loop_and_no_scalar_memory_writes(P, tmp_path):
    """The illustration's gradient accumulates with the hardware float add (global_atomic_add_f32), not a compare-and-swap loop."""
    flags = [f for f in P._build.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    asm = tmp_path / "p3d_paste_grad.s"
    subprocess.check_call([P._build._hipcc()] + flags + ["--cuda-device-only", "-S", os.path.join(P._build.CSRC, "p3d_paste_grad.hip"), "-o", str(asm)])
    text = asm.read_text().lower()
    assert "cmpswap" not in text and "global_atomic_add_f32" in text
    assert "k_paste_bwd_pixel" in text and "k_paste_bwd_xyz" in text


def _inputs(seed, N, r, S, shared, scale=0.25):
    g = torch.Generator().manual_seed(seed)
    xyz = torch.randn(N, 3, r, r, generator=g) * scale  # box_warp 0.7: |x| > 0.35 leaves the illustration -> clamped samples
    front = torch.rand(1 if shared else N, 3, S, S, generator=g)
    mask = (torch.rand(N, 1, S, S, generator=g) * 1.5).clamp_max(1.0) * (torch.rand(N, 1, S, S, generator=g) > 0.3)
    return xyz, front, mask, torch.randn(N, 3, S, S, generator=g), torch.randn(N, 3, S, S, generator=g)


@pytest.mark.parametrize("r,S,N,shared,norm", [(16, 64, 2, False, True), (37, 96, 2, True, False)])
def test_paste_reference_is_torch_autograd(r, S, N, shared, norm):
    """The term-by-term float64 restatement (coords='float64') IS float64 torch autograd of
    torch.lerp(image, sample_orthofront(tocopy, interpolate(xyz, S)), mask) plus the returned paste's cotangent."""
    from panic3d_amd import paste
    xyz, front, mask, g_out, g_paste = _inputs(5, N, r, S, shared)
    x64, f64 = xyz.double().requires_grad_(True), front.double().requires_grad_(True)
    img = torch.randn(N, 3, S, S, dtype=torch.float64, requires_grad=True)
    tocopy = (f64 * 2 - 1 if norm else f64).expand(N, -1, -1, -1)
    p = paste.sample_orthofront(tocopy, F.interpolate(x64, S, mode="bilinear"), 0.7)
    out = torch.lerp(img, p, mask.double())
    ((out * g_out.double()).sum() + (p * g_paste.double()).sum()).backward()
    ref = TC.paste_backward_ref(g_out, g_paste, mask, xyz, front, 0.7, norm, True, coords="float64")
    clamped = float((ref["g_xyz"][0][:, :2] == 0).double().mean())
    for name, want in (("g_image", img.grad), ("g_xyz", x64.grad), ("g_front", f64.grad)):
        assert TC.rel_l2(ref[name][0], want) < 1e-12, name
        assert float((ref[name][1] - ref[name][0].abs()).min()) > -1e-18  # the absolute-value sum bounds the value
    assert torch.count_nonzero(x64.grad[:, 2]) == 0 and 0.0 <= clamped < 0.9


def test_gate_catches_dropped_tap_swapped_channels_and_missing_border_zero():
    """A binary32 result within rounding of the restatement passes the gate of the GPU test (8 sqrt(K) 2^-24 of the absolute-value
    sum); the three faults fail it, each through g_xyz."""
    xyz, front, mask, g_out, g_paste = _inputs(9, 2, 16, 64, False, scale=0.3)
    ref = TC.paste_backward_ref(g_out, g_paste, mask, xyz, front, 0.7, True, True)
    good = TC.paste_backward_torch(g_out, g_paste, mask, xyz, front, 0.7, True, True, want_xyz=True, want_front=True)
    for name, ours in zip(("g_image", "g_xyz", "g_front"), good):
        assert TC.gate_ratio(ours, *ref[name]) <= 8.0, name
    for fault in ("tap", "swap", "border"):
        bad = TC.paste_backward_torch(g_out, g_paste, mask, xyz, front, 0.7, True, True, want_xyz=True, want_front=True, fault=fault)
        r = TC.gate_ratio(bad[1], *ref["g_xyz"])
        print(fault, r)
        assert r > 8.0, fault


def test_torch_formulation_vs_reference_train_step(monkeypatch):
    """paste.paste_front_torch under autograd on the reference's own inputs (its occlusion render comes from the fixture: the renderer
    is a device kernel): mask disagreement < 1 %, and on the agreeing pixels / the texels whose footprint holds no disagreeing pixel
    (at least 95 % of them) the gradients of the fixture's loss agree to rel-L2 1e-5."""
    from panic3d_amd import paste
    g = T.load_golden("train_step.npz")
    tt = lambda k: torch.from_numpy(g[k])
    x = TC.paste_x("cpu")
    x.update(force_rays={"ray_origins": tt("ray_origins"), "ray_directions": tt("ray_directions")}, normalize_images=False)
    out = {"image": TC.prepaste_from_sub4(g["image_sub4"]).requires_grad_(True), "image_xyz": tt("image_xyz").requires_grad_(True),
           "image_weights": tt("image_weights").requires_grad_(True)}
    monkeypatch.setattr(paste, "front_occlusion", lambda *a, **k: tt("occ"))
    G = types.SimpleNamespace(rendering_kwargs=TC.TRI_KW["rendering_kwargs"])
    res = paste.paste_front_torch(G, x, out, **TC.PASTE_PARAMS)
    TC.paste_loss(res["image"], out["image_weights"], out["image_xyz"]).backward()
    TC.check_paste_against_fixture(g, res["mask"], out["image"].grad, out["image_xyz"].grad)
