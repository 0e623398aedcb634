"""CPU (-m "not gpu"): LPIPS without a device — the C ABI of its operators (include/p3d_lpips.h, _lib.LPIPS_SIGNATURES and the library's
exports; argument errors come back before any launch), the restatements and gates that tests/test_hip_lpips.py holds the kernels to
(the binary32 stand-in passes them against float64, seeded faults fail them), and the host logic of panic3d_amd/lpips.py and
ops.lpips_distance on torch stand-ins of the operators.  On the parent commit the module, the table and the symbols do not exist."""
import os
import re

import pytest
import torch

import lpips_cases as LPC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def P():
    import panic3d_amd
    panic3d_amd.build()
    return panic3d_amd


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_lpips_header_table_and_exports_agree(P):
    hdr = open(os.path.join(ROOT, "include", "p3d_lpips.h")).read()
    declared = set(re.findall(r"\b(p3d_[a-z0-9_]+)\s*\(", hdr))
    lib = P._lib
    assert declared == set(lib.LPIPS_SIGNATURES) and len(declared) == 7 and all(n.startswith("p3d_lpips_") for n in declared)
    others = set(lib.SIGNATURES) | set(lib.GRAD_SIGNATURES) | set(lib.SYN_GRAD_SIGNATURES) | set(lib.PASTE_GRAD_SIGNATURES) | set(lib.DISC_SIGNATURES) \
        | set(lib.LOSS_SIGNATURES) | set(lib.OPTIM_SIGNATURES)
    assert not declared & others
    L = lib.lib()
    for name in declared:
        assert hasattr(L, name)
    B = P._build
    assert "p3d_lpips.hip" in B.SOURCES and os.path.join("..", "..", "include", "p3d_lpips.h") in B.HEADERS
    for unit in (B.RENDER_UNIT, B.SYNTHESIS_UNIT):
        assert not any("p3d_lpips" in s for s in unit)
    for name in ("MAX_K", "MAX_STRIDE", "BWD_MAX_CI"):
        assert int(re.search(rf"#define P3D_LPIPS_{name} (\d+)", hdr).group(1)) == getattr(lib, f"P3D_LPIPS_{name}")
    assert lib.P3D_ABI_VERSION == 9 and L.p3d_abi_version() == 9
    src = open(os.path.join(B.CSRC, "p3d_lpips.hip")).read()
    assert "sg_mma_chunk" in src and "atomic" not in src.replace("no float atomics", "").replace("with atomics", "")
    assert P.LPIPS is P.lpips.LPIPS and P.LPIPSLoss is P.lpips.LPIPSLoss


def test_lpips_argument_errors_without_gpu(P):
    L = P._lib.lib()
    p = 256  # never dereferenced: the checks come first

    def conv(x=p, N=1, Ci=3, Hi=31, Wi=31, wk=p, k=11, Co=8, Ho=7, Wo=7, stride=4, pad=2, bias=p, shift=None, scale=None, out=p):
        return L.p3d_lpips_conv_relu_f32(x, N, Ci, Hi, Wi, wk, k, Co, Ho, Wo, stride, pad, bias, shift, scale, out, None)
    assert conv(x=None) == -1 and conv(wk=None) == -1 and conv(bias=None) == -1 and conv(out=None) == -1 and conv(N=0) == -1 and conv(Co=0) == -1
    assert conv(shift=p) == -1 and conv(scale=p) == -1  # both or neither
    assert conv(k=12, Ho=6, Wo=6) == -2 and conv(stride=5) == -2 and conv(stride=0) == -2 and conv(pad=11) == -2 and conv(pad=-1) == -2
    assert conv(Ho=8) == -2 and conv(Wo=6) == -2 and conv(Hi=3, Wi=3, k=11, pad=2, Ho=1, Wo=1) == -2

    def bwd(g_in=p, g_head=p, a=p, N=1, Co=8, Ho=7, Wo=7, wkb=p, k=11, Ci=3, Hi=31, Wi=31, stride=4, pad=2, scale=None, gx=p):
        return L.p3d_lpips_conv_relu_backward_f32(g_in, g_head, a, N, Co, Ho, Wo, wkb, k, Ci, Hi, Wi, stride, pad, scale, gx, None)
    assert bwd(g_in=None, g_head=None) == -1 and bwd(wkb=None) == -1 and bwd(gx=None) == -1 and bwd(N=0) == -1
    assert bwd(Ci=5) == -2  # a strided layer's backward: at most P3D_LPIPS_BWD_MAX_CI input channels
    assert bwd(Ho=8) == -2 and bwd(stride=5) == -2
    assert bwd(k=3, stride=1, pad=1, Ho=31, Wo=31, scale=p) == -2  # the scaling layer belongs to the stem

    pool = lambda x=p, planes=4, H=7, W=7, y=p: L.p3d_lpips_pool_f32(x, planes, H, W, y, None)
    assert pool(x=None) == -1 and pool(y=None) == -1 and pool(planes=0) == -1 and pool(H=0) == -1 and pool(H=2) == -2 and pool(W=2) == -2
    poolb = lambda x=p, g=p, planes=4, H=7, W=7, gx=p: L.p3d_lpips_pool_backward_f32(x, g, planes, H, W, gx, None)
    assert poolb(x=None) == -1 and poolb(g=None) == -1 and poolb(gx=None) == -1 and poolb(W=2) == -2

    assert L.p3d_lpips_head_workspace_bytes(3, 70) == 3 * 70 * 4 and L.p3d_lpips_head_workspace_bytes(0, 70) == 0

    def head(a0=p, a1=p, lin=p, N=2, C=5, HW=7, v=p, out=None, acc=0, ws=p, nbytes=1 << 20):
        return L.p3d_lpips_head_f32(a0, a1, lin, N, C, HW, v, out, acc, ws, nbytes, None)
    assert head(a0=None) == -1 and head(a1=None) == -1 and head(lin=None) == -1 and head(v=None) == -1 and head(ws=None) == -1 and head(C=0) == -1
    assert head(N=70000) == -2 and head(nbytes=2 * 7 * 4 - 1) == -3
    headb = lambda a0=p, a1=p, lin=p, g=p, N=2, C=5, HW=7, ga=p: L.p3d_lpips_head_backward_f32(a0, a1, lin, g, N, C, HW, None, 1, ga, None)
    assert headb(a0=None) == -1 and headb(g=None) == -1 and headb(ga=None) == -1 and headb(HW=0) == -1 and headb(N=70000) == -2


def test_public_operators_check_before_any_launch(P):
    """Python-side argument errors: raised on CPU tensors' shapes before anything reaches the library."""
    ops = P.ops
    with pytest.raises(RuntimeError, match="CUDA/ROCm"):
        ops.lpips_pool(torch.zeros(1, 1, 7, 7))
    with pytest.raises(ValueError, match="k 12"):
        ops._lpips_out_hw(31, 31, 12, 4, 2)
    with pytest.raises(ValueError, match="smaller than the kernel"):
        ops._lpips_out_hw(3, 3, 11, 4, 2)
    assert ops._lpips_out_hw(512, 512, 11, 4, 2) == (127, 127) and ops.LPIPS_MIN_SIZE == 31


# ---- the gates: the binary32 stand-in passes, seeded faults fail ------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(LPC.CONV_SHAPES))
def test_conv_stand_in_passes_and_faults_fail(name):
    c = LPC.conv_case(name)
    ref = LPC.conv_ref(c)
    assert LPC.conv_gate(LPC.run_conv(LPC.TorchOps, c, "cpu"), ref, c) == []
    assert float((c["a"] == 0).float().mean()) > 0.2, "the mask does not bite"
    if c["fold"]:
        assert torch.count_nonzero(ref["gx"][..., 37]) == 0 and torch.count_nonzero(ref["gx"][..., 36]) > 0  # column 37: read by no window
    faults = ["mask", "unflipped"] + (["phase"] if c["stride"] > 1 else [])
    if name == "k3-tiny":
        faults.remove("unflipped")  # a 1 x 2 input under a 3 x 3 kernel: flipping exchanges taps that all read padding but one column pair
    for fault in faults:
        bad = LPC.conv_ref(c, torch.float32, fault=fault)
        got = LPC.gate(f"[{fault}] {name} gx", bad["gx"], ref["gx"], ref["gx_abs"], c["Kb"])
        assert got != [], (name, fault)


@pytest.mark.parametrize("shape", LPC.POOL_SHAPES)
def test_pool_restatement_is_torch_and_last_maximum_fails(shape):
    c = LPC.pool_case(*shape)
    x64 = c["x"].double().requires_grad_(True)
    LPC.pool(x64).backward(c["g"].double())  # torch's own float64 backward: the first maximum in scan order
    ref = LPC.pool_backward(c["x"].double(), c["g"].double())
    assert torch.equal(ref, x64.grad)
    absref = LPC.pool_backward(c["x"].double(), c["g"].double().abs())
    assert LPC.gate(f"pool {shape}", LPC.pool_backward(c["x"], c["g"]), ref, absref, 4) == []
    assert LPC.gate(f"[last] pool {shape}", LPC.pool_backward(c["x"], c["g"], fault="last"), ref, absref, 4) != []
    H, W = shape[1:]
    if H % 2 == 0:
        assert torch.count_nonzero(ref[:, :, H - 1]) == 0
    if W % 2 == 0:
        assert torch.count_nonzero(ref[:, :, :, W - 1]) == 0


@pytest.mark.parametrize("shape", LPC.HEAD_SHAPES)
def test_head_stand_in_passes_and_dropped_projection_fails(shape):
    c = LPC.head_case(*shape)
    d = lambda v: v.double()
    ref_v, abs_v = LPC.head(d(c["a0"]), d(c["a1"]), d(c["lin"])), LPC.head(d(c["a0"]), d(c["a1"]), d(c["lin"]), absref=True)
    ref_g = LPC.head_backward(d(c["a0"]), d(c["a1"]), d(c["lin"]), d(c["g"]))
    abs_g = LPC.head_backward(d(c["a0"]), d(c["a1"]), d(c["lin"]), d(c["g"]), absref=True)
    assert LPC.gate(f"head {shape} v", LPC.head(c["a0"], c["a1"], c["lin"]), ref_v, abs_v, c["K"]) == []
    got = LPC.head_backward(c["a0"], c["a1"], c["lin"], c["g"])
    assert torch.isfinite(got).all() and LPC.gate(f"head {shape} g_a0", got, ref_g, abs_g, c["K"] + 4) == []
    gz = LPC.head_backward(c["a0"], c["a1"], c["lin"], c["g"], g_add=c["g_add"], relu_mask=True)
    assert torch.equal(gz, torch.where(c["a0"] > 0, c["g_add"] + got, torch.zeros_like(got)))
    # the closed form is autograd's, where autograd is finite
    a0 = d(c["a0"]).requires_grad_(True)
    (LPC.head(a0, d(c["a1"]), d(c["lin"])) * d(c["g"])).sum().backward()
    keep = torch.isfinite(a0.grad)
    assert LPC.rel_l2(ref_g[keep], a0.grad[keep]) < 1e-12
    if shape[1] > 1:
        bad = LPC.head_backward(c["a0"], c["a1"], c["lin"], c["g"], fault="projection")
        assert LPC.gate(f"[projection] head {shape}", bad, ref_g, abs_g, c["K"] + 4) != []


def test_whole_distance_stand_in(P, monkeypatch):
    """ops.lpips_distance on the stand-ins against the float64 restatement, value and gradient, at the device test's bounds."""
    LPC.install_ops(monkeypatch, P.ops)
    H, W, N, ch = 35, 47, 3, LPC.SMALL
    c = LPC.distance_case(H, W, N, ch)
    model = LPC.fill_model(P.LPIPS(channels=ch), c["weights"])
    x0 = c["x0"].clone().requires_grad_(True)
    out = model(x0, c["x1"])
    assert tuple(out.shape) == (N, 1, 1, 1) and out.grad_fn is not None
    with torch.no_grad():
        assert torch.equal(model(c["x0"], c["x1"]), out.detach())  # grad mode and no_grad: the same launches
    (out.flatten() * c["g"]).sum().backward()
    err_v = float(((out.detach().flatten().double() - c["v64"]).abs() / c["v64"].abs()).max())
    e_ours, e_t32 = LPC.rel_l2(x0.grad, c["gx64"]), LPC.rel_l2(c["gx32"], c["gx64"])
    print(f"value {err_v:.2e}; gradient ours {e_ours:.2e}, torch32 {e_t32:.2e}")
    assert err_v <= 1e-5 and e_ours <= 4 * e_t32
    assert all(p.grad is None and not p.requires_grad for p in model.parameters())


# ---- the module's host logic ------------------------------------------------------------------------------------------------------------
class _FakeLpips(torch.nn.Module):
    """A module with the names the `lpips` package is believed to use."""

    def __init__(self, channels):
        super().__init__()
        S = torch.nn.Sequential
        self.scaling_layer = torch.nn.Module()
        self.scaling_layer.register_buffer("shift", torch.tensor(LPC.SHIFT).view(1, 3, 1, 1))
        self.scaling_layer.register_buffer("scale", torch.tensor(LPC.SCALE).view(1, 3, 1, 1))
        self.net = torch.nn.Module()
        Ci = 3
        for i, ((k, s, p, _), Co, idx) in enumerate(zip(LPC.LAYERS, channels, (0, 3, 6, 8, 10))):
            sl = torch.nn.Module()
            sl.add_module(str(idx), torch.nn.Conv2d(Ci, Co, k, s, p))
            self.net.add_module(f"slice{i + 1}", sl)
            lin = torch.nn.Module()
            lin.model = S(torch.nn.Dropout(), torch.nn.Conv2d(Co, 1, 1, bias=False))
            self.add_module(f"lin{i}", lin)
            Ci = Co


def test_state_dict_names_load(P):
    ch = LPC.SMALL
    fake = _FakeLpips(ch)
    model = P.LPIPS(channels=ch)
    assert set(model.state_dict()) == set(fake.state_dict())
    res = model.load_state_dict(fake.state_dict(), strict=False)
    assert res.missing_keys == [] and res.unexpected_keys == []
    assert all(torch.equal(a, b) for a, b in zip(model.state_dict().values(), fake.state_dict().values()))
    assert all(not p.requires_grad for p in model.parameters())
    full = P.LPIPS()
    assert full.channels == (64, 192, 384, 256, 256) and tuple(getattr(full.net.slice1, "0").weight.shape) == (64, 3, 11, 11)
    tv = {f"features.{idx}.{leaf}": getattr(getattr(getattr(fake.net, f"slice{i + 1}"), str(idx)), leaf).detach() * 2
          for i, idx in enumerate((0, 3, 6, 8, 10)) for leaf in ("weight", "bias")}
    model.load_torchvision_alexnet(tv)
    assert torch.equal(model.convs()[2].weight, tv["features.6.weight"]) and torch.equal(model.convs()[4].bias, tv["features.10.bias"])
    with pytest.raises(KeyError):
        model.load_torchvision_alexnet({})
    for kw in (dict(spatial=True), dict(lpips=False), dict(version="0.0")):
        with pytest.raises(NotImplementedError, match="spatial=False"):
            P.LPIPS(**kw)
    assert P.LPIPS(channels=ch, pretrained=True, verbose=False).channels == ch  # the package's other options are accepted
    for net in ("vgg", "squeeze"):
        with pytest.raises(NotImplementedError, match="training_loop_v0.py:168"):
            P.LPIPS(net=net)
        with pytest.raises(NotImplementedError, match="training_loop_v0.py:168"):
            P.LPIPSLoss(net_type=net)


def test_module_host_logic(P, monkeypatch):
    LPC.install_ops(monkeypatch, P.ops)
    ch = LPC.SMALL
    c = LPC.distance_case(31, 31, 3, ch)
    loss = P.LPIPSLoss()
    assert isinstance(loss.model, P.LPIPS) and loss.net_type == "alex"
    loss.model = LPC.fill_model(P.LPIPS(channels=ch), c["weights"])
    v = loss(c["x0"], c["x1"])
    assert tuple(v.shape) == (3,) and float(((v.double() - c["v64"]).abs() / c["v64"]).max()) <= 1e-5
    model = loss.model
    # normalize=True maps [0, 1] to [-1, 1] first
    assert torch.allclose(model((c["x0"] + 1) / 2, (c["x1"] + 1) / 2, normalize=True).flatten(), v, rtol=1e-5)
    # sizes and shapes
    small = torch.zeros(1, 3, 30, 40)
    with pytest.raises(ValueError, match="31"):
        model(small, small)
    with pytest.raises(ValueError, match="31"):
        model(small.transpose(2, 3), small.transpose(2, 3))
    with pytest.raises(ValueError, match="shape"):
        model(c["x0"], c["x1"][:2])
    with pytest.raises(ValueError, match="expected"):
        model(c["x0"][:, :2], c["x1"][:, :2])
    # a target with grad
    with pytest.raises(NotImplementedError, match="target"):
        model(c["x0"], c["x1"].clone().requires_grad_(True))
    with torch.no_grad():
        model(c["x0"], c["x1"].clone().requires_grad_(True))  # nothing is recorded: allowed
    # double backward
    x0 = c["x0"].clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match="first order"):
        torch.autograd.grad([model(x0, c["x1"]).sum()], [x0], create_graph=True)
    # the cached layouts: reused while nothing changes, re-derived after an in-place write
    ops1 = model.operands()
    assert model.operands() is ops1
    before = model(c["x0"], c["x1"]).clone()
    with torch.no_grad():
        model.convs()[1].weight.mul_(1.5)
    ops2 = model.operands()
    assert ops2 is not ops1 and not torch.equal(ops2["layers"][1][0], ops1["layers"][1][0])
    assert torch.equal(ops2["layers"][1][2], P.ops.lpips_backward_weights(ops2["layers"][1][0]))
    assert not torch.equal(model(c["x0"], c["x1"]), before)
    with torch.no_grad():
        model.lin3.weight.zero_()
    assert float(model.operands()["layers"][3][3].abs().max()) == 0.0
    prev = P.memo.set_enabled(False)
    try:
        assert model.operands() is not model.operands()
    finally:
        P.memo.set_enabled(prev)


def test_loss_takes_the_model(P, monkeypatch):
    """StyleGAN2LossOrthoCondA(lpips_model=LPIPSLoss()) as it is: one Gcond phase on the stand-ins, against the restatement as the model."""
    import loss_cases as LC
    LC.install_ops(monkeypatch, P.ops)
    LPC.install_ops(monkeypatch, P.ops)
    got, want = LPC.gcond_phase(P, monkeypatch, "cpu")
    LPC.compare_phase(got, want)
