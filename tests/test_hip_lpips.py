"""GPU (-m gpu): LPIPS on the HIP kernels (include/p3d_lpips.h, panic3d_amd/lpips.py).  Stage level: every kernel on the binary32 inputs
of the float64 restatement (tests/lpips_cases.py; no decision can differ) under the project's gates — per value 8 sqrt(K) 2^-24
sum|terms|, rel-L2 <= 1e-5 — at the smallest shapes that can still go wrong; two runs give the same bits.  Whole distance: the value to
1e-5 relative against float64, the gradient against torch's binary32 autograd of the same restatement (a few ReLU pre-activations lie
inside the rounding band, so a per-element gate is wrong there): rel-L2(ours, f64) <= 4 rel-L2(torch32, f64); grad mode and no_grad give
the same bits.  Loss: one Gcond phase of StyleGAN2LossOrthoCondA with LPIPSLoss() as lpips_model against the torch restatement as the
model.  The gates' sensitivity to seeded faults is shown on CPU in tests/test_lpips_cpu.py.  On the parent commit the module, the
operators and the symbols do not exist."""
import pytest
import torch

import lpips_cases as LPC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P():
    import panic3d_amd
    panic3d_amd.build()
    panic3d_amd._lib.lib()
    return panic3d_amd


@pytest.mark.parametrize("name", sorted(LPC.CONV_SHAPES))
def test_conv_relu_and_its_backward(P, name):
    c = LPC.conv_case(name)
    ref = LPC.conv_ref(c)
    a, b = LPC.run_conv(P.ops, c, "cuda"), LPC.run_conv(P.ops, c, "cuda")
    assert LPC.conv_gate([t.cpu() for t in a], ref, c) == []
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), "two runs differ"
    if c["fold"]:  # column 37 of the 38-wide input is read by no window: an exact zero, not a small number
        assert torch.count_nonzero(a[1][..., 37]) == 0 and torch.count_nonzero(a[1][..., 36]) > 0


@pytest.mark.parametrize("shape", LPC.POOL_SHAPES)
def test_pool_and_its_backward(P, shape):
    c = LPC.pool_case(*shape)
    x, g = c["x"].cuda(), c["g"].cuda()
    y = P.ops.lpips_pool(x)
    assert torch.equal(y.cpu(), LPC.pool(c["x"])) and torch.equal(P.ops.lpips_pool(x), y)
    gx = P.ops.lpips_pool_backward(x, g)
    ref = LPC.pool_backward(c["x"].double(), c["g"].double())
    assert LPC.gate(f"pool {shape} gx", gx.cpu(), ref, LPC.pool_backward(c["x"].double(), c["g"].double().abs()), 4) == []
    assert torch.equal(P.ops.lpips_pool_backward(x, g), gx), "two runs differ"
    H, W = shape[1:]
    if H % 2 == 0:
        assert torch.count_nonzero(gx[:, :, H - 1]) == 0
    if W % 2 == 0:
        assert torch.count_nonzero(gx[:, :, :, W - 1]) == 0


@pytest.mark.parametrize("shape", LPC.HEAD_SHAPES)
def test_head_and_its_backward(P, shape):
    c = LPC.head_case(*shape)
    d = lambda v: v.double()
    a0, a1, lin, g = (c[k].cuda() for k in ("a0", "a1", "lin", "g"))
    v = P.ops.lpips_head(a0, a1, lin)
    ga = P.ops.lpips_head_backward(a0, a1, lin, g)
    bad = LPC.gate(f"head {shape} v", v.cpu(), LPC.head(d(c["a0"]), d(c["a1"]), d(c["lin"])), LPC.head(d(c["a0"]), d(c["a1"]), d(c["lin"]), absref=True), c["K"])
    bad += LPC.gate(f"head {shape} g_a0", ga.cpu(), LPC.head_backward(d(c["a0"]), d(c["a1"]), d(c["lin"]), d(c["g"])),
                    LPC.head_backward(d(c["a0"]), d(c["a1"]), d(c["lin"]), d(c["g"]), absref=True), c["K"] + 4)
    # the optional last step: the incoming cotangent added, the ReLU mask of a0 applied
    gz = P.ops.lpips_head_backward(a0, a1, lin, g, c["g_add"].cuda(), True)
    bad += LPC.gate(f"head {shape} gz", gz.cpu(), LPC.head_backward(d(c["a0"]), d(c["a1"]), d(c["lin"]), d(c["g"]), g_add=d(c["g_add"]), relu_mask=True),
                    LPC.head_backward(d(c["a0"]), d(c["a1"]), d(c["lin"]), d(c["g"]), absref=True, g_add=d(c["g_add"]), relu_mask=True), c["K"] + 5)
    assert torch.equal(gz, torch.where(a0 > 0, c["g_add"].cuda() + ga, torch.zeros_like(ga)))
    assert bad == []
    assert torch.isfinite(ga).all()
    if shape[2] >= 3:
        assert torch.count_nonzero(ga[:, :, 0]) == 0 and torch.count_nonzero(ga[:, :, 2]) == 0  # the all-zero pixels of a0
    assert torch.equal(P.ops.lpips_head(a0, a1, lin), v) and torch.equal(P.ops.lpips_head_backward(a0, a1, lin, g), ga), "two runs differ"


def test_public_operators_check_their_arguments(P):
    z = lambda *s: torch.zeros(*s, device="cuda")
    with pytest.raises(ValueError):
        P.ops.lpips_conv_relu(z(1, 3, 31, 31), z(121, 3, 8), z(8), 11, 5, 2)      # stride
    with pytest.raises(ValueError):
        P.ops.lpips_conv_relu(z(1, 3, 31, 31), z(121, 4, 8), z(8), 11, 4, 2)      # wk's channels
    with pytest.raises(ValueError):
        P.ops.lpips_conv_relu(z(1, 3, 31, 31), z(121, 3, 8), z(8), 11, 4, 2, shift=z(3))
    with pytest.raises(ValueError):
        P.ops.lpips_conv_relu_backward(None, None, z(1, 8, 7, 7), z(121, 3, 8), 11, 3, 31, 31, 4, 2)
    with pytest.raises(ValueError):
        P.ops.lpips_conv_relu_backward(None, z(1, 8, 7, 7), z(1, 8, 7, 7), z(121, 5, 8), 11, 5, 31, 31, 4, 2)  # a strided layer: Ci <= 4
    with pytest.raises(ValueError):
        P.ops.lpips_pool(z(1, 1, 2, 7))
    with pytest.raises(ValueError):
        P.ops.lpips_head(z(1, 4, 5), z(1, 4, 6), z(4))


@pytest.mark.parametrize("H,W,N,channels", LPC.DISTANCE_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_whole_distance(P, H, W, N, channels):
    c = LPC.distance_case(H, W, N, channels)
    model = LPC.fill_model(P.LPIPS(channels=channels), c["weights"]).cuda()
    runs = []
    for _ in range(2):
        x0 = c["x0"].cuda().requires_grad_(True)
        out = model(x0, c["x1"].cuda())
        assert tuple(out.shape) == (N, 1, 1, 1)
        (out.flatten() * c["g"].cuda()).sum().backward()
        runs.append((out.detach().clone(), x0.grad.clone()))
    with torch.no_grad():
        assert torch.equal(model(c["x0"].cuda(), c["x1"].cuda()), runs[0][0]), "grad mode and no_grad differ"
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), "two runs differ"
    v, gx = runs[0][0].flatten().cpu().double(), runs[0][1].cpu()
    err_v, err_v32 = float(((v - c["v64"]).abs() / c["v64"].abs()).max()), float(((c["v32"].double() - c["v64"]).abs() / c["v64"].abs()).max())
    e_ours, e_t32 = LPC.rel_l2(gx, c["gx64"]), LPC.rel_l2(c["gx32"], c["gx64"])
    print(f"lpips {H}x{W} N={N} widths {channels}: value {err_v:.2e} (torch32 {err_v32:.2e}); gradient rel-L2 ours {e_ours:.2e}, torch32 {e_t32:.2e}")
    assert torch.isfinite(gx).all()
    assert err_v <= 1e-5
    assert e_ours <= 4 * e_t32
    assert all(p.grad is None for p in model.parameters())


def test_distance_argument_errors(P):
    model = P.LPIPS(channels=LPC.SMALL).cuda()
    x = torch.zeros(1, 3, 30, 31, device="cuda")
    with pytest.raises(ValueError, match="31"):
        model(x, x)
    y = torch.zeros(1, 3, 31, 31, device="cuda")
    with pytest.raises(NotImplementedError, match="target"):
        model(y, y.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="CUDA/ROCm"):
        model(y.cpu(), y.cpu())
    x0 = (y + 0.25).requires_grad_(True)
    with pytest.raises(RuntimeError, match="first order"):
        torch.autograd.grad([model(x0, y).sum()], [x0], create_graph=True)


def test_gcond_phase_with_the_model(P, monkeypatch):
    import loss_cases as LC
    LC.draws_on_cpu(monkeypatch)
    got, want = LPC.gcond_phase(P, monkeypatch, "cuda")
    LPC.compare_phase(got, want)
