"""Cases of LPIPS (panic3d_amd/lpips.py, include/p3d_lpips.h), shared by tests/test_lpips_cpu.py and tests/test_hip_lpips.py:

  * restatements of the four stages and of the whole distance, written from the formulas of include/p3d_lpips.h in plain torch and
    generic in the number format: in float64 they are the reference, in binary32 the stand-in (`TorchOps`, and install_ops(monkeypatch,
    ops) for CPU runs of the host wiring).  The backward stages are written out by hand (with seedable faults, so that the tests can
    show that the gates notice them); the whole distance is differentiated by torch's autograd;
  * the gates (loss_cases.gate: per value 8 sqrt(K) 2^-24 sum|terms|, rel-L2 <= 1e-5) and the scale each value is judged by;
  * the case lists.
"""
import math

import torch

import loss_cases as LC

F = torch.nn.functional
EPS = 1e-10
SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
LAYERS = ((11, 4, 2, True), (5, 1, 2, True), (3, 1, 1, False), (3, 1, 1, False), (3, 1, 1, False))  # (k, stride, pad, pool after it)
FULL = (64, 192, 384, 256, 256)
SMALL = (5, 18, 33, 20, 9)


def scaling(dtype, device="cpu"):
    """The scaling layer's constants as the device holds them: binary32 values, then widened."""
    return tuple(torch.tensor(v, dtype=torch.float32, device=device).to(dtype) for v in (SHIFT, SCALE))


# ---- the stages, generic in dtype ---------------------------------------------------------------------------------------------------------
def conv_relu(x, w, b, stride, pad, fold, absref=False):
    """max(corr(s(x), w) + b, 0); w [Co,Ci,k,k].  absref: the sum of the |terms| of z instead."""
    if fold:
        shift, scale = scaling(x.dtype, x.device)
        x = (x - shift.view(1, -1, 1, 1)) / scale.view(1, -1, 1, 1)
    if absref:
        return F.conv2d(x.abs(), w.abs(), b.abs(), stride=stride, padding=pad)
    return F.relu(F.conv2d(x, w, b, stride=stride, padding=pad))


def conv_relu_backward(g_in, g_head, a, w, stride, pad, hw, fold, fault=None, absref=False):
    """The data gradient written out: every tap (ty, tx) sends gz[oy][ox] w[ty][tx] to the input pixel (stride oy + ty - pad, ...).
    faults: 'unflipped' (the gather form run with unflipped weights: the taps mirrored), 'phase' (the taps one row off: another
    phase's), 'mask' (taken from a + g, not from a)."""
    g = (g_in if g_in is not None else 0) + (g_head if g_head is not None else 0)
    if absref:
        g = (g_in.abs() if g_in is not None else 0) + (g_head.abs() if g_head is not None else 0)
        w = w.abs()
    gz = torch.where((a + g if fault == "mask" else a) > 0, g, torch.zeros_like(g)) if a is not None else g  # a None: masked already
    if fault == "unflipped":
        w = w.flip(2, 3)
    if fault == "phase":
        w = w.roll(1, 2)
    N, Co, Ho, Wo = gz.shape
    Ci, k = w.shape[1], w.shape[2]
    Hi, Wi = hw
    buf = torch.zeros(N, Ci, max(Hi + 2 * pad, stride * (Ho - 1) + k), max(Wi + 2 * pad, stride * (Wo - 1) + k), dtype=gz.dtype, device=gz.device)
    for ty in range(k):
        for tx in range(k):
            buf[:, :, ty:ty + stride * (Ho - 1) + 1:stride, tx:tx + stride * (Wo - 1) + 1:stride] += torch.einsum("nohw,oc->nchw", gz, w[:, :, ty, tx])
    gx = buf[:, :, pad:pad + Hi, pad:pad + Wi]
    if fold:
        gx = gx / scaling(gz.dtype, gz.device)[1].view(1, -1, 1, 1)
    return gx.contiguous()


def pool(x):
    return F.max_pool2d(x, 3, 2)


def pool_backward(x, g, fault=None):
    """Each cotangent to the FIRST maximum of its window in row-major scan order ('last': to the last one)."""
    N, C, H, W = x.shape
    Ho, Wo = g.shape[2:]
    win = x.unfold(2, 3, 2).unfold(3, 3, 2).reshape(N, C, Ho, Wo, 9)
    eq = win == win.max(dim=-1, keepdim=True).values
    if fault == "last":
        pick = eq & (eq.flip(-1).cumsum(-1).flip(-1) == 1)
    else:
        pick = eq & (eq.cumsum(-1) == 1)
    gx = torch.zeros_like(x)
    for t in range(9):
        ty, tx = divmod(t, 3)
        gx[:, :, ty:ty + 2 * (Ho - 1) + 1:2, tx:tx + 2 * (Wo - 1) + 1:2] += g * pick[..., t].to(g.dtype)
    return gx


def head(a0, a1, lin, absref=False):
    """v [N]; a0, a1 [N,C,HW]; lin [C].  absref: the scale v is judged by — the terms of lin (n0 - n1)^2 multiplied out,
    sum_c |lin| (|n0| + |n1|)^2: the roundings of n0 and n1 enter d in proportion to n0 and n1, not to their difference."""
    n0 = a0 / (a0.square().sum(1, keepdim=True).sqrt() + EPS)
    n1 = a1 / (a1.square().sum(1, keepdim=True).sqrt() + EPS)
    lin = lin.view(1, -1, 1)
    if absref:
        return (lin.abs() * (n0.abs() + n1.abs()).square()).sum(1).mean(1)
    return (lin * (n0 - n1).square()).sum(1).mean(1)


def head_backward(a0, a1, lin, g, fault=None, absref=False, g_add=None, relu_mask=False):
    """include/p3d_lpips.h's closed form ('projection': its second term dropped); a pixel with r0 == 0 gets 0.  g_add, relu_mask: the
    kernel's optional last step, a0 > 0 ? g_add + g_a0 : 0."""
    HW = a0.shape[2]
    r0 = a0.square().sum(1, keepdim=True).sqrt()
    i0 = r0 + EPS
    n0, n1 = a0 / i0, a1 / (a1.square().sum(1, keepdim=True).sqrt() + EPS)
    lin, gs = lin.view(1, -1, 1), (g / HW).view(-1, 1, 1)
    if absref:
        u = 2 * lin.abs() * (n0.abs() + n1.abs()) * gs.abs()
        a0 = a0.abs()
    else:
        u = 2 * lin * (n0 - n1) * gs
    den = r0 * i0.square()
    proj = a0 * (u * a0).sum(1, keepdim=True) / torch.where(r0 > 0, den, torch.ones_like(den))
    out = u / i0 + proj if absref else (u / i0 if fault == "projection" else u / i0 - proj)
    out = torch.where(r0 > 0, out, torch.zeros_like(out))
    if g_add is not None:
        out = (g_add.abs() if absref else g_add) + out
    return torch.where(a0 > 0, out, torch.zeros_like(out)) if relu_mask else out


# ---- the whole distance (torch differentiates this one) ---------------------------------------------------------------------------------
def make_weights(channels, seed):
    """Seeded He-scaled trunk, small biases, non-negative lin with some exact zeros: [(w [Co,Ci,k,k], b [Co], lin [Co])] in binary32."""
    g = torch.Generator().manual_seed(seed)
    out, Ci = [], 3
    for (k, _, _, _), Co in zip(LAYERS, channels):
        w = torch.randn(Co, Ci, k, k, generator=g) * math.sqrt(2.0 / (Ci * k * k))
        b = torch.randn(Co, generator=g) * 0.1
        lin = torch.rand(Co, generator=g) / Co
        lin[::5] = 0.0
        out.append((w, b, lin))
        Ci = Co
    return out


def distance(x0, x1, weights, dtype):
    """[N] in `dtype`; differentiable in x0 by autograd."""
    x = torch.cat([x0.to(dtype), x1.to(dtype)])
    N = x0.shape[0]
    total = 0
    for l, ((k, stride, pad, pool_after), (w, b, lin)) in enumerate(zip(LAYERS, weights)):
        x = conv_relu(x, w.to(dtype), b.to(dtype), stride, pad, l == 0)
        a = x.flatten(2)
        total = total + head(a[:N], a[N:], lin.to(dtype))
        if pool_after:
            x = pool(x)
    return total


def make_images(N, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    x0 = torch.rand(N, 3, H, W, generator=g) * 2 - 1
    x1 = (x0 + 0.3 * torch.randn(N, 3, H, W, generator=g)).clamp(-1, 1)
    return x0, x1


DISTANCE_CASES = [(H, W, N, SMALL) for (H, W) in ((31, 31), (35, 47), (64, 64)) for N in (1, 3)] + [(64, 64, 2, FULL)]
_DISTANCE_REF = {}


def distance_case(H, W, N, channels):
    """The images, the weights and, computed once: the float64 value and gradient, and torch's binary32 autograd of the same
    restatement (the yardstick of the gradient's bound)."""
    key = (H, W, N, channels)
    if key not in _DISTANCE_REF:
        x0, x1 = make_images(N, H, W, 100 + H + W + N)
        weights = make_weights(channels, 7)
        g = torch.linspace(0.5, 1.5, N)
        res = {}
        for dtype in (torch.float64, torch.float32):
            xg = x0.to(dtype).clone().requires_grad_(True)
            v = distance(xg, x1, weights, dtype)
            (v * g.to(dtype)).sum().backward()
            res[dtype] = (v.detach(), torch.nan_to_num(xg.grad, nan=0.0))
        _DISTANCE_REF[key] = dict(x0=x0, x1=x1, weights=weights, g=g, v64=res[torch.float64][0], gx64=res[torch.float64][1],
                                  v32=res[torch.float32][0], gx32=res[torch.float32][1])
    return _DISTANCE_REF[key]


def fill_model(model, weights):
    """Copy [(w, b, lin)] into an LPIPS module (through the tensors: the version counters move)."""
    with torch.no_grad():
        for conv, lin_mod, (w, b, lin) in zip(model.convs(), model.lins(), weights):
            conv.weight.copy_(w)
            conv.bias.copy_(b)
            lin_mod.weight.copy_(lin.view(1, -1, 1, 1))
    return model


# ---- stage cases ------------------------------------------------------------------------------------------------------------------------
# (N, Ci, Co, Hi, Wi, k, stride, pad, the scaling fold)
CONV_SHAPES = {
    "stem-fold-ragged": (2, 3, 7, 31, 38, 11, 4, 2, True),   # ragged Co; column 37 is read by no window
    "stem-64": (1, 3, 64, 43, 31, 11, 4, 2, False),
    "k5-co70": (2, 9, 70, 7, 9, 5, 1, 2, False),              # Co across a 64 tile, K = 225
    "k3-ci65": (1, 65, 33, 5, 6, 3, 1, 1, False),
    "k3-tiny": (1, 6, 6, 1, 2, 3, 1, 1, False),               # input smaller than the kernel
}
POOL_SHAPES = ((5, 7, 7), (3, 8, 10), (2, 3, 3), (1, 63, 63))
HEAD_SHAPES = ((1, 1, 1), (2, 5, 7), (3, 64, 33), (2, 384, 70))


def conv_case(name, seed=0):
    N, Ci, Co, Hi, Wi, k, stride, pad, fold = CONV_SHAPES[name]
    g = torch.Generator().manual_seed(seed + 31 * sorted(CONV_SHAPES).index(name))
    Ho, Wo = (Hi + 2 * pad - k) // stride + 1, (Wi + 2 * pad - k) // stride + 1
    x = torch.randn(N, Ci, Hi, Wi, generator=g) * (0.5 if fold else 1.0)
    w = torch.randn(Co, Ci, k, k, generator=g) * math.sqrt(2.0 / (Ci * k * k))
    b = torch.randn(Co, generator=g) * 0.1
    a = F.relu(torch.randn(N, Co, Ho, Wo, generator=g))  # the stored output the mask is taken from: exact zeros on about half
    g_in = torch.randn(N, Co, Ho, Wo, generator=g) if name != "k3-tiny" else None
    g_head = torch.randn(N, Co, Ho, Wo, generator=g)
    return dict(name=name, x=x, w=w, b=b, a=a, g_in=g_in, g_head=g_head, k=k, stride=stride, pad=pad, fold=fold, K=k * k * Ci + 2, Kb=k * k * Co + 2)


def conv_ref(c, dtype=torch.float64, fault=None):
    """(a, the scale of a, gx, the scale of gx) of a case in `dtype`."""
    t = lambda v: v.to(dtype) if v is not None else None
    args = (t(c["g_in"]), t(c["g_head"]), t(c["a"]), t(c["w"]), c["stride"], c["pad"], tuple(c["x"].shape[2:]), c["fold"])
    return dict(a=conv_relu(t(c["x"]), t(c["w"]), t(c["b"]), c["stride"], c["pad"], c["fold"]),
                a_abs=conv_relu(t(c["x"]), t(c["w"]), t(c["b"]), c["stride"], c["pad"], c["fold"], absref=True),
                gx=conv_relu_backward(*args, fault=fault), gx_abs=conv_relu_backward(*args, absref=True))


def pool_case(planes, H, W, seed=0):
    """Planted exact ties (values from a set of five), an all-zero window, an all-negative window."""
    g = torch.Generator().manual_seed(seed + planes * 1000 + H * 10 + W)
    x = torch.randint(-2, 3, (1, planes, H, W), generator=g).float() * 0.5
    if H >= 7:
        x[:, :, 0:3, 0:3] = 0.0
        x[:, :, 2:5, 4:7] = -1.5
        x[:, 0, 4:7, 0:3] = torch.randn(3, 3, generator=g)  # and one window without ties
    Ho, Wo = (H - 3) // 2 + 1, (W - 3) // 2 + 1
    return dict(x=x, g=torch.randn(1, planes, Ho, Wo, generator=g))


def head_case(N, C, HW, seed=0):
    g = torch.Generator().manual_seed(seed + N * 100000 + C * 100 + HW)
    a0, a1 = F.relu(torch.randn(N, C, HW, generator=g)), F.relu(torch.randn(N, C, HW, generator=g))
    if HW >= 3:  # an all-zero pixel in a0, in a1, and in both
        a0[:, :, 0] = 0.0
        a1[:, :, 1] = 0.0
        a0[:, :, 2] = 0.0
        a1[:, :, 2] = 0.0
    lin = torch.rand(C, generator=g)
    if C > 1:
        lin[::3] = 0.0
    return dict(a0=a0, a1=a1, lin=lin, g=torch.randn(N, generator=g), g_add=torch.randn(N, C, HW, generator=g) * 0.1, K=C)


def gate(name, ours, ref, absref, K, verbose=True):
    return LC.gate(name, ours, ref, absref, K, verbose=verbose)


rel_l2 = LC.rel_l2


# ---- the loss --------------------------------------------------------------------------------------------------------------------------
def gcond_phase(P, monkeypatch, device, size=64):
    """One Gcond phase of StyleGAN2LossOrthoCondA on loss_cases' stand-in G and D at size x size, twice: with LPIPSLoss() (full widths,
    seeded weights) as lpips_model, and with the binary32 torch restatement on the same weights.  ((reports, grads), (reports, grads))."""
    monkeypatch.setattr(LC, "S", size)
    weights = make_weights(FULL, 9)
    ours = P.LPIPSLoss()
    fill_model(ours.model, weights)
    ours.to(device)
    capture = lambda hook: monkeypatch.setattr(P.loss, "report", hook)
    runs = []
    # (the restatement runs on the CPU whatever the device: torch's own arithmetic, no convolution library's choice of algorithm)
    for model in (ours, lambda a, b: distance(a.cpu(), b.cpu(), weights, torch.float32).to(a.device)):
        monkeypatch.setattr(LC, "lpips_stand_in", model)
        runs.append(LC.run_phase(P.StyleGAN2LossOrthoCondA, LC.PHASE_CASES["Gcond"], capture, device=device))
    return runs


def compare_phase(got, want):
    """The loss tests' own bounds: the reported LPIPS term to 1e-5 relative, every gradient to rel-L2 <= 1e-4."""
    (r_got, g_got), (r_want, g_want) = got, want
    assert set(r_got) == set(r_want) and set(g_got) == set(g_want) and "Loss/G/cond/lpips" in r_got and "G.image" in g_got
    for k in sorted(r_want):
        err = float((r_got[k] - r_want[k]).abs().max()) / max(float(r_want[k].abs().max()), 1e-30)
        print(f"Gcond {k}: {err:.2e}")
        assert err <= 1e-5, (k, err)
    for k in sorted(g_want):
        assert torch.isfinite(g_got[k]).all()
        err = rel_l2(g_got[k], g_want[k]) if float(g_want[k].abs().max()) > 0 else float(g_got[k].abs().max())
        print(f"Gcond grad {k}: {err:.2e}")
        assert err <= 1e-4, (k, err)


# ---- the stages through an operator namespace (panic3d_amd.ops on the device, TorchOps on the CPU) ---------------------------------------
def to_wk(w):
    Co, Ci, k, _ = w.shape
    return w.permute(2, 3, 1, 0).reshape(k * k, Ci, Co).contiguous()


def from_wk(wk, k):
    return wk.reshape(k, k, wk.shape[1], wk.shape[2]).permute(3, 2, 0, 1).contiguous()


class TorchOps:
    """The public operators' signatures on the binary32 restatements."""

    @staticmethod
    def lpips_conv_relu(x, wk, bias, k, stride, pad, shift=None, scale=None):
        return conv_relu(x, from_wk(wk, k), bias, stride, pad, shift is not None)

    @staticmethod
    def lpips_backward_weights(wk):
        return wk.flip(0).transpose(1, 2).contiguous()

    @staticmethod
    def lpips_conv_relu_backward(g_in, g_head, a, wkb, k, Ci, Hi, Wi, stride, pad, scale=None):
        wk = wkb.flip(0).transpose(1, 2) if stride == 1 else wkb
        return conv_relu_backward(g_in, g_head, a, from_wk(wk.contiguous(), k), stride, pad, (Hi, Wi), scale is not None)

    @staticmethod
    def lpips_pool(x):
        return pool(x)

    @staticmethod
    def lpips_pool_backward(x, g):
        return pool_backward(x, g)

    @staticmethod
    def lpips_head(a0, a1, lin):
        return head(a0.flatten(2), a1.flatten(2), lin.reshape(-1))

    @staticmethod
    def lpips_head_backward(a0, a1, lin, g, g_add=None, relu_mask=False):
        return head_backward(a0.flatten(2), a1.flatten(2), lin.reshape(-1), g.reshape(-1), g_add=g_add.flatten(2) if g_add is not None else None,
                             relu_mask=relu_mask).reshape(a0.shape)


def run_conv(ops, c, device):
    """(a, gx) of a conv case through `ops`."""
    d = lambda v: v.to(device) if v is not None else None
    wk = d(to_wk(c["w"]))
    shift, scale = (d(s) for s in scaling(torch.float32)) if c["fold"] else (None, None)
    a = ops.lpips_conv_relu(d(c["x"]), wk, d(c["b"]), c["k"], c["stride"], c["pad"], shift, scale)
    wkb = ops.lpips_backward_weights(wk) if c["stride"] == 1 else wk
    Ci, Hi, Wi = c["x"].shape[1:]
    gx = ops.lpips_conv_relu_backward(d(c["g_in"]), d(c["g_head"]), d(c["a"]), wkb, c["k"], Ci, Hi, Wi, c["stride"], c["pad"], scale)
    # the same cotangent handed over finished (one binary32 addition, then the mask: the same numbers): the same bits
    g = c["g_head"] if c["g_in"] is None else c["g_in"] + c["g_head"]
    gz = torch.where(c["a"] > 0, g, torch.zeros_like(g))
    assert torch.equal(ops.lpips_conv_relu_backward(d(gz), None, None, wkb, c["k"], Ci, Hi, Wi, c["stride"], c["pad"], scale), gx), "pre-masked form"
    return a, gx


def conv_gate(got, ref, c, verbose=True):
    a, gx = got
    return gate(f"{c['name']} a", a, ref["a"], ref["a_abs"], c["K"], verbose) + gate(f"{c['name']} gx", gx, ref["gx"], ref["gx_abs"], c["Kb"], verbose)


def install_ops(monkeypatch, ops):
    """Replace the seven device operators of panic3d_amd.ops by the binary32 restatements (CPU runs of the host wiring)."""
    T = TorchOps

    def head_impl(a0, a1, lin, v, out, accumulate):
        r = T.lpips_head(a0, a1, lin)
        v.copy_(r)
        if out is not None:
            out.copy_(out + r if accumulate else r)

    monkeypatch.setattr(ops, "_lpips_conv_relu_impl", T.lpips_conv_relu)
    monkeypatch.setattr(ops, "_lpips_conv_relu_backward_impl", T.lpips_conv_relu_backward)
    monkeypatch.setattr(ops, "_lpips_pool_impl", T.lpips_pool)
    monkeypatch.setattr(ops, "_lpips_pool_backward_impl", T.lpips_pool_backward)
    monkeypatch.setattr(ops, "_lpips_head_impl", head_impl)
    monkeypatch.setattr(ops, "_lpips_head_backward_impl", T.lpips_head_backward)
