"""Cases shared by the dual discriminator's tests (tests/test_discriminator_cpu.py, tests/test_hip_discriminator.py) and by the
generator of their fixture (tests/golden/make_golden_discriminator.py): a seeded parameter fill and inputs that either implementation
of DualDiscriminator rebuilds bit for bit, float64 restatements of every layer written from the reference's formulas (torch's own
float64 convolution and autograd, not the code under test), binary32 stand-ins of the device operators for the CPU tests, and the
gates.  Not collected."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import synthesis_grad_ref as R
from train_step_cases import bias_act_backward_torch, rel_l2  # noqa: F401

SQRT2, SQRT_HALF = float(np.sqrt(2)), float(np.sqrt(0.5))

# ---- the small network of tests/golden/discriminator.npz -----------------------------------------------------------------------------
D_KW = dict(c_dim=25, img_resolution=32, img_channels=3, cond_mode="resnetcond_8", channel_base=1024, channel_max=48, conv_clamp=256,
            epilogue_kwargs={"mbstd_group_size": 2})
BATCH, RESNET_K = 4, 8
IMG_SCALE = 150.0   # fromrgb's outputs (~ sqrt(2) * IMG_SCALE in deviation) reach the clamp of 256 on some pixels
OUT_SCALE = 0.01    # b4.out's weights: the logits stay O(1), where the 1e-5 absolute forward gate means something in binary32
FILL_SEED, INPUT_SEED = 41, 42


def fill_discriminator(D, seed=FILL_SEED):
    """Seeded parameters for either implementation (same names by construction), in sorted-name order from one CPU generator: weights
    N(0,1) / lr_multiplier (StyleGAN2's init), biases 0.2 N(0,1) / lr_multiplier, b4.out's weights times OUT_SCALE."""
    g = torch.Generator().manual_seed(int(seed))
    with torch.no_grad():
        for name, p in sorted(D.named_parameters()):
            layer = D.get_submodule(name.rsplit(".", 1)[0])
            v = torch.randn(p.shape, generator=g) / getattr(layer, "bias_gain", 1)
            p.copy_(v if name.endswith("weight") else 0.2 * v)
        D.b4.out.weight.mul_(OUT_SCALE)
    return D


def discriminator_inputs(seed=INPUT_SEED, res=32, batch=BATCH):
    g = torch.Generator().manual_seed(int(seed))
    return {"image": torch.randn(batch, 3, res, res, generator=g) * IMG_SCALE,
            "image_raw": torch.randn(batch, 3, res // 2, res // 2, generator=g) * IMG_SCALE,
            "c": torch.randn(batch, 25, generator=g), "feats": torch.randn(batch, 16, generator=g), "g": torch.randn(batch, 1, generator=g)}


def checksum(D, inp):
    return float(sum(p.detach().double().sum() for p in D.parameters()) + sum(v.double().sum() for v in inp.values()))


def dsub(t):
    """What the fixture keeps of a gradient: all of a small tensor, every 2nd output and input channel of a large weight."""
    return t[::2, ::2].contiguous() if t.dim() >= 2 and t.numel() > 8192 else t


def key(name):
    return name.replace(".", "__")


# ---- operators from the reference's formulas, any dtype ------------------------------------------------------------------------------
def _pad4(padding):
    if isinstance(padding, int):
        padding = [padding, padding]
    padding = list(padding)
    if len(padding) == 2:
        padding = [padding[0], padding[0], padding[1], padding[1]]
    return [int(v) for v in padding]


def upfirdn2d_torch(x, f, up=1, down=1, padding=0, flip_filter=False, gain=1):
    """upfirdn2d.py:169-213 (_upfirdn2d_ref): zero-insert, pad or crop, convolve with f * gain (flipped unless flip_filter), decimate."""
    px0, px1, py0, py1 = _pad4(padding)
    N, C, H, W = x.shape
    z = x
    if up > 1:
        z = torch.zeros(N, C, H * up, W * up, dtype=x.dtype, device=x.device)
        z[:, :, ::up, ::up] = x
    z = F.pad(z, [max(px0, 0), max(px1, 0), max(py0, 0), max(py1, 0)])
    z = z[:, :, max(-py0, 0):z.shape[2] - max(-py1, 0), max(-px0, 0):z.shape[3] - max(-px1, 0)]
    ff = f.to(x) * gain
    if not flip_filter:
        ff = ff.flip([0, 1])
    y = F.conv2d(z, ff[None, None].repeat(C, 1, 1, 1), groups=C)
    return y[:, :, ::down, ::down]


def bias_act_any(z, b, act, gain, clamp):
    """bias_act.py:93-122: z + b -> act -> * gain -> clamp."""
    if b is not None:
        z = z + b.reshape(1, -1, *([1] * (z.ndim - 2)))
    if act == "lrelu":
        z = F.leaky_relu(z, 0.2)
    z = z * gain
    return z.clamp(-clamp, clamp) if clamp is not None and clamp >= 0 else z


def mbstd_any(x, group, Fc, fault=None):
    """MinibatchStdLayer.forward (networks_stylegan2.py:854-869), line for line."""
    N, C, H, W = x.shape
    G = min(group, N) if group is not None else N
    c = C // Fc
    y = x.reshape(G, -1, Fc, c, H, W)
    y = y - y.mean(dim=1 if fault == "axis" else 0, keepdim=fault == "axis")
    y = y.square().mean(dim=0)
    y = (y + 1e-8).sqrt()
    y = y.mean(dim=[2, 3, 4])
    y = y.reshape(-1, Fc, 1, 1)
    y = y.repeat(G, 1, H, W)
    return torch.cat([x, y], dim=1)


def wk_of(weight, weight_gain=1.0):
    """[O,I,k,k] -> the kernel's operand [taps][I][O]."""
    O, I, kh, kw = weight.shape
    return (weight * weight_gain).permute(2, 3, 1, 0).reshape(kh * kw, I, O).contiguous()


def weight_of(wk):
    taps, I, O = wk.shape
    k = 3 if taps == 9 else 1
    return wk.reshape(k, k, I, O).permute(3, 2, 0, 1)


# ---- one convolution layer: float64 restatement and a binary32 stand-in with seeded faults ---------------------------------------------
def conv_layer_f64(x, wk, bias, res, act, gain, clamp, stride, pad, gy):
    """The layer's forward from torch's float64 convolution and its gradients from torch autograd.  gain is the binary32 value the
    kernel receives.  Returns out, pre, the gradients, and for the gates the sums of absolute terms (abs_z of the forward, abs_gwk)."""
    d = torch.float64
    x, wk = x.to(d).requires_grad_(True), wk.to(d).requires_grad_(True)
    bias = bias.to(d).requires_grad_(True) if bias is not None else None
    res = res.to(d).requires_grad_(True) if res is not None else None
    z = F.conv2d(x, weight_of(wk), stride=stride, padding=pad)
    z.retain_grad()
    pre = bias_act_any(z, bias, act, R.f32(gain), None if clamp is None else R.f32(clamp))
    out = pre if res is None else pre + res
    (out * gy.to(d)).sum().backward()
    r = dict(out=out.detach(), pre=pre.detach(), gx=x.grad, gwk=wk.grad, gb=None if bias is None else bias.grad,
             gres=None if res is None else res.grad, gz=z.grad)
    with torch.no_grad():
        taps, Ci, Co = wk.shape
        _, absz = R.conv_dgrad_ref(x.detach(), wk.detach(), Co, out.shape[2], out.shape[3], stride, pad)
        r["abs_out"] = (absz + (bias.detach().abs().reshape(1, -1, 1, 1) if bias is not None else 0)) * abs(R.f32(gain)) + \
            (res.detach().abs() if res is not None else 0)
        r["K_out"] = taps * Ci + 2
        w = R.conv_wgrad_ref(z.grad, (1, 0, 0), x.detach(), None, (stride, 1 if taps == 9 else 0, pad), taps, out.shape[2:])
        assert rel_l2(w["dw"].transpose(1, 2), wk.grad) < 1e-12  # the header's index maps against autograd
        r["abs_gwk"] = w["abs_dw"].transpose(1, 2)
        r["K_gwk"] = x.shape[0] * out.shape[2] * out.shape[3]
    return r


def conv_layer_f32(x, wk, bias, res, act, gain, clamp, stride, pad, gy, fault=None):
    """A binary32 stand-in of the layer and its backward from the formulas of include/p3d_discriminator.h and p3d_synthesis_grad.h.
    fault: 'tap' (the centre or only tap dropped in the forward), 'unflipped' (the data gradient with the weights as they are),
    'mask' (the bias_act mask taken from the sum with the residual instead of the value before it)."""
    f = torch.float32
    taps, Ci, Co = wk.shape
    k = 3 if taps == 9 else 1
    N, _, Hi, Wi = x.shape
    Ho, Wo = (Hi + 2 * pad - k) // stride + 1, (Wi + 2 * pad - k) // stride + 1
    wf = wk.clone()
    if fault == "tap":
        wf[taps // 2, Ci // 2:] = 0
    z, _ = R.conv_dgrad_ref(x, wf, Co, Ho, Wo, stride, pad, dtype=f)
    pre = bias_act_any(z, bias, act, R.f32(gain), None if clamp is None else R.f32(clamp))
    out = pre if res is None else pre + res
    idx = 1 if act == "lrelu" else 0
    gz, gb, _ = bias_act_backward_torch(out if fault == "mask" else pre, gy, idx, 0.2, R.f32(gain), clamp)
    Z = gz
    if stride == 2:
        Z = torch.zeros(N, Co, 2 * Ho, 2 * Wo)
        Z[:, :, ::2, ::2] = gz
    wd = wk if fault == "unflipped" else wk.flip(0)
    gx, _ = R.conv_dgrad_ref(Z, wd.transpose(1, 2).contiguous(), Ci, Hi, Wi, 1, k - 1 - pad, dtype=f)
    dw = R.conv_wgrad_ref(gz, (1, 0, 0), x, None, (stride, 1 if k == 3 else 0, pad), taps, (Ho, Wo), dtype=f)["dw"]
    return dict(out=out, pre=pre, gx=gx, gwk=dw.transpose(1, 2), gb=gb.sum(0) if bias is not None else None, gres=gy if res is not None else None)


def layer_gate(got, ref, verbose=""):
    """The per-layer gate: rel-L2 <= 1e-5 against float64 for the output and every gradient, and for the two long sums (the output over
    taps * Ci terms, the weight gradient over N * Ho * Wo terms) |ours - ref| <= 8 sqrt(K) 2^-24 sum|terms| element by element.
    Returns the list of what failed."""
    bad = []
    for name in ("out", "gx", "gwk", "gb", "gres"):
        if ref.get(name) is None:
            continue
        e = rel_l2(got[name], ref[name])
        msg = f"{verbose}{name}: rel-L2 {e:.2e}"
        ok = e <= R.REL_L2
        if name in ("out", "gwk"):
            q = R.gate_ratio(got[name], ref[name], ref["abs_" + name], ref["K_" + name])
            msg += f", gate ratio {q:.3f} of {R.GATE_C:g}"
            ok = ok and q <= R.GATE_C
        print(msg)
        if not ok:
            bad.append(name)
    return bad


# (N, Ci, Co, H, W, taps, stride, pad): the issue's four shapes
CONV_SHAPES = {"fromrgb": (6, 5, 7, 9, 1, 1, 0), "conv0": (17, 65, 9, 11, 9, 1, 1), "conv1": (33, 20, 11, 11, 9, 2, 0), "epilogue": (49, 48, 4, 4, 9, 1, 1)}
# (bias, act, clamp, residual, N)
CONV_VARIANTS = {"plain": (False, "linear", None, False, 1), "bias_lrelu": (True, "lrelu", None, False, 3),
                 "clamp": (True, "lrelu", 0.7, False, 1), "residual": (True, "lrelu", 0.7, True, 3),
                 "linear_residual": (False, "linear", 0.9, True, 1)}


def conv_case(shape, variant, seed=0):
    Ci, Co, H, W, taps, stride, pad = CONV_SHAPES[shape]
    has_b, act, clamp, has_r, N = CONV_VARIANTS[variant]
    g = torch.Generator().manual_seed(1000 + seed + 17 * sorted(CONV_SHAPES).index(shape) + 101 * sorted(CONV_VARIANTS).index(variant))
    k = 3 if taps == 9 else 1
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    x = torch.randn(N, Ci, H, W, generator=g)
    wk = torch.randn(taps, Ci, Co, generator=g) / math.sqrt(taps * Ci)  # z ~ N(0,1): a clamp of 0.7 bites on about half the values
    return dict(x=x, wk=wk, bias=torch.randn(Co, generator=g) * 0.3 if has_b else None, res=torch.randn(N, Co, Ho, Wo, generator=g) if has_r else None,
                act=act, gain=SQRT2 * SQRT_HALF if has_r else None, clamp=clamp, stride=stride, pad=pad, gy=torch.randn(N, Co, Ho, Wo, generator=g))


def conv_case_args(c):
    gain = c["gain"] if c["gain"] is not None else (SQRT2 if c["act"] == "lrelu" else 1.0)
    return (c["x"], c["wk"], c["bias"], c["res"], c["act"], gain, c["clamp"], c["stride"], c["pad"], c["gy"])


def run_conv_layer(ops, c, device):
    """ops.conv2d_act on one case under autograd (and the same call under no_grad: the same bits): the output and every gradient."""
    t = {k: (v.clone().to(device).requires_grad_(True) if k in ("x", "wk", "bias", "res") else v) for k, v in c.items() if isinstance(v, torch.Tensor)}
    out = ops.conv2d_act(t["x"], t["wk"], t.get("bias"), act=c["act"], gain=c["gain"], clamp=c["clamp"], stride=c["stride"], pad=c["pad"],
                         res=t.get("res"))
    with torch.no_grad():
        plain = ops.conv2d_act(t["x"].detach(), t["wk"].detach(), None if c["bias"] is None else t["bias"].detach(), act=c["act"], gain=c["gain"],
                               clamp=c["clamp"], stride=c["stride"], pad=c["pad"], res=None if c["res"] is None else t["res"].detach())
    assert torch.equal(out.detach(), plain), "grad-mode forward bits differ from the no_grad call"
    out.backward(t["gy"].to(device))
    g = lambda k: t[k].grad.cpu() if k in t and t[k].grad is not None else None
    return dict(out=out.detach().cpu(), gx=g("x"), gwk=g("wk"), gb=g("bias"), gres=g("res"))


# ---- minibatch standard deviation ------------------------------------------------------------------------------------------------------
MBSTD_SHAPES = {"one_group": (4, 4, 5, 1, 4, 4), "two_stats": (6, 2, 6, 2, 3, 3), "g3": (3, 4, 4, 1, 4, 4)}  # (N, group, C, F, H, W)


def mbstd_case(name):
    N, group, C, Fc, H, W = MBSTD_SHAPES[name]
    g = torch.Generator().manual_seed(2000 + sorted(MBSTD_SHAPES).index(name))
    return dict(x=torch.randn(N, C, H, W, generator=g), gy=torch.randn(N, C + Fc, H, W, generator=g), group=group, F=Fc)


def mbstd_f64(c):
    x = c["x"].double().requires_grad_(True)
    y = mbstd_any(x, c["group"], c["F"])
    (y * c["gy"].double()).sum().backward()
    return dict(y=y.detach(), gx=x.grad)


def mbstd_f32(c, fault=None):
    x = c["x"].clone().requires_grad_(True)
    y = mbstd_any(x, c["group"], c["F"], fault=fault)
    (y * c["gy"]).sum().backward()
    return dict(y=y.detach(), gx=x.grad)


def mbstd_gate(got, ref, c):
    """rel-L2 <= 1e-5 for the concatenated output and for g_x; the statistic (a mean of c * HW positive deviations, so sum|terms| is
    the statistic itself) to 8 sqrt(K) 2^-24 of its value."""
    C = c["x"].shape[1]
    bad = [n for n in ("y", "gx") if rel_l2(got[n], ref[n]) > R.REL_L2]
    K = (C // c["F"]) * c["x"].shape[2] * c["x"].shape[3]
    q = R.gate_ratio(got["y"][:, C:], ref["y"][:, C:], ref["y"][:, C:].abs(), K)
    print(f"mbstd: rel-L2 y {rel_l2(got['y'], ref['y']):.2e}, g_x {rel_l2(got['gx'], ref['gx']):.2e}, statistic gate ratio {q:.3f} of {R.GATE_C:g}")
    if q > R.GATE_C:
        bad.append("stat")
    return bad


def mbstd_impl_torch(x, group, Fc):
    """ops._mbstd_impl on CPU tensors: (y, the deviation map [M,C,H,W], G)."""
    N, C, H, W = x.shape
    G = N if group is None else min(int(group), N)
    xg = x.reshape(G, N // G, C, H, W)
    sd = ((xg - xg.mean(0)).square().mean(0) + 1e-8).sqrt()
    return mbstd_any(x, group, Fc), sd, G


def mbstd_backward_torch(x, sd, gy, G, Fc):
    """ops.mbstd_backward from the header's formula."""
    N, C, H, W = x.shape
    M, c = N // G, C // Fc
    xg = x.reshape(G, M, C, H, W)
    gs = gy[:, C:].reshape(G, M, Fc, H * W).sum(dim=(0, 3))  # [M,F]
    gsc = gs[:, :, None].expand(M, Fc, c).reshape(1, M, C, 1, 1)
    return (gsc * (xg - xg.mean(0)) / (G * sd[None] * (c * H * W))).reshape(N, C, H, W)


# ---- stand-ins of the device operators, so that the host wiring runs on CPU ----------------------------------------------------------
def conv2d_act_impl_torch(x, wk, bias, act, gain, clamp, stride, pad, res, want_pre=False):
    g = gain if gain is not None else (SQRT2 if act == "lrelu" else 1.0)
    pre = bias_act_any(F.conv2d(x, weight_of(wk), stride=stride, padding=pad), bias, act, R.f32(g), clamp)
    out = pre if res is None else pre + res
    return (out, pre) if want_pre else out


def install_ops(monkeypatch, ops):
    import p3d_torch_ops
    for name, fn in dict(
            _conv2d_act_impl=conv2d_act_impl_torch, bias_act=p3d_torch_ops.bias_act, bias_act_backward=bias_act_backward_torch,
            conv_dgrad=lambda g, wk, Co, Ho, Wo, stride, pad: R.conv_dgrad_ref(g, wk, Co, Ho, Wo, stride, pad, dtype=torch.float32)[0],
            conv_wgrad=lambda g, gmap, x, s, xmap, taps, domain, wk=None, dscale=None:
                (R.conv_wgrad_ref(g, gmap, x, s, xmap, taps, domain, dtype=torch.float32)["dw"], None),
            upfirdn2d=upfirdn2d_torch, _mbstd_impl=mbstd_impl_torch, mbstd_backward=mbstd_backward_torch).items():
        monkeypatch.setattr(ops, name, fn)


# ---- the whole network in float64 ------------------------------------------------------------------------------------------------------
def filtered_resizing_any(img, size, f, filter_mode="antialiased"):
    """dual_discriminator.py:86-102 on upfirdn2d_torch."""
    it = lambda x, s, aa=False: F.interpolate(x, size=(s, s), mode="bilinear", align_corners=False, antialias=aa)
    if filter_mode == "antialiased":
        return it(img, size, True)
    if filter_mode == "classic":
        y = upfirdn2d_torch(img, f, up=2, padding=[2, 1, 2, 1], gain=4)   # upsample2d: pad ((4 + 1) // 2, (4 - 2) // 2), gain up^2
        y = it(y, size * 2 + 2)
        return upfirdn2d_torch(y, f, down=2, padding=0, flip_filter=True)  # downsample2d, padding -1: -1 + (4 - 2 + 1) // 2 = 0, -1 + 1 = 0
    if filter_mode == "none":
        return it(img, size)
    return (1 - filter_mode) * it(img, size) + filter_mode * it(img, size, True)


def discriminator_f64(p, image, image_raw, c, feats, kw=D_KW):
    """DualDiscriminator.forward restated from the reference's formulas on torch's own operators, in the dtype and on the device of its
    arguments (float64 on CPU in the tests; tools/bench_discriminator.py times it in binary32 on the GPU).  p: name -> raw parameter."""
    f = torch.tensor([1.0, 3.0, 3.0, 1.0], dtype=image.dtype, device=image.device)
    f = f.ger(f) / 64
    clamp, group = kw["conv_clamp"], kw["epilogue_kwargs"]["mbstd_group_size"]

    def conv(name, x, act, down=1, gain=1.0, has_clamp=True):
        w = p[name + ".weight"]
        k = w.shape[-1]
        w = w * (1 / math.sqrt(w.shape[1] * k * k))
        stride, pad = 1, k // 2
        if down == 2:  # conv2d_resample.py: the FIR first (padding k // 2 + 1 on every side; decimating for 1x1), then the convolution
            if k == 1:
                x = upfirdn2d_torch(x, f, down=2, padding=pad + 1)
            else:
                x, stride = upfirdn2d_torch(x, f, padding=pad + 1), 2
            pad = 0
        z = F.conv2d(x, w, stride=stride, padding=pad)
        return bias_act_any(z, p.get(name + ".bias"), act, (SQRT2 if act == "lrelu" else 1.0) * gain, clamp * gain if has_clamp else None)

    def fc(name, x, lr, act):
        w, b = p[name + ".weight"], p[name + ".bias"]
        y = x @ (w * (lr / math.sqrt(w.shape[1]))).t() + b * lr
        return F.leaky_relu(y, 0.2) * math.sqrt(2) if act else y
    img = torch.cat([image, filtered_resizing_any(image_raw, image.shape[-1], f)], 1)
    x, res = None, kw["img_resolution"]
    while res > 4:
        b = f"b{res}"
        if x is None:
            x = conv(b + ".fromrgb", img, "lrelu")
        y = conv(b + ".skip", x, "linear", down=2, gain=math.sqrt(0.5), has_clamp=False)
        x = conv(b + ".conv0", x, "lrelu")
        x = y + conv(b + ".conv1", x, "lrelu", down=2, gain=math.sqrt(0.5))
        res //= 2
    x = mbstd_any(x, group, 1)
    x = conv("b4.conv", x, "lrelu")
    x = fc("b4.out", fc("b4.fc", x.flatten(1), 1.0, True), 1.0, False)
    norm2 = lambda v: v * (v.square().mean(dim=1, keepdim=True) + 1e-8).rsqrt()
    m = norm2(fc("mapping.embed", torch.cat([c, feats[:, :RESNET_K]], 1), 1.0, False))
    i = 0
    while f"mapping.fc{i}.weight" in p:
        m = fc(f"mapping.fc{i}", m, 0.01, True)
        i += 1
    return (x * m).sum(dim=1, keepdim=True) * (1 / math.sqrt(m.shape[1]))


def discriminator_against_fixture(P, device):
    """The body of the network-level test, on CPU (stand-in operators) and on the GPU: logits to 1e-5 absolute, every gradient to
    rel-L2 1e-4 against the reference's fp32 autograd and 1e-5 against the float64 restatement (mapping_against_fixture's gates)."""
    import p3d_testing as T
    g = T.load_golden("discriminator.npz")
    D = fill_discriminator(P.DualDiscriminator(**D_KW)).to(device)
    inp = discriminator_inputs()
    assert abs(checksum(D, inp) - float(g["checksum"])) < 1e-6 * abs(float(g["checksum"])) + 1e-6, "re-drawn parameters / inputs differ"
    image, raw = (inp[k].clone().to(device).requires_grad_(True) for k in ("image", "image_raw"))
    logits = D({"image": image, "image_raw": raw}, inp["c"].to(device), {"resnet_feats": inp["feats"].to(device)})
    assert logits.grad_fn is not None
    (logits * inp["g"].to(device)).sum().backward()
    p64 = {n: q.detach().cpu().double().requires_grad_(True) for n, q in D.named_parameters()}
    i64, r64 = inp["image"].double().requires_grad_(True), inp["image_raw"].double().requires_grad_(True)
    l64 = discriminator_f64(p64, i64, r64, inp["c"].double(), inp["feats"].double())
    (l64 * inp["g"].double()).sum().backward()
    e_ref, e_64 = float((logits.detach().cpu() - torch.from_numpy(g["logits"])).abs().max()), float((logits.detach().cpu().double() - l64.detach()).abs().max())
    print(f"logits: max |.| {float(l64.detach().abs().max()):.3f}, vs reference fp32 {e_ref:.2e}, vs float64 {e_64:.2e}")
    first = D.b32.fromrgb(torch.cat([inp["image"], F.interpolate(inp["image_raw"], size=(32, 32), mode="bilinear", antialias=True)], 1).to(device)).detach()
    assert float(first.abs().max()) == 256.0, "no activation of the first block reaches the clamp"
    assert e_ref < 1e-5 and e_64 < 1e-5
    bad = []
    for name, ours, ref32, ref64 in [("image", image.grad, g["g_image"], i64.grad), ("image_raw", raw.grad, g["g_image_raw"], r64.grad)] + \
            [(n, q.grad, g["g_" + key(n)], p64[n].grad) for n, q in D.named_parameters()]:
        assert ours is not None and torch.isfinite(ours).all() and torch.count_nonzero(ours) > 0, name
        stored = ours.cpu() if name in ("image", "image_raw") else dsub(ours.cpu())
        e32, e64 = rel_l2(stored, ref32), rel_l2(ours, ref64)
        print(f"{name}: vs reference fp32 {e32:.2e}, vs float64 {e64:.2e}")
        if not (e32 <= 1e-4 and e64 <= 1e-5):
            bad.append((name, e32, e64))
        if name not in ("image", "image_raw"):
            n_ref = float(g["n_" + key(name)])
            assert abs(float(ours.double().norm()) - n_ref) <= 1e-4 * n_ref, name
    assert not bad, bad
