"""Cases of the conditioning encoder (panic3d_amd/encoder.py, include/p3d_encoder.h), shared by tests/test_encoder_cpu.py and
tests/test_hip_encoder.py:

  * a restatement of the stages and of the whole extractor in plain torch (F.conv2d, F.batch_norm in eval form, F.max_pool2d,
    F.interpolate), generic in the number format: with UNFOLDED batch norm and the unfolded PCA expression of katepca.py:27-29.  In
    float64 it is the reference; in binary32 on the CPU it is the yardstick the whole network's error is measured against;
  * binary32 stand-ins of the four device operators on the FOLDED operands (`TorchOps`, install_ops(monkeypatch, ops)) for CPU runs of
    the host wiring, with seedable faults so that the tests can show that the gates notice them;
  * the gates (loss_cases.gate: per value 8 sqrt(K) 2^-24 sum|terms|, rel-L2 <= 1e-5; the front end: 4 2^-24 sum|terms|) and the case lists.
"""
import math

import torch

import loss_cases as LC

F = torch.nn.functional
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
BN_EPS = 1e-5
STAGES = ("conv1", "layer1", "layer2", "layer3", "layer4")
rel_l2 = LC.rel_l2
gate = LC.gate


# ---- the stages, generic in dtype -----------------------------------------------------------------------------------------------------
def resize_hw(H, W, size):
    return (int(size * H / W), size) if W <= H else (size, int(size * W / H))


def norm_consts(dtype):
    """mean, std as the device holds them: binary32 values, then widened."""
    return tuple(torch.tensor(v, dtype=torch.float32).to(dtype).view(1, 3, 1, 1) for v in (MEAN, STD))


def prepare(img, size, absref=False):
    """[N,C>=3,H,W] -> [2N,3,h,w]: the image and its mirror, resized (bilinear, align_corners=False, no antialiasing), normalised."""
    x = img[:, :3]
    x = torch.cat([x, x.flip(dims=(-1,))], dim=0)
    h, w = resize_hw(img.shape[2], img.shape[3], size)
    mean, std = norm_consts(img.dtype)
    r = F.interpolate(x.abs() if absref else x, size=(h, w), mode="bilinear", align_corners=False)
    return (r + mean) / std if absref else (r - mean) / std


def conv(x, w, b, stride, res=None, relu=False, absref=False, fault=None):
    """[relu](corr(x, w) + b [+ res]); w [Co,Ci,k,k], pad (k - 1) / 2.  absref: the sum of the |terms| instead.
    faults: 'no_res' (the residual dropped), 'bias_per_split' (the bias added once per split of two, not once)."""
    pad = (w.shape[2] - 1) // 2
    if absref:
        z = F.conv2d(x.abs(), w.abs(), b.abs(), stride=stride, padding=pad)
        return z + res.abs() if res is not None else z
    z = F.conv2d(x, w, b * 2 if fault == "bias_per_split" else b, stride=stride, padding=pad)
    if res is not None and fault != "no_res":
        z = z + res
    return F.relu(z) if relu else z


def maxpool(x, fault=None):
    """3 x 3 stride 2 padding 1; 'zero_pad': the padding counts as 0, not as -infinity."""
    if fault == "zero_pad":
        return F.max_pool2d(F.pad(x, (1, 1, 1, 1)), 3, 2, 0)
    return F.max_pool2d(x, 3, 2, 1)


# ---- the whole extractor: unfolded batch norm, unfolded PCA ---------------------------------------------------------------------------
def block_plan(blocks, base_width, stem_width):
    """[(prefix, Ci, width, stride, has_downsample)] in order."""
    out, Ci = [], stem_width
    for l, nb in enumerate(blocks):
        width, stride = base_width << l, 1 if l == 0 else 2
        for b in range(nb):
            s = stride if b == 0 else 1
            out.append((f"layer{l + 1}.{b}", Ci, width, s, b == 0 and (s != 1 or Ci != width * 4)))
            Ci = width * 4
    return out


def make_weights(blocks=(3, 4, 6, 3), base_width=64, stem_width=64, pca_dim=None, num_classes=None, seed=0):
    """A seeded state dict under torchvision's names (binary32), batch norms with non-trivial statistics; plus 'pca.components' [D,C]
    and 'pca.mean' [C] when pca_dim is given."""
    g = torch.Generator().manual_seed(seed)
    sd = {}

    def add_conv(name, Ci, Co, k):
        sd[f"{name}.weight"] = torch.randn(Co, Ci, k, k, generator=g) * math.sqrt(2.0 / (Ci * k * k))

    def add_bn(name, C, gain=1.0):
        sd[f"{name}.weight"] = (0.5 + torch.rand(C, generator=g)) * gain
        sd[f"{name}.bias"] = torch.randn(C, generator=g) * 0.1
        sd[f"{name}.running_mean"] = torch.randn(C, generator=g) * 0.1
        sd[f"{name}.running_var"] = 0.5 + torch.rand(C, generator=g)
        sd[f"{name}.num_batches_tracked"] = torch.tensor(7, dtype=torch.long)
    add_conv("conv1", 3, stem_width, 7)
    add_bn("bn1", stem_width)
    Ci = stem_width
    for pre, Ci, width, _, down in block_plan(blocks, base_width, stem_width):
        add_conv(f"{pre}.conv1", Ci, width, 1), add_bn(f"{pre}.bn1", width)
        add_conv(f"{pre}.conv2", width, width, 3), add_bn(f"{pre}.bn2", width)
        add_conv(f"{pre}.conv3", width, width * 4, 1), add_bn(f"{pre}.bn3", width * 4, 0.5)
        if down:
            add_conv(f"{pre}.downsample.0", Ci, width * 4, 1), add_bn(f"{pre}.downsample.1", width * 4, 0.5)
    C = (base_width << 3) * 4
    if num_classes is not None:
        sd["fc.weight"], sd["fc.bias"] = torch.randn(num_classes, C, generator=g) / math.sqrt(C), torch.randn(num_classes, generator=g) * 0.1
    if pca_dim is not None:
        sd["pca.components"] = torch.linalg.qr(torch.randn(C, pca_dim, generator=g))[0].t().contiguous()
        sd["pca.mean"] = torch.rand(C, generator=g)
    return sd


def network(sd, img, size, blocks, base_width, stem_width, dtype, features=STAGES + ("pca",)):
    """The reference's forward (katebackbone.py:103-121, katepca.py:17-30) on the state dict `sd` in `dtype`: {feature: [2N,C,h,w]}."""
    t = lambda name: sd[name].to(dtype)

    def bn(x, name):
        return F.batch_norm(x, t(f"{name}.running_mean"), t(f"{name}.running_var"), t(f"{name}.weight"), t(f"{name}.bias"), False, 0.0, BN_EPS)
    ans = {}
    x = prepare(img.to(dtype), size)
    x = F.relu(bn(F.conv2d(x, t("conv1.weight"), stride=2, padding=3), "bn1"))
    ans["conv1"] = x
    x = F.max_pool2d(x, 3, 2, 1)
    for pre, _, _, stride, down in block_plan(blocks, base_width, stem_width):
        idn = x
        y = F.relu(bn(F.conv2d(x, t(f"{pre}.conv1.weight")), f"{pre}.bn1"))
        y = F.relu(bn(F.conv2d(y, t(f"{pre}.conv2.weight"), stride=stride, padding=1), f"{pre}.bn2"))
        y = bn(F.conv2d(y, t(f"{pre}.conv3.weight")), f"{pre}.bn3")
        if down:
            idn = bn(F.conv2d(x, t(f"{pre}.downsample.0.weight"), stride=stride), f"{pre}.downsample.1")
        x = F.relu(y + idn)
        ans[pre.split(".")[0]] = x  # (the last block's output stays)
    if "pca.components" in sd:
        pw, pb = t("pca.components")[None][:, None, None], t("pca.mean")[None][..., None, None]
        ans["pca"] = (pw @ (x - pb).permute(0, 2, 3, 1)[..., None]).squeeze(-1).permute(0, 3, 1, 2)  # katepca.py:27-29
    return {k: v for k, v in ans.items() if k in features}


def fill_model(model, sd):
    """Load a make_weights dict into a ResNetEncoder (or the .rfe of a ResnetFeatureExtractorPCA)."""
    res = model.load_state_dict({k: v for k, v in sd.items() if not k.startswith("pca.")}, strict=False)
    assert res.missing_keys == [] and res.unexpected_keys == [], res
    if "pca.components" in sd:
        model.set_pca(sd["pca.components"], sd["pca.mean"])
    return model


TINY = dict(blocks=(1, 2, 1, 1), base_width=8, stem_width=8)
FULL = dict(blocks=(3, 4, 6, 3), base_width=64, stem_width=64)
# name -> (architecture, PCA components, image shape, size)
NETWORK_CASES = {"tiny": (TINY, 16, (2, 4, 40, 36), 32), "full-128": (FULL, 512, (1, 3, 128, 128), 128)}
_NETWORK_REF = {}


def make_image(shape, seed):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed))


def network_case(name):
    """The case's weights, image, float64 reference and binary32 CPU restatement: computed once, shared, left unchanged."""
    if name not in _NETWORK_REF:
        arch, dim, shape, size = NETWORK_CASES[name]
        sd = make_weights(pca_dim=dim, seed=11 + len(name), **arch)
        img = make_image(shape, 5)
        with torch.no_grad():
            f64 = network(sd, img, size, dtype=torch.float64, **arch)
            f32 = network(sd, img, size, dtype=torch.float32, **arch)
        _NETWORK_REF[name] = dict(arch=arch, dim=dim, size=size, sd=sd, img=img, f64=f64, f32=f32)
    return _NETWORK_REF[name]


def network_gate(name, ours, c, factor=4.0, verbose=True):
    """Per feature: rel-L2(ours, f64) <= factor * rel-L2(torch binary32 of the same restatement on the CPU, f64).  -> violations."""
    bad = []
    for k in sorted(ours):
        e, e32 = rel_l2(ours[k].cpu(), c["f64"][k]), rel_l2(c["f32"][k], c["f64"][k])
        if verbose:
            print(f"encoder {name} {k}: rel-L2 ours {e:.3e}, torch32 {e32:.3e} (ratio {e / max(e32, 1e-30):.2f})")
        if tuple(ours[k].shape) != tuple(c["f64"][k].shape) or not e <= factor * e32:
            bad.append(f"{name} {k}: {e:.3g} > {factor} * {e32:.3g}")
    return bad


# ---- stage cases ----------------------------------------------------------------------------------------------------------------------
# name -> (N, Ci, Co, H, W, k, stride, residual, relu)
CONV_CASES = {
    "k1-res-relu": (2, 20, 40, 5, 7, 1, 1, True, True),
    "k1-s2": (2, 6, 10, 9, 7, 1, 2, False, False),               # 9 x 7 -> 5 x 4
    "k3-relu": (2, 12, 24, 6, 5, 3, 1, False, True),
    "k3-s2-odd": (2, 10, 12, 9, 7, 3, 2, False, True),
    "k3-s2-even": (2, 10, 12, 8, 8, 3, 2, False, True),
    "k7-s2-stem": (2, 3, 16, 20, 18, 7, 2, False, True),
    "k1-splitk": (2, 520, 72, 2, 2, 1, 1, True, True),           # large K, eight output pixels: the split-K regime
    "k1-pca": (2, 136, 20, 3, 3, 1, 1, False, False),            # bias only: the PCA layer
    "one-pixel": (1, 5, 3, 1, 1, 3, 1, False, True),             # N = 1, a single output pixel
}
# every plan: both tiles, without a split, with two, with as many as there are chunks (want is clipped to the chunk count)
PLANS = (0,) + tuple((tile << 8) | want for tile in (1, 2) for want in (1, 2, 255))
POOL_SHAPES = ((3, 7, 9), (1, 8, 8), (2, 1, 1), (1, 2, 3))
PREPARE_CASES = (((12, 16), 8), ((10, 10), 7), ((5, 6), 8))


def conv_case(name, seed=0):
    N, Ci, Co, H, W, k, stride, has_res, relu = CONV_CASES[name]
    g = torch.Generator().manual_seed(seed + 17 * sorted(CONV_CASES).index(name))
    pad = (k - 1) // 2
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    x = torch.randn(N, Ci, H, W, generator=g)
    w = torch.randn(Co, Ci, k, k, generator=g) * math.sqrt(2.0 / (Ci * k * k))
    b = torch.randn(Co, generator=g) * 0.5
    res = torch.randn(N, Co, Ho, Wo, generator=g) if has_res else None
    return dict(name=name, x=x, w=w, b=b, res=res, k=k, stride=stride, relu=relu, K=Ci * k * k + 1 + int(has_res))


def conv_ref(c, dtype=torch.float64, fault=None):
    t = lambda v: v.to(dtype) if v is not None else None
    return dict(y=conv(t(c["x"]), t(c["w"]), t(c["b"]), c["stride"], t(c["res"]), c["relu"], fault=fault),
                y_abs=conv(t(c["x"]), t(c["w"]), t(c["b"]), c["stride"], t(c["res"]), absref=True))


def to_wk(w):
    Co, Ci, k, _ = w.shape
    return w.permute(2, 3, 1, 0).reshape(k * k, Ci, Co).contiguous()


def from_wk(wk, k):
    return wk.reshape(k, k, wk.shape[1], wk.shape[2]).permute(3, 2, 0, 1).contiguous()


def run_conv(ops, c, device, plan=0):
    d = lambda v: v.to(device) if v is not None else None
    return ops.enc_conv(d(c["x"]), d(to_wk(c["w"])), d(c["b"]), c["k"], c["stride"], d(c["res"]), c["relu"], plan)


def conv_gate(y, ref, c, tag="", verbose=True):
    return gate(f"{c['name']}{tag}", y, ref["y"], ref["y_abs"], c["K"], verbose=verbose)


def pool_case(planes, H, W, seed=0):
    """Two inputs: mixed signs, and all negative (the network feeds the pool post-ReLU values only, which cannot expose zero padding)."""
    g = torch.Generator().manual_seed(seed + planes * 1000 + H * 10 + W)
    x = torch.randn(2, planes, H, W, generator=g)
    return dict(x=x, neg=-x.abs() - 0.25)


def prepare_case(hw, size, seed=0):
    g = torch.Generator().manual_seed(seed + hw[0] * 100 + hw[1])
    return dict(img=torch.rand(2, 4, hw[0], hw[1], generator=g), size=size)


PREPARE_C = 4.0


def prepare_gate(name, ours, img, size, verbose=True):
    """Per value 4 2^-24 sum|terms| against the float64 resize of the image and of its mirror (all 2N rows alike).  -> violations."""
    ref, absref = prepare(img.double(), size), prepare(img.double(), size, absref=True)
    r = LC.gate_ratio(ours, ref, absref, 1)
    if verbose:
        print(f"gate {name}: worst {r:.3f} (c = {PREPARE_C:g})")
    return [f"{name}: ratio {r:.3g}"] if tuple(ours.shape) != tuple(ref.shape) or not r <= PREPARE_C else []


# ---- binary32 stand-ins of the device operators (the folded operands, the kernels' formulas) ----------------------------------------------
def _source(d, n_in, n_out):
    """The kernel's source cells and weights along one axis: the exact rational ((2d + 1) in - out) / (2 out), each weight rounded once."""
    num = (2 * d + 1) * n_in - n_out
    den = 2 * n_out
    num = num.clamp_min(0)
    i0, rem = num // den, num % den
    i1 = (i0 + 1).clamp_max(n_in - 1)
    return i0, i1, ((den - rem).float() / float(den)), (rem.float() / float(den))


class TorchOps:
    """The public operators' signatures on binary32 torch arithmetic."""

    @staticmethod
    def enc_conv(x, wk, bias, k, stride=1, res=None, relu=False, force_plan=0, fault=None):
        return conv(x, from_wk(wk, k), bias, stride, res, relu, fault=fault)

    @staticmethod
    def enc_maxpool(x, fault=None):
        return maxpool(x, fault=fault)

    @staticmethod
    def enc_prepare_hw(img, mean, std, h, w):
        N, _, H, W = img.shape
        x = img[:, :3].float()
        x0, x1, lx0, lx1 = _source(torch.arange(w), W, w)
        y0, y1, ly0, ly1 = _source(torch.arange(h), H, h)
        ly0, ly1 = ly0.view(-1, 1), ly1.view(-1, 1)
        rows = []
        for mirror in (False, True):
            a0, a1 = (W - 1 - x0, W - 1 - x1) if mirror else (x0, x1)
            v = lambda yy, xx: x[:, :, yy][:, :, :, xx]
            # fma(lx1, v01, lx0 v00) restated with the product rounded separately: binary32 without the fused step (one more rounding)
            top = torch.addcmul(lx0 * v(y0, a0), lx1, v(y0, a1))
            bot = torch.addcmul(lx0 * v(y1, a0), lx1, v(y1, a1))
            rows.append(torch.addcmul(ly0 * top, ly1, bot))
        r = torch.cat(rows)
        return (r - mean.view(1, 3, 1, 1)) / std.view(1, 3, 1, 1)

    @staticmethod
    def enc_prepare(img, mean, std, size):
        return TorchOps.enc_prepare_hw(img, mean, std, *resize_hw(img.shape[2], img.shape[3], size))


def install_ops(monkeypatch, ops):
    """Replace the four device operators of panic3d_amd.ops by the binary32 stand-ins (CPU runs of the host wiring)."""
    T = TorchOps

    def forward_impl(prog):
        for r in prog.records:
            src = prog.buffer(r["src"], r["shape"])
            if r["kind"] == "prepare":
                y = T.enc_prepare_hw(src, r["w"], r["b"], r["out_shape"][2], r["out_shape"][3])
            elif r["kind"] == "maxpool":
                y = T.enc_maxpool(src)
            else:
                res = prog.buffer(r["res"], r["out_shape"]) if r.get("res") is not None else None
                y = T.enc_conv(src, r["w"], r["b"], r["k"], r["stride"], res, r["relu"])
            prog.buffer(r["dst"], r["out_shape"]).copy_(y)

    monkeypatch.setattr(ops, "_enc_conv_impl", lambda x, wk, bias, k, stride, res, relu, plan: T.enc_conv(x, wk, bias, k, stride, res, relu))
    monkeypatch.setattr(ops, "_enc_maxpool_impl", T.enc_maxpool)
    monkeypatch.setattr(ops, "_enc_prepare_impl", T.enc_prepare_hw)
    monkeypatch.setattr(ops, "_encoder_forward_impl", forward_impl)
