"""Cases of the CLIP image tower and the 2-D metrics (panic3d_amd/clip.py, metrics.psnr, include/p3d_clip.h), shared by
tests/test_clip_cpu.py and tests/test_hip_clip.py:

  * a restatement of every stage and of the whole network in plain torch, generic in the number format: float64 is the reference,
    binary32 on the CPU the yardstick the device's error is measured against (LayerNorm, attention, the whole network, the similarity:
    ours <= 4 x torch's, per case);
  * a numpy restatement of Pillow's 8-bit bicubic resize (integer arithmetic) and of clip's whole preprocessing;
  * binary32 stand-ins of the device operators (`TorchOps`, install_ops(monkeypatch, ops)) for CPU runs of the host wiring, with
    seedable faults so that the tests can show that the gates notice them;
  * the gates, as functions that return a list of complaints, and the case lists.

The GEMM's gate is the project's standing one (loss_cases.gate): per value 8 sqrt(K) 2^-24 sum|terms| and rel-L2 <= 1e-5, where the
terms are the K products, the bias and the residual.  With QuickGELU g(v) = v sigmoid(1.702 v) between the sum and the residual the
bound is carried through g: |g'| <= 1.1 everywhere (its maximum is 1.0998 at v = 1.44), so an error t in v becomes at most 1.1 t in
g(v), and g's own evaluation (a product, an exp, an addition, a division, a product) adds a few 2^-24 |g(v)|; hence
sum|terms| := 1.1 (sum|a w| + |bias|) + |g(v)| + |res| with one more term counted in K.
"""
import math

import numpy as np
import torch

import loss_cases as LC

F = torch.nn.functional
MEAN = (0.48145466, 0.4578275, 0.40821073)
STD = (0.26862954, 0.26130258, 0.27577711)
EPS = 1e-5
EPS32 = 2.0 ** -24
rel_l2 = LC.rel_l2
gate = LC.gate


# ---- Pillow's 8-bit bicubic resize, restated ------------------------------------------------------------------------------------------
def _cubic(t):
    a = -0.5
    t = abs(t)
    if t < 1.0:
        return ((a + 2.0) * t - (a + 3.0)) * t * t + 1.0
    if t < 2.0:
        return (((t - 5.0) * t + 8.0) * t - 4.0) * a
    return 0.0


def pil_table(n_in, n_out):
    """Per output: (xmin, [k]) with k = PIL's fixed-point coefficients (22 fractional bits)."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 2.0 * fs
    out = []
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in)
        w = [_cubic((x + xmin - center + 0.5) * (1.0 / fs)) for x in range(xmax - xmin)]
        ww = 0.0
        for v in w:
            ww += v
        w = [v / ww if ww != 0.0 else v for v in w]
        out.append((xmin, [int(-0.5 + v * (1 << 22)) if v < 0 else int(0.5 + v * (1 << 22)) for v in w]))
    return out


def table_matrix(n_in, n_out):
    m = np.zeros((n_out, n_in), dtype=np.int64)
    for xx, (xmin, k) in enumerate(pil_table(n_in, n_out)):
        m[xx, xmin:xmin + len(k)] = k
    return m


def resize_u8(q, h, w, fault=None):
    """q uint8 [..., H, W] -> uint8 [..., h, w]: the horizontal pass, then the vertical pass over its uint8 result.
    fault 'no_round': the rounding constant 2^21 left out."""
    half = 0 if fault == "no_round" else 1 << 21
    H, W = q.shape[-2:]
    t = np.clip((q.astype(np.int64) @ table_matrix(W, w).T + half) >> 22, 0, 255)
    t = np.clip((np.swapaxes(t, -1, -2) @ table_matrix(H, h).T + half) >> 22, 0, 255)
    return np.swapaxes(t, -1, -2).astype(np.uint8)


def resize_hw(H, W, S):
    return (int(S * H / W), S) if W <= H else (S, int(S * W / H))


def crop_offset(size, S):
    return int(round((size - S) / 2.0))


def quantise(img):
    """to_pil_image(x.float().clamp(0, 1)): byte(x * 255), in binary32.  -> uint8 numpy [N,3,H,W]"""
    return torch.floor(img[:, :3].float().clamp(0, 1) * 255.0).to(torch.uint8).numpy()


def preprocess_u8(img, S, fault=None):
    """clip's Resize(S, BICUBIC) + CenterCrop(S) of the quantised image: uint8 numpy [N,3,S,S].  fault 'crop': the offset off by one."""
    q = quantise(img)
    h, w = resize_hw(q.shape[2], q.shape[3], S)
    r = resize_u8(q, h, w, fault)
    oy, ox = crop_offset(h, S), crop_offset(w, S)
    if fault == "crop":
        oy, ox = (oy + 1 if h > S else oy), (ox + 1 if w > S else ox)
        r = np.pad(r, ((0, 0), (0, 0), (0, 1), (0, 1)), mode="edge")
    return np.ascontiguousarray(r[:, :, oy:oy + S, ox:ox + S])


def preprocess_from_tables(img, tabx, taby, fault=None):
    """The front end's integer sums as the kernels form them, from the library's tables (int32 [S, 2 + ksize]: xmin, n, k...) of the S kept
    columns and rows: quantise, horizontal pass, vertical pass, normalise.  fault 'no_round': the rounding constant left out."""
    q = quantise(img).astype(np.int64)
    half = 0 if fault == "no_round" else 1 << 21

    def dense(tab, n_in):
        m = np.zeros((tab.shape[0], n_in), dtype=np.int64)
        for i, row in enumerate(tab):
            m[i, row[0]:row[0] + row[1]] = row[2:2 + row[1]]
        return m
    t = np.clip((q @ dense(tabx, q.shape[3]).T + half) >> 22, 0, 255)
    t = np.clip((np.swapaxes(t, -1, -2) @ dense(taby, q.shape[2]).T + half) >> 22, 0, 255)
    return normalise(np.ascontiguousarray(np.swapaxes(t, -1, -2)).astype(np.uint8))


def pil_preprocess_u8(img, S):
    """The same through Pillow itself: Image.resize(BICUBIC) and crop."""
    from PIL import Image
    q = quantise(img)
    out = []
    for n in range(q.shape[0]):
        im = Image.fromarray(np.ascontiguousarray(q[n].transpose(1, 2, 0)), "RGB")
        h, w = resize_hw(q.shape[2], q.shape[3], S)
        im = im.resize((w, h), Image.BICUBIC)
        oy, ox = crop_offset(h, S), crop_offset(w, S)
        out.append(np.asarray(im.crop((ox, oy, ox + S, oy + S))).transpose(2, 0, 1))
    return np.stack(out)


def normalise(u8, dtype=torch.float32):
    """ToTensor + Normalize with torchvision's operations: v / 255, - mean, / std, mean and std binary32 values."""
    mean, std = (torch.tensor(v, dtype=torch.float32).to(dtype).view(1, 3, 1, 1) for v in (MEAN, STD))
    return (torch.from_numpy(u8).to(dtype) / 255.0 - mean) / std


def denormalise(x):
    """The 8-bit value an output of the front end was made from: exact, the levels are 1 / (255 std) ~ 0.0146 apart."""
    mean, std = (torch.tensor(v, dtype=torch.float64).view(1, 3, 1, 1) for v in (MEAN, STD))
    return torch.round((x.double().cpu() * std + mean) * 255.0).to(torch.int64).numpy()


def preprocess(img, S, dtype=torch.float32, fault=None):
    return normalise(preprocess_u8(img, S, fault), dtype)


# (H, W) -> S: the sizes the numpy restatement was matched with Pillow at, plus an upscale-and-crop and an identity
RESIZE_CASES = (((301, 187), 224), ((187, 301), 224), ((512, 512), 224), ((97, 640), 224), ((224, 224), 224), ((230, 225), 224), ((40, 33), 224),
                ((33, 40), 64), ((64, 64), 64))


def image_case(hw, seed=0, levels=True, batch=1, channels=3):
    """levels: values k / 255 (which the quantisation maps back to k); else arbitrary floats in [-0.2, 1.2]."""
    g = torch.Generator().manual_seed(seed + 1000 * hw[0] + hw[1])
    if levels:
        return torch.randint(0, 256, (batch, channels, hw[0], hw[1]), generator=g).float() / 255.0
    return torch.rand(batch, channels, hw[0], hw[1], generator=g) * 1.4 - 0.2


def prepare_gate(name, ours, img, S, verbose=True):
    """The integers equal Pillow's exactly; the normalised value within 2 2^-24 |value| of torchvision's binary32 arithmetic."""
    want = pil_preprocess_u8(img, S)
    bad = []
    if tuple(ours.shape) != want.shape:
        return [f"{name}: shape {tuple(ours.shape)}"]
    got = denormalise(ours)
    n = int((got != want).sum())
    ref = normalise(want)
    r = float(((ours.cpu() - ref).abs() / (2 * EPS32 * ref.abs()).clamp_min(1e-300)).max())
    if verbose:
        print(f"clip prepare {name}: {n} of {want.size} integers differ from Pillow's (worst {int(np.abs(got - want).max())}), normalisation ratio {r:.3f}")
    if n:
        bad.append(f"{name}: {n} integers differ from Pillow's")
    if not r <= 1.0:
        bad.append(f"{name}: normalisation ratio {r:.3g}")
    return bad


# ---- the stages, generic in dtype -----------------------------------------------------------------------------------------------------
def quick_gelu(v):
    return v * torch.sigmoid(1.702 * v)


def layernorm(x, gamma, beta, eps=EPS, fault=None):
    """fault 'one_pass': the variance as E[x^2] - mean^2."""
    mean = x.mean(-1, keepdim=True)
    var = (x * x).mean(-1, keepdim=True) - mean * mean if fault == "one_pass" else ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * gamma + beta


def attention(qkv, N, T, heads, fault=None):
    """qkv [N T, 3 D] -> [N T, D].  faults: 'no_max' (exp without subtracting the maximum), 'no_scale' (the 0.125 missing), 'kv_swap'."""
    D = qkv.shape[1] // 3
    q, k, v = (t.reshape(N, T, heads, 64).transpose(1, 2) for t in qkv.reshape(N, T, 3 * D).split(D, dim=2))
    if fault == "kv_swap":
        k, v = v, k
    s = q @ k.transpose(-1, -2)
    if fault != "no_scale":
        s = s * 0.125
    if fault == "no_max":
        p = torch.exp(s)
        p = p / p.sum(-1, keepdim=True)
    else:
        p = torch.softmax(s, dim=-1)
    return (p @ v).transpose(1, 2).reshape(N * T, D)


def embed(patches, cls, pos, N, gamma, beta, fault=None):
    """fault 'pos_after_ln': the positional embedding added after ln_pre."""
    T, D = pos.shape
    x = torch.cat([cls.expand(N, 1, D), patches.reshape(N, T - 1, D)], dim=1)
    if fault == "pos_after_ln":
        return (layernorm(x, gamma, beta) + pos).reshape(N * T, D)
    return layernorm(x + pos, gamma, beta).reshape(N * T, D)


def cosine(a, b):
    return (a * b).sum(-1) / (a.norm(dim=-1) * b.norm(dim=-1))


def psnr64(pred, target, data_range=None):
    p, t = pred.double(), target.double()
    rng = float(data_range) if data_range is not None else float(t.max() - t.min())
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(10.0 * np.log10(np.float64(rng * rng) / np.float64(((p - t) ** 2).mean())))


# ---- the whole network ----------------------------------------------------------------------------------------------------------------
TINY1 = dict(width=128, layers=2, heads=2, image_size=64, patch_size=32, output_dim=32)
TINY2 = dict(width=192, layers=1, heads=3, image_size=96, patch_size=32, output_dim=48)
FULL = dict(width=768, layers=12, heads=12, image_size=224, patch_size=32, output_dim=512)


def make_weights(width, layers, heads, image_size, patch_size, output_dim, seed=0):
    """A seeded state dict under OpenAI's names (binary32), every matrix scaled by its fan-in so that activations stay O(1), LayerNorm
    gains around 1 and small non-zero biases everywhere."""
    g = torch.Generator().manual_seed(seed)
    D, T = width, 1 + (image_size // patch_size) ** 2
    rn = lambda *s: torch.randn(*s, generator=g)
    sd = {"conv1.weight": rn(D, 3, patch_size, patch_size) / math.sqrt(3 * patch_size ** 2), "class_embedding": rn(D), "positional_embedding": rn(T, D) * 0.5}

    def ln(name):
        sd[f"{name}.weight"], sd[f"{name}.bias"] = 0.75 + 0.5 * torch.rand(D, generator=g), rn(D) * 0.1

    def lin(name, Ci, Co):
        sd[f"{name}.weight"], sd[f"{name}.bias"] = rn(Co, Ci) / math.sqrt(Ci), rn(Co) * 0.1
    ln("ln_pre")
    for i in range(layers):
        b = f"transformer.resblocks.{i}"
        ln(f"{b}.ln_1"), ln(f"{b}.ln_2")
        sd[f"{b}.attn.in_proj_weight"], sd[f"{b}.attn.in_proj_bias"] = rn(3 * D, D) * (2.0 / math.sqrt(D)), rn(3 * D) * 0.1
        lin(f"{b}.attn.out_proj", D, D), lin(f"{b}.mlp.c_fc", D, 4 * D), lin(f"{b}.mlp.c_proj", 4 * D, D)
    ln("ln_post")
    sd["proj"] = rn(D, output_dim) / math.sqrt(D)
    return sd


def network(sd, x, heads, dtype, fault=None):
    """clip/model.py's VisionTransformer.forward on the state dict `sd` in `dtype`: x [N,3,S,S] preprocessed -> [N,output_dim]."""
    t = lambda name: sd[name].to(dtype)
    ln = lambda v, name: layernorm(v, t(name + ".weight"), t(name + ".bias"))
    w = t("conv1.weight")
    D, patch = w.shape[0], w.shape[-1]
    N = x.shape[0]
    p = F.conv2d(x.to(dtype), w, stride=patch).reshape(N, D, -1).permute(0, 2, 1)
    T = p.shape[1] + 1
    v = embed(p.reshape(-1, D), t("class_embedding"), t("positional_embedding"), N, t("ln_pre.weight"), t("ln_pre.bias"), fault=fault)
    i = 0
    while f"transformer.resblocks.{i}.ln_1.weight" in sd:
        b = f"transformer.resblocks.{i}"
        qkv = F.linear(ln(v, f"{b}.ln_1"), t(f"{b}.attn.in_proj_weight"), t(f"{b}.attn.in_proj_bias"))
        v = v + F.linear(attention(qkv, N, T, heads, fault=fault), t(f"{b}.attn.out_proj.weight"), t(f"{b}.attn.out_proj.bias"))
        f = F.linear(ln(v, f"{b}.ln_2"), t(f"{b}.mlp.c_fc.weight"), t(f"{b}.mlp.c_fc.bias"))
        f = F.gelu(f) if fault == "gelu" else quick_gelu(f)
        v = v + F.linear(f, t(f"{b}.mlp.c_proj.weight"), t(f"{b}.mlp.c_proj.bias"))
        i += 1
    return ln(v.reshape(N, T, D)[:, 0], "ln_post") @ t("proj")


# name -> (architecture, N, source (H, W))
NETWORK_CASES = {"tiny1": (TINY1, 3, (80, 70)), "tiny2": (TINY2, 1, (96, 96)), "full": (FULL, 2, (256, 256))}
_NETWORK_REF = {}


def network_case(name):
    """The case's weights, images, preprocessed batch, float64 reference and binary32 CPU restatement: computed once, shared, unchanged."""
    if name not in _NETWORK_REF:
        arch, N, hw = NETWORK_CASES[name]
        sd = make_weights(seed=21 + len(name), **arch)
        img = image_case(hw, seed=3, levels=False, batch=N, channels=4)
        x = preprocess(img, arch["image_size"])
        with torch.no_grad():
            f64, f32 = network(sd, x, arch["heads"], torch.float64), network(sd, x, arch["heads"], torch.float32)
        _NETWORK_REF[name] = dict(arch=arch, N=N, sd=sd, img=img, x=x, f64=f64, f32=f32)
    return _NETWORK_REF[name]


def ratio_gate(name, ours, f64, f32, factor=4.0, verbose=True, kinds=("max", "l2")):
    """ours <= factor x torch's binary32 error against float64, in max-abs and in rel-L2 (a non-finite value fails).  -> violations"""
    ours = torch.as_tensor(ours).double().cpu().reshape(f64.shape)
    bad = []
    m, m32 = float((ours - f64).abs().max()), float((f32.double() - f64).abs().max())
    e, e32 = rel_l2(ours, f64), rel_l2(f32, f64)
    if verbose:
        print(f"clip {name}: max-abs ours {m:.3e}, torch32 {m32:.3e}; rel-L2 ours {e:.3e}, torch32 {e32:.3e}")
    if "max" in kinds and not m <= factor * m32:
        bad.append(f"{name}: max-abs {m:.3g} > {factor} * {m32:.3g}")
    if "l2" in kinds and not e <= factor * e32:
        bad.append(f"{name}: rel-L2 {e:.3g} > {factor} * {e32:.3g}")
    return bad


def network_gate(name, ours, c, verbose=True):
    return ratio_gate(f"network {name}", ours, c["f64"], c["f32"], verbose=verbose, kinds=("l2",))


# ---- stage cases ----------------------------------------------------------------------------------------------------------------------
GEMM_SHAPES = ((1, 4, 1), (5, 64, 64), (50, 100, 70), (67, 192, 130), (100, 768, 96))
EPILOGUES = tuple((b, g, r) for b in (False, True) for g in (False, True) for r in (False, True))
# every plan: both tiles, without a split, with two, with as many as there are chunks (want is clipped to the chunk count)
PLANS = (0,) + tuple((tile << 8) | want for tile in (1, 2) for want in (1, 2, 255))
PATCH_CASES = ((2, 64, 32, 40), (1, 96, 32, 70), (3, 32, 16, 24))  # (N, image, patch, width)


def gemm_case(shape, seed=0):
    M, K, Nout = shape
    g = torch.Generator().manual_seed(seed + M * 7 + K * 3 + Nout)
    return dict(a=torch.randn(M, K, generator=g), w=torch.randn(K, Nout, generator=g) / math.sqrt(K), bias=torch.randn(Nout, generator=g) * 0.5,
                res=torch.randn(M, Nout, generator=g), shape=shape)


def gemm_ref(c, bias, gelu, res, dtype=torch.float64, fault=None):
    """(y, sum|terms|, terms): see the module docstring for the QuickGELU form.  fault 'bias_per_split': the bias added twice."""
    a, w = c["a"].to(dtype), c["w"].to(dtype)
    v, s, K = a @ w, a.abs() @ w.abs(), c["shape"][1]
    if bias:
        v, s, K = v + c["bias"].to(dtype) * (2 if fault == "bias_per_split" else 1), s + c["bias"].to(dtype).abs(), K + 1
    if gelu:
        v = F.gelu(v) if fault == "gelu" else quick_gelu(v)
        s, K = 1.1 * s + v.abs(), K + 1
    if res and fault != "no_res":
        v = v + c["res"].to(dtype)
    if res:
        s, K = s + c["res"].to(dtype).abs(), K + 1
    return v, s, K


def run_gemm(ops, c, bias, gelu, res, device, plan=0):
    d = lambda t: t.to(device)
    return ops.clip_gemm(d(c["a"]), d(c["w"]), d(c["bias"]) if bias else None, d(c["res"]) if res else None, gelu, 0, plan)


def patch_case(N, S, patch, width, seed=0):
    g = torch.Generator().manual_seed(seed + S + patch)
    x, w = torch.randn(N, 3, S, S, generator=g), torch.randn(width, 3, patch, patch, generator=g) / math.sqrt(3 * patch * patch)
    y = F.conv2d(x.double(), w.double(), stride=patch).reshape(N, width, -1).permute(0, 2, 1).reshape(-1, width)
    s = F.conv2d(x.double().abs(), w.double().abs(), stride=patch).reshape(N, width, -1).permute(0, 2, 1).reshape(-1, width)
    return dict(x=x, w=w, wk=w.reshape(width, -1).t().contiguous(), y=y, y_abs=s, K=3 * patch * patch, patch=patch)


LN_D, LN_M = (64, 100, 192, 768), (1, 5, 67)


def ln_case(M, D, kind="plain", seed=0):
    """kinds: 'plain'; 'offset' (mean 1e3, spread 1); 'constant' (every row constant 1.25: a value whose sums are exact in binary32, so
    the mean is exact, every deviation is 0 and the output is beta)."""
    g = torch.Generator().manual_seed(seed + M * 1000 + D)
    x = torch.randn(M, D, generator=g)
    if kind == "offset":
        x = x + 1000.0
    if kind == "constant":
        x = torch.full((M, D), 1.25)
    return dict(x=x, gamma=0.75 + 0.5 * torch.rand(D, generator=g), beta=torch.randn(D, generator=g) * 0.1)


def ln_gate(name, ours, c, x=None, verbose=True):
    x = c["x"] if x is None else x
    t = lambda v, dt: v.to(dt)
    f64 = layernorm(t(x, torch.float64), t(c["gamma"], torch.float64), t(c["beta"], torch.float64))
    f32 = F.layer_norm(x, (x.shape[-1],), c["gamma"], c["beta"], EPS)
    return ratio_gate(f"layernorm {name}", ours, f64, f32, verbose=verbose)


ATTN_T, ATTN_HEADS, ATTN_N = (1, 2, 5, 17, 50, 64), (1, 3), (1, 3)


def attn_case(N, T, heads, kind="plain", seed=0):
    """kinds: 'plain'; 'pm80' (logits of +-80: q = k rows of +-sqrt(10), so that 0.125 q.k = +-80; binary32's exp does not overflow there —
    e^80 = 5.5e34 — but the probabilities span 69 orders of magnitude); 'pm120' (logits of +-120, where exp DOES overflow without the
    maximum); 'dominant' (one key 30 above the others for every query)."""
    g = torch.Generator().manual_seed(seed + N * 10000 + T * 100 + heads)
    D = 64 * heads
    qkv = torch.randn(N * T, 3 * D, generator=g)
    if kind in ("pm80", "pm120"):
        amp = math.sqrt(10.0 if kind == "pm80" else 15.0)
        sign = (torch.randint(0, 2, (N * T, 1), generator=g).float() * 2 - 1)
        qkv[:, :D] = amp * sign
        qkv[:, D:2 * D] = amp * (torch.randint(0, 2, (N * T, 1), generator=g).float() * 2 - 1)
    if kind == "dominant":
        qkv[:, :D] = 1.0
        qkv[:, D:2 * D] = torch.randn(N * T, D, generator=g) * 0.1
        qkv.view(N, T, 3 * D)[:, T // 2, D:2 * D] += 30.0 * 8.0 / 64.0
    return dict(qkv=qkv, N=N, T=T, heads=heads)


def attn_gate(name, ours, c, verbose=True):
    f64 = attention(c["qkv"].double(), c["N"], c["T"], c["heads"])
    f32 = attention(c["qkv"], c["N"], c["T"], c["heads"])
    return ratio_gate(f"attention {name}", ours, f64, f32, verbose=verbose)


PSNR_SHAPES = ((1, 3, 7, 5), (2, 3, 64, 64), (1, 3, 301, 187))


def psnr_case(shape, seed=0):
    g = torch.Generator().manual_seed(seed + shape[-1])
    target = torch.rand(*shape, generator=g) * 0.9 + 0.05
    return dict(pred=(target + 0.05 * torch.randn(*shape, generator=g)).clamp(0, 1), target=target)


# ---- binary32 stand-ins of the device operators ---------------------------------------------------------------------------------------
class TorchOps:
    """The _impl operators' signatures on binary32 torch arithmetic, with seedable faults."""
    fault = None

    @staticmethod
    def prepare(img, S):
        return preprocess(img, S, fault=TorchOps.fault)

    @staticmethod
    def gemm(a, w, bias, res, gelu, patch, force_plan, out=None):
        if patch:
            a = F.unfold(a, patch, stride=patch).permute(0, 2, 1).reshape(-1, w.shape[0])
        v = a @ w
        if bias is not None:
            v = v + bias
        if gelu:
            v = F.gelu(v) if TorchOps.fault == "gelu" else quick_gelu(v)
        if res is not None:
            v = res + v
        if out is not None:
            out.copy_(v)
            return out
        return v

    @staticmethod
    def layernorm(x, rows, D, ld, gamma, beta, eps):
        return layernorm(x.reshape(-1).as_strided((rows, D), (ld, 1)), gamma, beta, eps, fault=TorchOps.fault)

    @staticmethod
    def embed(patches, cls, pos, N, gamma, beta, eps):
        return embed(patches, cls, pos, N, gamma, beta, fault=TorchOps.fault)

    @staticmethod
    def attention(qkv, N, T, heads):
        return attention(qkv, N, T, heads, fault=TorchOps.fault)

    @staticmethod
    def cosine(a, b):
        return cosine(a, b)

    @staticmethod
    def psnr_sums(pred, target):
        return torch.stack([((pred - target) ** 2).sum(), target.min(), target.max()])


def install_ops(monkeypatch, ops, fault=None):
    """Replace the device operators of panic3d_amd.ops by the binary32 stand-ins (CPU runs of the host wiring)."""
    T = TorchOps
    monkeypatch.setattr(T, "fault", fault)

    def forward_impl(prog):
        W = prog.weights
        blob = lambda off, *shape: W[off:off + math.prod(shape)].view(*shape)
        for r in prog.records:
            k = r["kind"]
            if k == "prepare":
                y = T.prepare(prog.buffer(r["src"], (r["N"], r["K"], r["H"], r["W"])), r["S"])
            elif k == "gemm":
                src = prog.buffer(r["src"], (r["N"], 3, r["S"], r["S"]) if r.get("patch") else (r["M"], r["K"]))
                res = prog.buffer(r["res"], (r["M"], r["Nout"])) if r.get("res") is not None else None
                y = T.gemm(src, blob(r["w"], r["K"], r["Nout"]), blob(r["b"], r["Nout"]) if r.get("b") is not None else None, res, r.get("gelu"),
                           r.get("patch", 0), 0)
            elif k == "layernorm":
                y = T.layernorm(prog.arena[prog.buf_off[r["src"]]:], r["M"], r["K"], r["ld"], blob(r["w"], r["K"]), blob(r["b"], r["K"]), r["eps"])
            elif k == "embed":
                y = T.embed(prog.buffer(r["src"], (r["N"] * (r["T"] - 1), r["K"])), blob(r["w2"], r["K"]), blob(r["b2"], r["T"], r["K"]), r["N"],
                            blob(r["w"], r["K"]), blob(r["b"], r["K"]), r["eps"])
            else:
                y = T.attention(prog.buffer(r["src"], (r["M"], r["K"])), r["N"], r["T"], r["heads"])
            prog.buffer(r["dst"], tuple(y.shape)).copy_(y)

    monkeypatch.setattr(ops, "_clip_prepare_impl", T.prepare)
    monkeypatch.setattr(ops, "_clip_gemm_impl", T.gemm)
    monkeypatch.setattr(ops, "_clip_layernorm_impl", T.layernorm)
    monkeypatch.setattr(ops, "_clip_embed_impl", T.embed)
    monkeypatch.setattr(ops, "_clip_attention_impl", T.attention)
    monkeypatch.setattr(ops, "_clip_cosine_impl", T.cosine)
    monkeypatch.setattr(ops, "_psnr_sums_impl", T.psnr_sums)
    monkeypatch.setattr(ops, "_clip_forward_impl", forward_impl)
