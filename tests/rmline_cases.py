"""The illustration-to-render module's reference, cases, gates and stand-ins (tests/test_hip_rmline.py, tests/test_rmline_cpu.py).

The reference is restated here in torch, float64 unless a dtype is given, with line citations of the reference tree:
  _util/sketchers_v2.py:64-83           batch_dog: grey, two Gaussian blurs with a replicate border, 0.5 + t (g1 - g0) - epsilon, clip
  _train/img2img/util/rmline_wrapper.py:15-50   the wrapper: composite on white, dog > 0.5, dilation by ones(2, 2), & ~hull, model, lerp
  _train/img2img/models/rmlineganA.py:57-143    the generator's nn.Sequential and its forward (mask, cat, replicate pad)
The reference modules themselves cannot be imported here (pytorch_lightning, kornia and skimage are absent), so kornia's two functions
are restated too: gaussian_blur2d as weights exp(-x^2 / 2 sigma^2) / sum over x = -(k/2) .. k/2 applied along both axes of the
replicate-padded image, and morphology.dilation by ones(d, d) at kornia 0.6.5's defaults as the maximum over the in-bounds window with
origin d // 2 (what panic3d_amd.loss.dilation also restates).  Neither is pinned against kornia.

The generator is the literal nn.Sequential of rmlineganA.py:65-82, built from torch's own nn.Conv2d, nn.LeakyReLU, nn.BatchNorm2d and
nn.Tanh in eval mode with seeded non-trivial weights and running statistics.
"""
import math

import torch

F = torch.nn.functional
U = 2.0 ** -24

DOG_WRAPPER = dict(t=1.0, sigma=0.5, k=1.6, epsilon=0.01, kernel_factor=4)  # rmline_wrapper.py:24-33: 5 and 7 taps
DOG_WIDE = dict(t=2.0, sigma=1.0, k=1.6, epsilon=0.01, kernel_factor=4)     # batch_dog's own defaults: 9 and 13 taps
DOGS = {"wrapper": DOG_WRAPPER, "wide": DOG_WIDE}
MASK_TILE = (8, 32)   # k_rm_mask's tile
CONV_TILE = (8, 32)   # k_rm_conv's larger tile (the smaller one has 4 rows)
DEFAULT_ARCH = dict(gen_depth=6, gen_width=32, gen_batchnorm=True, gen_use_hull=True, gen_mask_input=True)
SMALL_ARCH = dict(gen_depth=2, gen_width=8, gen_batchnorm=False, gen_use_hull=False, gen_mask_input=False)
ARCHS = {"default": DEFAULT_ARCH, "small": SMALL_ARCH}


def rel_l2(a, b):
    a, b = a.double(), b.double()
    den = float(b.norm())
    return float((a - b).norm()) / den if den > 0 else float((a - b).norm())


# ---- batch_dog, the dilation, the mask ---------------------------------------------------------------------------------------------------
def taps(sigma, k, kernel_factor, **_):
    return max(2 * int(sigma * kernel_factor) + 1, 3), max(2 * int(sigma * k * kernel_factor) + 1, 3)  # sketchers_v2.py:72-73


def gauss_weights(n, sigma, dtype=torch.float64):
    x = torch.arange(n, dtype=torch.float64) - n // 2
    w = torch.exp(-x * x / (2.0 * sigma * sigma))
    return (w / w.sum()).to(dtype)


def gaussian_blur(x, n, sigma, border="replicate"):
    """kornia.filters.gaussian_blur2d(x, (n, n), (sigma, sigma), border_type='replicate') on [N,1,H,W]."""
    w = gauss_weights(n, sigma, x.dtype).to(x.device)
    r = n // 2
    x = F.pad(x, (r, r, r, r), mode=border) if border != "zeros" else F.pad(x, (r, r, r, r))
    return F.conv2d(F.conv2d(x, w.view(1, 1, 1, n)), w.view(1, 1, n, 1))


def composite(img):
    """img.bg('w').convert('RGB') (rmline_wrapper.py:20): RGBA on white; other channel counts pass."""
    return img[:, :3] * img[:, 3:4] + (1 - img[:, 3:4]) if img.shape[1] == 4 else img


def grey(img):
    if img.shape[1] == 1:
        return img
    return 0.299 * img[:, 0:1] + 0.587 * img[:, 1:2] + 0.114 * img[:, 2:3]  # kornia.color.rgb_to_grayscale


def batch_dog(img, t=2.0, sigma=1.0, k=1.6, epsilon=0.01, kernel_factor=4, clip=True, fault=None):
    """sketchers_v2.py:64-83 on the composited image (the wrapper composites before it calls batch_dog)."""
    g = grey(composite(img))
    k0, k1 = taps(sigma, k, kernel_factor)
    border = "zeros" if fault == "zero_pad" else "replicate"
    g0, g1 = gaussian_blur(g, k0, sigma, border), gaussian_blur(g, k1, sigma * k, border)
    ans = 0.5 + t * ((g0 - g1) if fault == "g0-g1" else (g1 - g0)) - epsilon
    return ans.clip(0, 1) if clip else ans


def response_bound(img, t=2.0, sigma=1.0, k=1.6, epsilon=0.01, kernel_factor=4, **_):
    """The response's gate per value: 8 sqrt(K) 2^-24 sum|terms| with K = 3 + 2 (k0 + k1) products (the grey's three, and each blur's
    taps along both axes); sum|terms| = 0.5 + |t| (g1 + g0 of the absolute values) + |epsilon|."""
    a = grey(composite(img.double().abs()))
    k0, k1 = taps(sigma, k, kernel_factor)
    terms = 0.5 + abs(t) * (gaussian_blur(a, k0, sigma) + gaussian_blur(a, k1, sigma * k)) + abs(epsilon)
    return 8.0 * math.sqrt(3 + 2 * (k0 + k1)) * U * terms


def dilation(x, d, fault=None):
    """kornia.morphology.dilation(x, ones(d, d)) at 0.6.5's defaults: origin d // 2, geodesic border (-inf outside)."""
    o = 0 if fault == "window_forward" else d // 2
    return F.max_pool2d(F.pad(x, [o, d - o - 1, o, d - o - 1], value=float("-inf")), d, stride=1)


def line_mask(img, hull=None, dog=DOG_WRAPPER, d=2, fault=None):
    """rmline_wrapper.py:24-41 -> float64 [N,1,H,W] of 0 / 1."""
    m = (batch_dog(img.double(), fault=fault if fault in ("zero_pad", "g0-g1") else None, **dog) > 0.5).double()
    if d > 1:
        m = dilation(m, d, fault)
    if hull is not None:
        m = m * (hull == 0)
    return m


def uncertain(img, dog=DOG_WRAPPER, d=2):
    """bool [N,1,H,W]: the pixels whose mask a binary32 run may decide differently — some response in the pixel's dilation window lies
    within the response's gate of the threshold."""
    close = ((batch_dog(img.double(), **dog) - 0.5).abs() <= response_bound(img, **dog)).double()
    return (dilation(close, d) if d > 1 else close) > 0


def mask_gate(name, ours, img, hull, dog, d, verbose=True, fault_ref=None):
    """The mask equals float64's on every pixel outside `uncertain`; at most 1 % of the pixels may be left out.  -> violations."""
    ref = line_mask(img, hull, dog, d) if fault_ref is None else fault_ref
    unc = uncertain(img, dog, d)
    share = float(unc.double().mean())
    wrong = int(((ours.double().cpu() != ref) & ~unc).sum())
    if verbose:
        print(f"{name}: {wrong} wrong pixels, {share:.4%} left out, mask mean {float(ref.mean()):.3f}")
    return ([f"{name}: {wrong} pixels differ from float64"] if wrong else []) + ([f"{name}: {share:.3%} of the pixels left out"] if share > 0.01 else [])


def smooth_image(N, C, H, W, seed, strokes=True):
    """A seeded smooth-noise image in [0, 1] with dark drawn strokes (and, for C = 4, a smooth alpha), on 8-bit levels like a file's."""
    g = torch.Generator().manual_seed(seed * 7919 + N * 1000003 + C * 10007 + H * 101 + W)
    low = torch.rand(N, C, max(H // 4, 1) + 1, max(W // 4, 1) + 1, generator=g)
    img = F.interpolate(low, size=(H, W), mode="bilinear", align_corners=True) * 0.6 + 0.3
    if strokes:
        for n in range(N):
            for _ in range(3):
                y, x = int(torch.randint(0, H, (1,), generator=g)), int(torch.randint(0, W, (1,), generator=g))
                if int(torch.randint(0, 2, (1,), generator=g)):
                    img[n, :min(C, 3), y, :] = 0.05
                else:
                    img[n, :min(C, 3), :, x] = 0.05
    return (img * 255).round() / 255


def flat_image(N, C, H, W):
    """Flat regions and one hard vertical edge at the middle column (C = 4: opaque)."""
    img = torch.full((N, C, H, W), 0.75)
    img[..., W // 2:] = 0.125
    if C == 4:
        img[:, 3] = 1.0
    return img


def make_hull(N, H, W):
    """A rectangle around the middle (non-zero inside; 2.0, not 1.0: `.bool()` is what the wrapper applies)."""
    h = torch.zeros(N, 1, H, W)
    h[:, :, H // 4:H // 2 + 1, W // 4:W // 2 + 1] = 2.0
    return h


RESPONSE_SHAPES = [(1, 1), (3, 3), (5, 7), (33, 31), (MASK_TILE[0] + 1, MASK_TILE[1] + 1), (1, 70)]
MASK_SHAPES = [(5, 7), (33, 31), (MASK_TILE[0] + 1, MASK_TILE[1] + 1), (1, 70)]


# ---- one layer ---------------------------------------------------------------------------------------------------------------------------
CONV_CHANNELS = [(4, 32), (32, 32), (32, 3), (5, 7), (64, 64)]
CONV_SHAPES = [(3, 3), (4, 9), (19, 35), (CONV_TILE[0] + 3, CONV_TILE[1] + 3)]
ACTS = {"none": lambda z, s: z, "leaky": lambda z, s: torch.where(z > 0, z, z * s), "tanh": lambda z, s: torch.tanh(z)}
_CONV = {}


def to_wk(w):
    Co, Ci = w.shape[:2]
    return w.permute(2, 3, 1, 0).reshape(9, Ci, Co).contiguous()


def conv_case(Ci, Co, H, W, N=2):
    """x [N,Ci,H,W], w [Co,Ci,3,3], b [Co] in binary32; z: float64's convolution; z_abs: its sum|terms|.  Computed once, left unchanged."""
    key = (Ci, Co, H, W, N)
    if key not in _CONV:
        g = torch.Generator().manual_seed(Ci * 1009 + Co * 101 + H * 11 + W)
        x = torch.randn(N, Ci, H, W, generator=g)
        w = torch.randn(Co, Ci, 3, 3, generator=g) / math.sqrt(9 * Ci)
        b = torch.randn(Co, generator=g) * 0.5
        z = F.conv2d(x.double(), w.double(), b.double())
        z_abs = F.conv2d(x.double().abs(), w.double().abs(), b.double().abs())
        _CONV[key] = dict(name=f"conv {Ci}->{Co} {H}x{W}", x=x, w=w, b=b, z=z, z_abs=z_abs, K=9 * Ci + 1, slope=0.01)
    return _CONV[key]


def conv_gate(name, y, c, act, slope=0.01, verbose=True):
    """y [N,Co,Ho,Wo] against act(float64's z): per value 8 sqrt(K) 2^-24 sum|terms| with K = 9 Ci + 1 and sum|terms| of the
    convolution's own products and bias (the activations are 1-Lipschitz for slope <= 1: nothing is added for them); and
    rel-L2 <= 1e-5.  -> violations."""
    ref = ACTS[act](c["z"], slope)
    bound = 8.0 * math.sqrt(c["K"]) * U * c["z_abs"]
    ratio = float(((y.double().cpu() - ref).abs() / bound).max())
    rl2 = rel_l2(y.cpu(), ref)
    if verbose:
        print(f"{name} [{act}]: worst {ratio:.3f} of the bound, rel-L2 {rl2:.2e}")
    return ([f"{name} [{act}]: {ratio:.2f} x the bound"] if not ratio <= 1.0 else []) + ([f"{name} [{act}]: rel-L2 {rl2:.2e}"] if not rl2 <= 1e-5 else [])


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def nchw(y):
    return y.permute(0, 3, 1, 2).contiguous()


# ---- the generator and the wrapper -------------------------------------------------------------------------------------------------------
def make_generator(gen_depth=6, gen_width=32, gen_batchnorm=True, gen_use_hull=True, gen_mask_input=True, seed=1):
    """The literal nn.Sequential of rmlineganA.py:65-82 in float64, eval mode; seeded: running variances in [0.5, 2], means, gammas and
    betas non-trivial."""
    gen, chin, w = [], 3 + int(gen_use_hull), gen_width
    for i in range(gen_depth):
        gen.append(torch.nn.Conv2d(chin if i == 0 else w, w if i != gen_depth - 1 else 3, 3, stride=1, padding=0))
        if i != gen_depth - 1:
            gen.append(torch.nn.LeakyReLU())
            if gen_batchnorm:
                gen.append(torch.nn.BatchNorm2d(w))
    gen.append(torch.nn.Tanh())
    seq = torch.nn.Sequential(*gen).double().eval()
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in seq:
            if isinstance(m, torch.nn.Conv2d):
                m.weight.copy_(torch.randn(m.weight.shape, generator=g, dtype=torch.float64) * math.sqrt(2.0 / (9 * m.weight.shape[1])))
                m.bias.copy_(torch.randn(m.bias.shape, generator=g, dtype=torch.float64) * 0.2)
            elif isinstance(m, torch.nn.BatchNorm2d):
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=g, dtype=torch.float64) * 1.5 + 0.5)
                m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g, dtype=torch.float64) * 0.3 + 0.1)
                m.weight.copy_(torch.rand(m.weight.shape, generator=g, dtype=torch.float64) + 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g, dtype=torch.float64) * 0.2 - 0.05)
    return seq


def model_forward(seq, x, arch, pad=True, fault=None):
    """rmlineganA.py:105-143 (forward) on the dict x."""
    img, mask, fhull = x["image"], x["line_mask"], x["face_hull"]
    if arch["gen_mask_input"]:
        img = img * (1 - mask)
    stackin = torch.cat([img, fhull], dim=1) if arch["gen_use_hull"] else img
    if pad:
        p = (arch["gen_depth"],) * 4
        stackin = F.pad(stackin, p, mode="replicate") if fault != "zero_pad" else F.pad(stackin, p)
    return {"image": seq(stackin), "line_mask": mask, "face_hull": fhull}


def wrapper_forward(seq, img, hull, arch, dog=DOG_WRAPPER, d=2, dtype=torch.float64, fault=None):
    """rmline_wrapper.py:17-50 without its 8-bit round trips: (result with the input's alpha, mask).  The mask is float64's whatever
    the dtype: dtype is the precision of the Sequential, its input and the lerp."""
    mask = line_mask(img, hull, dog, d)
    image = composite(img.double())
    net = seq.to(dtype)
    xin = {"image": image.to(dtype), "line_mask": mask.to(dtype), "face_hull": hull.to(dtype)}
    with torch.no_grad():
        out = model_forward(net, xin, arch)["image"]
    seq.double()
    ans = torch.lerp(out, xin["image"], xin["line_mask"]) if fault == "lerp_swapped" else torch.lerp(xin["image"], out, xin["line_mask"])
    return (torch.cat([ans, img[:, 3:].to(dtype)], dim=1) if img.shape[1] == 4 else ans), mask


def state_dict_of(seq, discriminator=True):
    """The Lightning model's state_dict around the Sequential: generator.* (+ some discriminator.* entries to be ignored)."""
    sd = {f"generator.{k}": v.detach().clone() for k, v in seq.state_dict().items()}
    if discriminator:
        sd["discriminator.0.weight"], sd["discriminator.0.bias"] = torch.zeros(16, 4, 3, 3), torch.zeros(16)
    return sd


MODULE_SHAPES = [(1, 1), (7, 5), (37, 41)]
_MODULE = {}


def module_case(arch_name, hw, N=2):
    """A whole-module case: RGBA image, hull, the literal generator, float64's and binary32's wrapper results, and the same for the bare
    generator on a seeded random mask.  The image's seed is the first for which no pixel's mask is uncertain (so that float64's mask IS
    the mask).  Computed once, left unchanged."""
    key = (arch_name, hw)
    if key not in _MODULE:
        arch = ARCHS[arch_name]
        H, W = hw
        seq = make_generator(seed=3 + len(arch_name), **arch)
        hull = make_hull(N, H, W)
        for seed in range(20):
            img = smooth_image(N, 4, H, W, seed)
            if not bool(uncertain(img).any()):
                break
        else:
            raise AssertionError("no seed without an uncertain pixel")
        f64, mask = wrapper_forward(seq, img, hull, arch)
        f32, _ = wrapper_forward(seq, img, hull, arch, dtype=torch.float32)
        g = torch.Generator().manual_seed(H * 100 + W)
        x = {"image": smooth_image(N, 3, H, W, 99), "line_mask": (torch.rand(N, 1, H, W, generator=g) > 0.6).float(), "face_hull": (hull != 0).float()}
        with torch.no_grad():
            g64 = model_forward(seq, {k: v.double() for k, v in x.items()}, arch)["image"]
            g32 = model_forward(seq.float(), x, arch)["image"]
        seq.double()
        _MODULE[key] = dict(name=f"{arch_name} {H}x{W}", arch=arch, seq=seq, sd=state_dict_of(seq), img=img, hull=hull, mask=mask, f64=f64, f32=f32,
                            x=x, g64=g64, g32=g32)
    return _MODULE[key]


def module_gate(name, ours, f64, f32, factor=4.0, verbose=True):
    """rel-L2(ours, f64) <= factor rel-L2(torch binary32 of the same Sequential on the CPU, f64): the encoder's rule.  -> violations."""
    e, e32 = rel_l2(ours.cpu(), f64), rel_l2(f32, f64)
    if verbose:
        print(f"{name}: rel-L2 ours {e:.3e}, torch binary32 {e32:.3e}")
    return [] if e <= factor * e32 else [f"{name}: rel-L2 {e:.3e} > {factor} x {e32:.3e}"]


def fill_model(model, sd):
    model.load_state_dict(sd)
    return model


# ---- binary32 torch stand-ins of the three device operators (CPU runs of the host wiring) --------------------------------------------------
class TorchOps:
    IN_STACK, OUT_PLANAR, OUT_LERP, IN_NO_MASK = 1, 2, 4, 8
    FWD_MASK_INPUT, FWD_LERP = 1, 2
    ACT_NAMES = {0: "none", 1: "leaky", 2: "tanh"}
    calls = []

    @staticmethod
    def mask(img, hull, dog, want_response):
        TorchOps.calls.append("mask")
        p = {k: dog[k] for k in ("t", "sigma", "k", "epsilon", "kernel_factor")}
        resp = batch_dog(img.float(), **p)
        m = (resp > 0.5).float()
        if dog["d"] > 1:
            m = dilation(m, dog["d"])
        if hull is not None:
            m = m * (hull == 0)
        return m, (composite(img) if img.shape[1] == 4 else None), (resp if want_response else None)

    @staticmethod
    def conv(x, image, mask, hull, wk, bias, act, slope, pad, flags, plan, fault=None):
        T = TorchOps
        T.calls.append("conv")
        Ci, Co = wk.shape[1:]
        w = wk.reshape(3, 3, Ci, Co).permute(3, 2, 0, 1)
        if flags & T.IN_STACK:
            xin = image * (1 - mask) if mask is not None and not flags & T.IN_NO_MASK else image
            xin = torch.cat([xin, hull], dim=1) if hull is not None else xin
            xin = F.pad(xin, (pad,) * 4, mode="replicate") if pad else xin
        else:
            xin = x.permute(0, 3, 1, 2)
        if fault == "slope":
            slope = 0.2
        y = ACTS[T.ACT_NAMES[act]](F.conv2d(xin, w, bias), slope)
        if flags & T.OUT_LERP:
            y = torch.lerp(image, y, mask)
        return y.contiguous() if flags & T.OUT_PLANAR else y.permute(0, 2, 3, 1).contiguous()

    @staticmethod
    def forward(prog, img, hull, dog, mask, pad, flags):
        T = TorchOps
        image = img
        n = 0
        if dog is not None:
            mask, comp, _ = T.mask(img, hull, dog, False)
            image = comp if comp is not None else img
            n += 1
        x = None
        for i, (t, l) in enumerate(zip(prog.table, prog.layers)):
            first, last = i == 0, i == len(prog.layers) - 1
            lf = (T.IN_STACK if first else 0) | (T.IN_NO_MASK if first and not flags & T.FWD_MASK_INPUT else 0) | (T.OUT_PLANAR if last else 0) \
                | (T.OUT_LERP if last and flags & T.FWD_LERP else 0)
            x = T.conv(x, image if first or lf & T.OUT_LERP else None, mask if first or lf & T.OUT_LERP else None, hull if first and t.Ci == 4 else None,
                       l["wk"], l["bias"], t.act, t.slope, pad if first else 0, lf, t.plan)
            n += 1
        prog.launches = n
        return x, mask, image


def install_ops(monkeypatch, ops):
    """Replace the three device operators of panic3d_amd.ops by the binary32 stand-ins, and let the public forms take host tensors."""
    monkeypatch.setattr(ops, "_chk", lambda t, name, dtype=torch.float32: t.contiguous())
    monkeypatch.setattr(ops, "_rmline_mask_impl", TorchOps.mask)
    monkeypatch.setattr(ops, "_rmline_conv_impl", TorchOps.conv)
    monkeypatch.setattr(ops, "_rmline_forward_impl", TorchOps.forward)
    TorchOps.calls.clear()
