"""The super-resolution case shared by the golden-gradient script (tests/golden/make_golden_superres_grad.py, the reference's own
SuperresolutionHybrid8XDC) and the tests that compare with it (tests/test_superres_grad_cpu.py, tests/test_hip_superres_grad.py):
constructor arguments, deterministic parameters and the seeded inputs / cotangent.  Nothing here imports the reference."""
import numpy as np
import torch

# the released module (256 hidden channels) with sr_num_fp16_res > 0, so the reference's blocks clamp at 256 (superresolution.py:277-280;
# on CPU they still compute in fp32, networks_stylegan2.py:444-446)
SR_KW = dict(channels=32, img_resolution=512, sr_num_fp16_res=4, sr_antialias=True, channels_hidden=256, channel_base=32768,
             channel_max=512, fused_modconv_default="inference_only")
THIN = 13  # every THIN-th element of tensors above 4096 elements (each fixture stays below 1 MiB)


def fill(sr, seed=41):
    """Every parameter and `noise_const` buffer of a SuperresolutionHybrid8XDC (ours or the reference's: the same names), in sorted-name
    order from one seeded CPU generator.  ToRGB biases +-255 put a third of the image on each side of the clamp's edge, so the clamp
    clips on both sides and the mask matters."""
    g = torch.Generator().manual_seed(int(seed))
    with torch.no_grad():
        named = dict(sr.named_parameters())
        named.update({n: b for n, b in sr.named_buffers() if n.endswith("noise_const")})
        for name in sorted(named):
            p = named[name]
            if name.endswith("noise_strength"):
                p.fill_(0.1)
            elif name.endswith("affine.bias"):
                p.fill_(1.0)
            elif name.endswith("torgb.bias"):
                p.copy_(torch.tensor([255.0, -255.0, 0.0]))
            elif name.endswith(".bias"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.2)
            else:
                p.copy_(torch.randn(p.shape, generator=g))
    return sr


def draws(seed=42):
    """(rgb [1,3,128,128], feature image [1,32,128,128], ws [1,3,512], cotangent of the image [1,3,512,512], checksum)."""
    g = torch.Generator().manual_seed(int(seed))
    rgb = torch.randn(1, 3, 128, 128, generator=g)
    x = torch.randn(1, 32, 128, 128, generator=g)
    ws = torch.randn(1, 3, 512, generator=g)
    g_out = torch.randn(1, 3, 512, 512, generator=g)
    chk = float(sum(t.double().sum() for t in (rgb, x, ws, g_out)))
    return rgb, x, ws, g_out, chk


def thin(a):
    a = np.asarray(a)
    return a.reshape(-1)[::THIN] if a.size > 4096 else a


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


# The gate against the reference's fp32 autograd.  Both sides are fp32 forwards that sum in different orders; over the ~50 M activations
# of the two blocks a handful per million lie within rounding of an lrelu kink, and one flipped slope moves that element's gradient by
# 80 % ("the full-size check").  Measured with the torch stand-ins on CPU (the reference's own arithmetic, another
# order): <= 6.5e-4 per tensor, 4.7e-3 for a noise strength (one sum of terms of both signs); the HIP path on the MI355X: <= 1.7e-3,
# 1.8e-3.  The tight check of the same module is tests/test_hip_superres_grad.py's float64 comparison with shared branch decisions
# (<= 1e-4; measured <= 2e-6).
TOL, TOL_NOISE = 5e-3, 2e-2


def check_against_fixture(sr, rgb, x, ws, g, tol=TOL, tol_noise=TOL_NOISE):
    """The gradients of rgb, the feature image, ws and every parameter within relative L2 `tol` of the fixture's (noise strengths:
    `tol_noise`)."""
    bad = []

    def cmp(name, ours, ref):
        if ours is None:
            bad.append((name, "missing"))
            return
        o = ours.detach().cpu().numpy()
        e = rel_l2(thin(o) if ref.ndim == 1 and o.size > 4096 else o, ref)
        print(f"{name}: rel-L2 {e:.2e}")
        if not e <= (tol_noise if name.endswith("noise_strength") else tol):
            bad.append((name, e))
    cmp("rgb", rgb.grad, g["g_rgb"])
    cmp("x", x.grad, g["g_x"])
    cmp("ws", ws.grad, g["g_ws"])
    n = 0
    for name, p in sr.named_parameters():
        key = "g_" + name.replace(".", "__")
        assert key in g, key
        cmp(name, p.grad, g[key])
        n += 1
    assert n == sum(1 for k in g if k.startswith("g_") and k not in ("g_rgb", "g_x", "g_ws"))
    assert not bad, bad
