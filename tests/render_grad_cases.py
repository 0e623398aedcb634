"""The designed edge matrix of the renderer / point-decode backward (tests/test_hip_render_grad_edges.py on the HIP kernels,
tests/test_render_grad_ref_cpu.py for the gate itself): the smallest shapes that reach each tail, launch edge, option and tap
geometry of csrc/p3d_render_grad.hip, as tuples with the reason for each.

Every case is built from seeds on the CPU (build_render / build_decode).  Rays are supplied with their merged depths (the backward
takes depths_sorted as an input and needs only Sc >= 2): origins on a sheet in front of the box, directions near +z with a small
tilt, depths sorted uniform draws.  Coordinates below are in box units q = p * 2 / box_warp (the planes cover |q| < 1, their
half-texel border reaches 1 + 1/W).  Inputs are tame on purpose (smooth planes, sigma row gain <= 1, unit cotangents) so that a
float32 evaluation of the reference stays within a quarter of the gate (test_render_grad_ref_cpu.py checks that for every case)."""
import zlib

import numpy as np
import torch

import p3d_testing as T
import render_grad_ref as R

# options: ext (x / y half-width of the ray sheet), zext (half-length of the rays along z), tilt, box_warp, plane_mode (use_triplane),
# white_back, fsig (force_sigmoid), crop / cull / binarize, per_view (P3D_FLAG_PER_VIEW_CLAMP), shared (one plane set for N views),
# depths ("rand", "repeat": runs of equal depths and a few rays whose depths are all equal, "centres": every sample on a texel
# centre of the (x, y) and (x, z) planes), gain (sigma row gain), smooth (plane noise grid)
_D = dict(ext=0.45, zext=0.7, tilt=0.1, box_warp=2.0, plane_mode=1, white_back=False, fsig=True, crop=None, cull=None, binarize=None,
          per_view=False, shared=False, depths="rand", gain=0.25, smooth=3, scale=1.0, centre=(0.0, 0.0))

# (name, N, R, Sc, Sf, H, W, options, cotangents)   cotangents: all | feat | depth | wsum | xyz | none | zeros (all four, with
# whole rays and single channels exactly zero)
RENDER_CASES = [
    ("r1", 1, 1, 8, 8, 5, 9, dict(ext=0.8), "all"),                       # one ray: one lane of k_g_ray / 16 of k_g_mlp's first chunk
    ("r63", 1, 63, 8, 8, 16, 8, dict(), "all"),                           # 1008 samples: a last chunk of 48 lanes (total % 64 != 0)
    ("r64", 1, 64, 8, 8, 32, 32, dict(ext=0.7), "all"),                   # exactly one wave of rays, whole chunks only
    ("r65", 1, 65, 8, 8, 16, 8, dict(plane_mode=0), "all"),               # one ray into the second wave; plane 2 = (z, x)
    ("r257", 1, 257, 8, 8, 32, 32, dict(ext=0.45, white_back=True), "all"),  # one ray past a 256-thread block of k_g_ray / k_g_range
    ("views_own", 3, 37, 8, 8, 16, 8, dict(per_view=True), "all"),        # a wave spans three views; depth ranges 3 apart; own planes
    ("views_shared", 3, 37, 8, 8, 16, 8, dict(per_view=True, shared=True, white_back=True), "all"),  # ... one plane set for all views
    ("chunks1050", 1, 700, 48, 48, 32, 32, dict(ext=0.4, zext=0.7, tilt=0.05), "all"),  # 1050 chunks > G_MAX_BLOCKS: 26 workgroups take two
    ("s2", 1, 65, 2, 0, 32, 32, dict(ext=0.8), "all"),                    # one interval per ray
    ("s_odd", 1, 33, 5, 4, 5, 9, dict(ext=0.5, fsig=False), "all"),       # S = 9; the MipNeRF-clamped sigmoid (1.002)
    ("sf0", 1, 40, 12, 0, 16, 8, dict(white_back=True, fsig=False), "all"),  # single pass
    ("repeat", 1, 48, 8, 8, 16, 8, dict(depths="repeat"), "all"),         # dl == 0 intervals; rays of zero weight with unmasked samples
    ("tiny_1x3", 1, 20, 4, 4, 1, 3, dict(ext=0.3, centre=(-0.7, -0.7), tilt=0.0), "all"),  # one row of three texels: every sample in a border
    ("mix_5x9", 1, 3, 8, 8, 5, 9, dict(ext=1.5, zext=1.5, tilt=0.3), "all"),   # outside / border / interior taps, H != W
    ("mix_16x8", 2, 12, 8, 8, 16, 8, dict(ext=1.5, zext=1.5, tilt=0.3, plane_mode=0), "all"),  # the same with H > W, two images
    ("centres", 1, 32, 4, 4, 16, 8, dict(depths="centres"), "all"),       # bilinear weights exactly zero
    ("crop", 1, 80, 8, 8, 16, 8, dict(ext=0.8, crop=0.4), "all"),         # masked samples: no density gradient, colours keep theirs
    ("cull", 1, 80, 8, 8, 16, 8, dict(cull=0.5, gain=2.0, scale=3.0), "all"),
    ("binarize", 1, 80, 8, 8, 16, 8, dict(binarize=0.5, gain=2.0, scale=3.0, white_back=True), "all"),  # every density a constant
    ("crop_cull", 1, 70, 8, 8, 16, 8, dict(ext=0.9, tilt=0.02, crop=0.4, cull=0.5, gain=2.0, scale=3.0), "all"),  # with fully masked rays
    ("only_feat", 1, 65, 8, 8, 16, 8, dict(white_back=True), "feat"),     # anyc alone (with the white_back constant)
    ("only_depth", 1, 65, 8, 8, 16, 8, dict(), "depth"),                  # kappa alone
    ("only_wsum", 1, 65, 8, 8, 16, 8, dict(), "wsum"),                    # gconst alone
    ("only_xyz", 1, 65, 8, 8, 16, 8, dict(white_back=True), "xyz"),       # positions reach the planes through the weights only
    ("none", 1, 65, 8, 8, 16, 8, dict(), "none"),                         # nothing to do: exact zeros
    ("zeros", 1, 130, 8, 8, 16, 8, dict(ext=0.5), "zeros"),               # dead rays, a chunk of dead lanes, zero channels
]

# options: ext (half-width of the cube the points are drawn from), points ("rand" | "centres"), plane_mode, fsig, masks, shared
_DD = dict(ext=0.8, points="rand", box_warp=2.0, plane_mode=1, fsig=True, crop=None, cull=None, binarize=None, shared=False,
           gain=1.0, smooth=3, scale=1.0)
# (name, N, M, H, W, options, cotangents)   cotangents: both | sigma | rgb | none
DECODE_CASES = [
    ("m1", 1, 1, 1, 3, dict(ext=0.5), "both"),                            # one lane
    ("m63", 1, 63, 32, 32, dict(), "both"),                                 # one lane short of a chunk
    ("m65", 1, 65, 16, 8, dict(), "both"),                                # a last chunk of one lane
    ("n2_m100", 2, 100, 16, 8, dict(), "both"),                           # the image boundary inside the second wave
    ("n3_shared", 3, 50, 16, 8, dict(shared=True), "both"),               # one plane set for three point batches
    ("crop", 1, 90, 32, 32, dict(crop=0.4), "both"),                       # masked: zero density gradient, colour gradient kept
    ("cull", 1, 90, 32, 32, dict(cull=0.5, gain=2.0, scale=3.0), "both"),
    ("binarize", 1, 90, 32, 32, dict(binarize=0.5, gain=2.0, scale=3.0), "both"),
    ("crop_cull", 2, 70, 32, 32, dict(crop=0.3, cull=0.5, gain=2.0, scale=3.0), "both"),
    ("only_sigma", 1, 90, 32, 32, dict(cull=0.5, gain=2.0, scale=3.0), "sigma"),                # masked points are dead lanes
    ("only_rgb", 1, 90, 32, 32, dict(cull=0.5, gain=2.0, scale=3.0), "rgb"),
    ("none", 1, 90, 32, 32, dict(), "none"),
    ("mix_5x9", 1, 14, 5, 9, dict(ext=1.5), "both"),                     # outside, border and interior points
    ("centres", 1, 64, 16, 8, dict(points="centres"), "both"),            # bilinear weights exactly zero
    ("mode0", 1, 70, 16, 8, dict(plane_mode=0), "both"),                  # plane 2 = (z, x)
    ("clamped_rgb", 1, 70, 32, 32, dict(fsig=False), "both"),               # the 1.002 factor
]

MIX_CASES = ("mix_5x9", "mix_16x8")          # each tap class holds 10 % .. 90 % of the (sample, plane) pairs
MASK_CASES = ("crop", "cull", "binarize", "crop_cull")  # 10 % .. 90 % of the samples at the -1000 sentinel
VIEW_GAP = 3.0                               # distance between the depth ranges of consecutive views


def _seed(kind, name):
    return zlib.crc32(f"{kind}:{name}".encode()) % (1 << 30)


def _scene(seed, Np, H, W, o):
    planes = torch.from_numpy(T.make_planes(seed, Np, H, W, scale=o["scale"], smooth=o["smooth"]))
    mlp = [torch.from_numpy(np.ascontiguousarray(x)) for x in T.make_decoder_params(seed + 1, 1.0, o["gain"])]
    mlp[0] = mlp[0] / np.float32(np.sqrt(32))  # the pre-scaled tensors the C ABI takes (FullyConnectedLayer's 1 / sqrt(fan_in))
    mlp[2] = mlp[2] / np.float32(np.sqrt(64))
    if o["cull"] or o["binarize"]:  # densities on both sides of the threshold (alpha = 0.5 at sigma = 1): median sigma -> 1
        probe = (torch.rand(1, 512, 3, generator=torch.Generator().manual_seed(seed + 4)) * 2 - 1) * 0.7 * o["box_warp"] / 2
        sig, _ = R._decode(planes[:1], mlp, probe, o["box_warp"], o["plane_mode"], True, {})
        mlp[3][0] += 1.0 - float(sig.median())
    return planes, mlp


def _ro(o, Sc=2, Sf=0):
    return dict(T.RENDERING_KWARGS, box_warp=o["box_warp"], use_triplane=o["plane_mode"], white_back=o["white_back"] if "white_back" in o else False,
                depth_resolution=Sc, depth_resolution_importance=Sf, ray_start=0.5, ray_end=1.5)


def build_render(case):
    """name, N, R, Sc, Sf, H, W, options, cotangents -> dict of CPU float32 tensors and the options."""
    name, N, R, Sc, Sf, H, W, opt, cots = case
    o = dict(_D, **opt)
    seed, S, half = _seed("render", name), Sc + Sf, o["box_warp"] / 2
    g = torch.Generator().manual_seed(seed + 2)
    planes, mlp = _scene(seed, 1 if o["shared"] else N, H, W, o)
    if o["depths"] == "centres":  # x on W-grid centres, y and z on H-grid centres (exact in binary32: box_warp 2, powers of two)
        assert N == 1 and o["box_warp"] == 2.0 and S * 2 == H and R == (W // 2) * (H // 2)
        xc = (2 * (2 * torch.arange(W // 2) + 0.5) / W - 1).float()
        yc = (2 * (2 * torch.arange(H // 2) + 1.5) / H - 1).float()
        zc = (2 * (2 * torch.arange(S) + 0.5) / H - 1).float()
        xy = torch.stack(torch.meshgrid(xc, yc, indexing="ij"), -1).reshape(1, R, 2)
        rays_o = torch.cat([xy, torch.full((1, R, 1), -1.5)], -1)
        rays_d = torch.tensor([0.0, 0.0, 1.0]).expand(1, R, 3).contiguous()
        depths = (zc + 1.5).expand(1, R, S).contiguous()
    else:
        xy = ((torch.rand(N, R, 2, generator=g) * 2 - 1) * o["ext"] + torch.tensor(o["centre"])) * half
        back = torch.arange(N).view(N, 1, 1) * VIEW_GAP  # view v stands VIEW_GAP further back: depth ranges well apart
        rays_o = torch.cat([xy, -(o["zext"] * half + 0.5) - back.expand(N, R, 1)], -1).contiguous()
        rays_d = torch.cat([(torch.rand(N, R, 2, generator=g) * 2 - 1) * o["tilt"], torch.ones(N, R, 1)], -1).contiguous()
        depths = (0.5 + back + torch.rand(N, R, S, generator=g) * (2 * o["zext"] * half)).sort(-1).values.contiguous()
        if o["depths"] == "repeat":
            depths[:, :, 3] = depths[:, :, 2]
            depths[:, :, 7] = depths[:, :, 6] = depths[:, :, 5]
            depths[:, ::7] = depths[:, ::7, S // 2:S // 2 + 1]  # every seventh ray: all depths equal, total weight exactly zero
    gc = torch.Generator().manual_seed(seed + 3)
    cot = [torch.randn(N, R, k, generator=gc) for k in (32, 1, 1, 3)]
    if cots == "zeros":
        for c in cot:
            c[:, 64:128] = 0          # a whole chunk of rays at every sample index: k_g_mlp steps with no live lane
            c[:, 5::9] = 0            # scattered dead rays
        cot[0][:, :, 3::4] = 0        # zero channels: the gk != 0 / dc != 0 skips
        cot[0][:, 1::3] = 0           # rays that keep only their density path (anyc false)
        cot[3][:, :, 1] = 0
    elif cots != "all":
        cot = [c if cots == k else None for c, k in zip(cot, ("feat", "depth", "wsum", "xyz"))]
    return dict(name=name, N=N, R=R, Sc=Sc, Sf=Sf, S=S, H=H, W=W, o=o, ro=_ro(o, Sc, Sf), planes=planes, mlp=mlp, rays_o=rays_o,
                rays_d=rays_d, depths=depths, cot=cot, kw=dict(triplane_crop=o["crop"], cull_clouds=o["cull"],
                                                                binarize_clouds=o["binarize"], force_sigmoid=o["fsig"]))


def build_decode(case):
    """name, N, M, H, W, options, cotangents -> dict of CPU float32 tensors and the options."""
    name, N, M, H, W, opt, cots = case
    o = dict(_DD, **opt)
    seed, half = _seed("decode", name), o["box_warp"] / 2
    g = torch.Generator().manual_seed(seed + 2)
    planes, mlp = _scene(seed, 1 if o["shared"] else N, H, W, o)
    if o["points"] == "centres":  # x on W-grid centres, y and z on H-grid centres
        assert o["box_warp"] == 2.0
        c = lambda n: (2 * (torch.randint(0, n, (N, M), generator=g) + 0.5) / n - 1).float()
        coords = torch.stack([c(W), c(H), c(H)], -1)
        coords[:, ::5] = (torch.rand(N, (M + 4) // 5, 3, generator=g) * 2 - 1) * 0.9  # and some generic ones among them
    else:
        coords = (torch.rand(N, M, 3, generator=g) * 2 - 1) * o["ext"] * half
    gc = torch.Generator().manual_seed(seed + 3)
    g_sigma, g_rgb = torch.randn(N, M, 1, generator=gc), torch.randn(N, M, 32, generator=gc)
    if cots in ("rgb", "none"):
        g_sigma = None
    if cots in ("sigma", "none"):
        g_rgb = None
    return dict(name=name, N=N, M=M, H=H, W=W, o=o, ro=_ro(o), planes=planes, mlp=mlp, coords=coords.contiguous(), g_sigma=g_sigma,
                g_rgb=g_rgb, kw=dict(triplane_crop=o["crop"], cull_clouds=o["cull"], binarize_clouds=o["binarize"],
                                     force_sigmoid=o["fsig"]))


def masks_from_sigma(sigma):
    """bool: the entries a mask overwrote (the forward writes the sentinels -1000 / +1000, renderer.py:143,190-198)."""
    s = np.asarray(sigma)
    return (s == -1000.0) | (s == 1000.0)


def oracle_sigma(oracle, c, pts):
    """The exact contract's densities with the case's masks applied (oracle/p3d_oracle.c: the library forward's bits) at binary32
    points [N,M,3] — the CPU stand-in for ops.triplane_decode."""
    o = c["o"]
    opts = oracle.make_opts(c["ro"], o["crop"], o["cull"], o["binarize"], o["fsig"])
    planes = c["planes"].expand(pts.shape[0], -1, -1, -1, -1).numpy()
    sigma, _ = oracle.decode(planes, np.asarray(pts, np.float32), [t.numpy() for t in c["mlp"]], o["box_warp"], o["plane_mode"],
                             opts.flags, opts.crop_limit, opts.cull_thresh, density_only=True)
    return sigma[..., 0]


def render_sigma_points(c):
    """The binary32 sample points of a render case, as one point batch per view: [N, R*S, 3]."""
    return R.points32(c["rays_o"], c["rays_d"], c["depths"]).reshape(c["N"], -1, 3)


def render_ref(c, sigma, dtype=torch.float64, mut=None):
    """(planes gradient [Np,3,32,H,W], decoder gradients, touched map) of a render case; sigma [N,R*S]: the forward's densities
    at render_sigma_points (only the sentinels are read)."""
    return R.restate64(c["planes"], c["mlp"], c["rays_o"], c["rays_d"], c["depths"], torch.as_tensor(np.asarray(sigma)), None, c["ro"],
                       c["cot"], c["o"]["per_view"], c["o"]["fsig"], dtype=dtype, mut=mut, touched=True)


def decode_ref(c, sigma, dtype=torch.float64, mut=None):
    return R.decode_restate64(c["planes"], c["mlp"], c["coords"], c["g_sigma"], c["g_rgb"], masks_from_sigma(sigma), c["ro"],
                              c["o"]["fsig"], dtype=dtype, mut=mut)
