#!/usr/bin/env python3
"""Generate tests/golden/grad_*.npz: gradients of the REFERENCE's own ImportanceRenderer.forward and run_model (imported
unmodified from the reference tree, CPU, autograd) with respect to the triplanes and the raw OSGDecoder parameters.

Runs only in the build container (the GPU box has no reference tree); its outputs are committed and read by
tests/test_hip_render_grad.py.

    python tests/golden/make_golden_grad.py

Inputs come from tests/p3d_testing seeds (planes make_planes(smooth > 0), decoder make_decoder_params, draws
make_random_draws, which the reference's own rand_like / rand reproduce under torch.manual_seed); the four output cotangents are
seeded normal draws.  Stored: the plane gradient (NCHW), the gradients of net.0 / net.2 weight and bias, the forward outputs, the
rays, and meta_* fields to rebuild everything else.  Every case asserts that no cull / binarize decision lies within 1e-4 of its
threshold (a ulp-level decision flip between the reference and the exact contract cannot then appear).
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402  (sets up the reference import path; turns autograd off, switched back on below)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import p3d_testing as T  # noqa: E402
from training.volumetric_rendering.renderer import ImportanceRenderer  # noqa: E402

torch.set_grad_enabled(True)
MARGIN = 1e-4


def cotangents(seed, N, R):
    g = torch.Generator().manual_seed(int(seed))
    return [torch.randn(N, R, k, generator=g) for k in (32, 1, 1, 3)]


def check_margin(sigmas, thr):
    """False if a cull / binarize decision lies within MARGIN of its threshold."""
    if not thr:
        return True
    for s in sigmas:
        alpha = 1 - torch.exp(-torch.nn.functional.softplus(s.detach().double() - 1))
        gap = float((alpha - thr).abs().min())
        if gap <= MARGIN:
            return False
    return True


def decoder_grads(dec):
    return dict(g_w0=dec.net[0].weight.grad.numpy(), g_b0=dec.net[0].bias.grad.numpy(), g_w1=dec.net[2].weight.grad.numpy(),
                g_b1=dec.net[2].bias.grad.numpy())


def render_case(name, *, seed, tries=20, **kw):
    """The case at the first seed in seed, seed + 1000, ... whose reference gradient is finite and whose cull decisions all
    keep the margin."""
    for k in range(tries):
        if render_try(name, seed=seed + 1000 * k, **kw):
            return
    raise AssertionError(f"{name}: no usable seed")


def render_try(name, *, res, Sc, Sf, seed, ortho=False, crop=None, cull=None, binarize=None, use_triplane=1, white_back=True,
                force_sigmoid=True, sigma_gain=1.0, plane_scale=1.0, smooth=4, H=32, W=32, N=2,
                views=((0.0, 20.0, 30.0), (10.0, -60.0, 20.0)), allow_nan=False):
    ro = dict(T.RENDERING_KWARGS, depth_resolution=Sc, depth_resolution_importance=Sf, use_triplane=use_triplane, white_back=white_back)
    planes_np = T.make_planes(seed, N, H, W, scale=plane_scale, smooth=smooth)
    with torch.no_grad():
        dec = G.ref_decoder(seed + 1, 1.0, force_sigmoid, sigma_gain)
    os_, ds_ = [], []
    for elev, azim, fov in views[:N]:
        o, d = G.ortho_rays(elev, azim, res) if ortho else G.persp_rays(elev, azim, fov, res)[:2]
        os_.append(o)
        ds_.append(d)
    rays_o, rays_d = torch.cat(os_).contiguous(), torch.cat(ds_).contiguous()
    R = rays_o.shape[1]
    rend = ImportanceRenderer(use_triplane=bool(use_triplane))
    seen = []
    orig = rend.run_model

    def run_model(*a, **k):  # the raw densities, before the masks overwrite them in place
        out = orig(*a, **k)
        seen.append(out["sigma"].detach().clone())
        return out
    rend.run_model = run_model
    planes = torch.from_numpy(planes_np).requires_grad_(True)
    torch.manual_seed(seed + 2)
    feat, depth, wsum, xyz = rend(planes, dec, rays_o, rays_d, ro, triplane_crop=crop, cull_clouds=cull, binarize_clouds=binarize)
    if not check_margin(seen, binarize or cull):
        return None
    jit, u = T.make_random_draws(seed + 2, N, R, Sc, Sf)  # the reference's own draws, reproduced from the seed
    gf, gd, gw, gx = cotangents(seed + 3, N, R)
    loss = (feat * gf).sum() + (depth * gd).sum() + (wsum * gw).sum() + (xyz * gx).sum()
    loss.backward()
    gp = planes.grad.numpy()
    if not allow_nan and not (np.isfinite(gp).all() and all(np.isfinite(v).all() for v in decoder_grads(dec).values())):
        # the reference's gradient is NaN where a ray with zero total weight keeps an unmasked sample (0 / 0 in the depth's
        # division backward reaches that sample's density).  allow_nan: keep such a scene; the test then compares the finite
        # entries and requires ours to be finite everywhere
        return None
    empty = int((wsum.detach() == 0).sum())
    if 2 * empty > N * R:  # mostly empty space: too little to pin
        return None
    clamped = int(((depth.detach() == depth.min()) | (depth.detach() == depth.max())).sum())
    print(f"{name}: {N}x{R} rays, empty rays {empty}, rays at a clamp bound {clamped}, non-finite plane-gradient entries "
          f"{int((~np.isfinite(gp)).sum())} / {gp.size}")
    arrs = dict(grad_planes=gp, **decoder_grads(dec), feat=feat.detach().numpy(), depth=depth.detach().numpy(),
                wsum=wsum.detach().numpy(), xyz=xyz.detach().numpy(), rays_o=rays_o.numpy(), rays_d=rays_d.numpy(),
                planes_checksum=np.array(T.checksum(planes_np)), jitter_checksum=np.array(T.checksum(jit, u)))
    meta = dict(kind="render", Sc=Sc, Sf=Sf, N=N, H=H, W=W, seed=seed, crop=crop or 0.0, cull=cull or 0.0, binarize=binarize or 0.0,
                use_triplane=use_triplane, white_back=int(white_back), force_sigmoid=int(force_sigmoid), sigma_gain=sigma_gain,
                plane_scale=plane_scale, smooth=smooth, empty_rays=empty, clamped_rays=clamped)
    for k, v in meta.items():
        arrs["meta_" + k] = np.array(v)
    G.save(name + ".npz", **arrs)
    return True


def run_model_case(name, *, seed, M=512, N=2, H=32, W=32, use_triplane=1, force_sigmoid=False, smooth=4):
    ro = dict(T.RENDERING_KWARGS, use_triplane=use_triplane)
    planes_np = T.make_planes(seed, N, H, W, smooth=smooth)
    with torch.no_grad():
        dec = G.ref_decoder(seed + 1, 1.0, force_sigmoid, 1.0)
    coords = torch.from_numpy(T.make_points(seed + 2, N, M))
    rend = ImportanceRenderer(use_triplane=bool(use_triplane))
    planes = torch.from_numpy(planes_np).requires_grad_(True)
    out = rend.run_model(planes, dec, coords, torch.zeros_like(coords), ro)
    g = torch.Generator().manual_seed(seed + 3)
    gs, gr = torch.randn(N, M, 1, generator=g), torch.randn(N, M, 32, generator=g)
    ((out["sigma"] * gs).sum() + (out["rgb"] * gr).sum()).backward()
    arrs = dict(grad_planes=planes.grad.numpy(), **decoder_grads(dec), sigma=out["sigma"].detach().numpy(),
                rgb=out["rgb"].detach().numpy(), planes_checksum=np.array(T.checksum(planes_np)))
    meta = dict(kind="run_model", M=M, N=N, H=H, W=W, seed=seed, use_triplane=use_triplane, force_sigmoid=int(force_sigmoid),
                smooth=smooth, plane_scale=1.0)
    for k, v in meta.items():
        arrs["meta_" + k] = np.array(v)
    G.save(name + ".npz", **arrs)


GRAD_CASES = ["grad_persp_crop_cull", "grad_ortho_binarize", "grad_sf0", "grad_plane_mode0", "grad_run_model"]

if __name__ == "__main__":
    # perspective, crop 0.1 + cull 0.5, force_sigmoid; solid density (sigma_gain) so that weights saturate, border rays fully cropped
    render_case("grad_persp_crop_cull", res=16, Sc=16, Sf=16, seed=101, crop=0.1, cull=0.5, sigma_gain=30.0, plane_scale=4.0,
                views=((0.0, 20.0, 45.0), (10.0, -60.0, 40.0)), allow_nan=True)
    # orthographic, white_back, MipNeRF-clamped sigmoid, binarize_clouds (every density overwritten: colour gradients only)
    render_case("grad_ortho_binarize", res=16, Sc=12, Sf=12, seed=202, ortho=True, binarize=0.5, force_sigmoid=False,
                N=1, views=((20.0, 90.0, 0.0),))
    # single pass (depth_resolution_importance = 0), no white_back
    render_case("grad_sf0", res=16, Sc=24, Sf=0, seed=303, crop=0.1, white_back=False, sigma_gain=4.0, N=1)
    # the other plane orientation (use_triplane = 0: plane 2 = (z, x))
    render_case("grad_plane_mode0", res=12, Sc=16, Sf=16, seed=404, use_triplane=0, cull=0.5, sigma_gain=30.0, plane_scale=4.0,
                force_sigmoid=False, N=1, allow_nan=True)
    run_model_case("grad_run_model", seed=505, N=1)
