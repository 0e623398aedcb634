"""Density-grid query for marching cubes — the hot loop of `_util/eg3d_metrics3d.py:94-183 get_eg3d_volume`
(`_scripts/eval/generate.py:97`, BASELINE config c5), on the fused density-only decode kernel.

Differences from the reference, all deliberate: the backbone is run ONCE (the reference re-synthesises the planes for
every 100k-point chunk, eg3d_metrics3d.py:140 -> triplane.py:283), points are generated on the device, and nothing
crosses PCIe until the caller asks for it.  Quirks that are kept because they change the numbers:
  * create_samples uses float division, so the y / "x" coordinates carry a fractional part of the faster index
    (eg3d_metrics3d.py:80-82);
  * the cull mask is evaluated on the already-activated densities and writes -1e3 into them (eg3d_metrics3d.py:155-163).
"""
import numpy as np
import torch

from . import ops
from .renderer import decoder_params


def create_samples(N=256, voxel_origin=(0, 0, 0), cube_length=2.0, device=None, lo=0, hi=None, idx=None):
    """Points [1, (hi-lo), 3] of the reference's N^3 grid, flat indices [lo, hi) — or the explicit flat indices `idx` —
    (eg3d_metrics3d.py:70-92)."""
    origin = np.array(voxel_origin) - cube_length / 2
    voxel_size = cube_length / (N - 1)
    if idx is None:
        hi = N ** 3 if hi is None else hi
        idx = torch.arange(lo, hi, 1, dtype=torch.long, device=device)
    s = torch.zeros(idx.numel(), 3, device=idx.device)
    s[:, 2] = idx % N
    s[:, 1] = (idx.float() / N) % N
    s[:, 0] = ((idx.float() / N) / N) % N
    s[:, 0] = (s[:, 0] * voxel_size) + origin[2]
    s[:, 1] = (s[:, 1] * voxel_size) + origin[1]
    s[:, 2] = (s[:, 2] * voxel_size) + origin[0]
    return s.unsqueeze(0), origin, voxel_size


def sigma2density(sigma):  # eg3d_metrics3d.py:65-69
    return 1 - torch.exp(-torch.nn.functional.softplus(sigma - 1))


def density_grid(G, ws, cond, resolution=256, max_batch=None, triplane_crop=None, cull_clouds=None, lo=0, hi=None,
                 planes=None, skip_cropped=False, fast=False, **synthesis_kwargs):
    """sigma / density for flat grid indices [lo, hi) of the resolution^3 grid, on the device: dict(sigmas, densities)
    of shape [1, hi-lo, 1].  `planes` (NCHW [1,3,32,H,W]) skips the backbone.  skip_cropped: the points triplane_crop masks
    (about half of the grid at the released crop of 0.1) are not decoded — identical densities, their `sigmas` read -1000."""
    rk = G.rendering_kwargs
    dev = ws.device
    if planes is None:
        planes = G._planes(ws, cond, **({"noise_mode": "const"} | synthesis_kwargs))
    hi = resolution ** 3 if hi is None else hi
    opts = G.renderer._opts(rk, G.decoder)
    mlp = decoder_params(G.decoder)
    nhwc = G.renderer._nhwc(planes)
    # the grid points are generated inside the decode kernel with create_samples' float arithmetic (no points tensor)
    origin = np.array([0, 0, 0]) - rk["box_warp"] / 2
    vs = rk["box_warp"] / (resolution - 1)
    lim = None if triplane_crop is None else rk["box_warp"] / 2 - triplane_crop
    res = ops.grid_density(nhwc, resolution, lo, hi, vs, (origin[2], origin[1], origin[0]), mlp, opts, crop_limit=lim,
                           skip_cropped=skip_cropped, fast=fast)
    sig, cropmask = res if lim is not None else (res, None)
    # activation + triplane_crop_mask (renderer.py:138-149, on the sample points, applied to the DENSITIES) + cull_clouds_mask
    # (applied to the densities, sic) in one pass over the grid
    dens = ops.sigma2density(sig, cropmask, cull_clouds)
    return {"sigmas": sig, "densities": dens}


def to_volume(t, resolution):
    """The reference's final layout: [1, C, N, N, N] with the first grid axis flipped (eg3d_metrics3d.py:166-177)."""
    return t.reshape(t.shape[0], resolution, resolution, resolution, t.shape[-1]).flip(dims=(1,)).permute(0, 4, 1, 2, 3)


def density_grid_sharded(G, ws, cond, resolution=256, dst=0, **kw):
    """c5 on N GPUs: each rank decodes a contiguous slab of the slowest grid axis; one gather of the sigma / density slabs."""
    import torch.distributed as dist
    from . import sharding
    world = dist.get_world_size() if dist.is_initialized() else 1
    rank = dist.get_rank() if dist.is_initialized() else 0
    a, b = sharding.partition(resolution, world, rank)
    if b > a:
        out = density_grid(G, ws, cond, resolution, lo=a * resolution ** 2, hi=b * resolution ** 2, **kw)
    else:  # more ranks than grid slices: an empty slab that still takes part in the gather
        out = {k: torch.empty((1, 0, 1), dtype=torch.float32, device=ws.device) for k in ("sigmas", "densities")}
    if world == 1:
        return out
    counts = [sharding.partition(resolution, world, r)[1] - sharding.partition(resolution, world, r)[0] for r in range(world)]
    res = {}
    for k, v in out.items():
        slabs = v.reshape(b - a, resolution * resolution)
        g = sharding.gather_frames(slabs, counts, dst)
        res[k] = g.reshape(1, -1, 1) if g is not None else None
    return res


def marching_cubes(vol, rgbs, boxwarp, level=0.5, flip0=False, allow_degenerate=False, as_tensors=False):
    """`_util/eg3d_metrics3d.py:186-210 marching_cubes(vol, rgbs, boxwarp, level)` with the surface extracted on the device.
    vol [n,n,n] (device tensor; numpy is uploaded), rgbs: [>=3,n,n,n] tensor indexed like the reference does
    (`rgbs[:3, a, b, c]` at `verts.astype(int)`), or a callable `rgbs(ijk[V,3] long) -> [V,3]`, or None.
    Returns the reference's dict (verts scaled by /n*bw - bw/2 as eg3d_metrics3d.py:201-202 — sic, n not n-1; numpy
    arrays).  The triangulation is this repo's, not Lewiner's: PARITY UNPINNED against skimage (absent here; the
    fixture generator tests/golden/make_golden_mesh.py and tests/test_mcubes_cpu.py::test_triangulation_against_skimage_lewiner are
    ready for a box that has it).  allow_degenerate=False is what the reference
    passes to skimage (eg3d_metrics3d.py:189-194): zero-area triangles (a grid value exactly on the level) are removed.
    as_tensors: the dict holds device tensors instead of numpy arrays (nothing is downloaded; metrics.geometry_metrics takes it)."""
    if not torch.is_tensor(vol):
        vol = torch.as_tensor(np.ascontiguousarray(vol, dtype=np.float32)).cuda()
    n = vol.shape[-1]
    verts, faces, normals, values = ops.marching_cubes(vol.contiguous(), level, flip0=flip0, allow_degenerate=allow_degenerate)
    out = {}
    host = (lambda t: t) if as_tensors else (lambda t: t.cpu().numpy())
    if rgbs is not None:
        ijk = verts.long()  # .astype(int): truncation; coordinates are >= 0
        if callable(rgbs):
            colors = rgbs(ijk)
        else:
            colors = rgbs[:3, ijk[:, 0], ijk[:, 1], ijk[:, 2]].t()
        out["colors"] = host(colors)
    out["verts"] = host(verts / n * boxwarp - 0.5 * boxwarp)
    out["faces"] = host(faces)
    out["normals"] = host(normals)
    out["values"] = host(values)
    return out


def mesh(G, ws, cond, resolution=256, level=0.5, triplane_crop=None, cull_clouds=None, planes=None, as_tensors=False, **synthesis_kwargs):
    """generate.py:97-103 (get_eg3d_volume + marching_cubes) without the volume leaving the GPU: density grid on the fused
    decode kernel, surface extraction on the device, and the 32-channel colour grid of the reference (17 GB at 512^3, of
    which three channels at the vertices' voxels are used) replaced by ONE decode of exactly those voxels."""
    rk = G.rendering_kwargs
    if planes is None:
        planes = G._planes(ws, cond, **({"noise_mode": "const"} | synthesis_kwargs))
    g = density_grid(G, ws, cond, resolution, triplane_crop=triplane_crop, cull_clouds=cull_clouds, planes=planes,
                     skip_cropped=True)  # only the densities are used below
    dens = g["densities"].reshape(resolution, resolution, resolution)
    mlp, opts = decoder_params(G.decoder), G.renderer._opts(rk, G.decoder)
    nhwc = G.renderer._nhwc(planes)

    def colors(ijk):  # volume index (a,b,c) -> flat index of the un-flipped grid -> create_samples point -> decoder rgb
        flat = ((resolution - 1 - ijk[:, 0]) * resolution + ijk[:, 1]) * resolution + ijk[:, 2]
        pts, _, _ = create_samples(resolution, (0, 0, 0), rk["box_warp"], idx=flat)
        if pts.shape[1] == 0:
            return torch.empty((0, 3), device=flat.device)
        _, rgb = ops.triplane_decode(nhwc, pts.contiguous(), mlp, opts)
        return rgb[0, :, :3]

    return marching_cubes(dens, colors, rk["box_warp"], level=level, flip0=True, as_tensors=as_tensors)
