"""Tensor-level operators over the C ABI (include/panic3d_hip.h).

PyTorch is plumbing here: it owns device memory and the current HIP stream; every computation is a call into
libpanic3d_hip.so.  All tensors must be float32 CUDA(ROCm) tensors; misuse raises like the reference's plugins do
(TORCH_CHECK -> RuntimeError, torch_utils/ops/bias_act.cpp:39-55).
"""
import ctypes as C
import math
import os
import weakref

import numpy as np
import torch

from . import _lib, memo
from ._lib import Opts, Dumps

__all__ = ["make_opts", "prescale_mlp", "planes_to_nhwc", "triplane_decode", "render", "sample_stratified", "composite",
           "importance", "unify_perm", "render_backward", "triplane_decode_backward"]


# torch.cuda.current_stream() builds a Stream object through three layers of Python (~7 us) and torch.cuda.current_device() goes
# through _lazy_init (~1 us); a G.f call asks ~45 times for each while the GPU waits for the launches of its 4^2 .. 32^2 layers
# (tools/host_profile.py: 0.3 ms of a 2.5 ms call).  The two C entry points below are what those wrappers end in.
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None) or (lambda index: torch.cuda.current_stream(index).cuda_stream)
_cur_device = getattr(torch._C, "_cuda_getDevice", None) or torch.cuda.current_device


def _stream():
    return C.c_void_p(_raw_stream(_cur_device()))


class _NoGuard:
    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


_NOGUARD = _NoGuard()


def _on(device):
    """The C ABI launches on the CURRENT device's stream, so a call has to run with its tensors' device current.
    `torch.cuda.device(...)` costs ~10 us of host time per entry (get + set + restore); when the device already is the current one
    — always, with one process per GPU — nothing has to be switched: a G.f call makes ~35 such calls and starts with an empty
    queue, so this is latency the GPU waits for (profiles/r04_notes.txt)."""
    idx = device.index
    if idx is None or idx == _cur_device():
        return _NOGUARD
    return torch.cuda.device(device)


def _chk(t, name, dtype=torch.float32):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA/ROCm tensor (the HIP path has no CPU fallback)")
    if t.dtype != dtype:
        raise RuntimeError(f"{name} must be {dtype}, got {t.dtype}")
    return t.contiguous()


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def make_opts(rendering_options, triplane_crop=None, cull_clouds=None, binarize_clouds=None, force_sigmoid=False,
              early_out=True, small_launch_kernel=True, fast_color=False):
    """rendering_kwargs + ImportanceRenderer.forward arguments (renderer.py:162) -> p3d_opts.
    The double -> binary32 conversions are the ones include/p3d_numerics.h states."""
    ro = rendering_options
    auto = ro.get("ray_start") == "auto" and ro.get("ray_end") == "auto"  # per-ray limits: render(..., ray_limits=...)
    if not auto and (ro.get("ray_start") == "auto" or ro.get("ray_end") == "auto"):
        raise ValueError("ray_start and ray_end must both be 'auto' or both be numbers (renderer.py:165)")
    disparity = bool(ro.get("disparity_space_sampling", False))  # renderer.py:309-316
    if disparity and auto:
        raise NotImplementedError("disparity_space_sampling together with ray_start = ray_end = 'auto'")
    if ro.get("clamp_mode", "softplus") != "softplus":
        raise AssertionError("MipRayMarcher only supports `clamp_mode`=`softplus`!")  # ray_marcher.py:35
    if (ro.get("density_noise", 0) or 0) > 0:  # (ImportanceRenderer.forward routes such calls to forward_staged)
        raise NotImplementedError("density_noise > 0 (renderer.py:276-277) is not an option of the fused kernel: ImportanceRenderer.forward_staged")
    if ro.get("triplane_depth", 1) != 1:
        raise NotImplementedError("triplane_depth != 1")
    bw = float(ro["box_warp"])
    Sc = int(ro["depth_resolution"])
    Sf = int(ro.get("depth_resolution_importance", 0) or 0)
    flags, crop_limit, thr = 0, 0.0, 0.0
    if triplane_crop:
        flags |= _lib.P3D_FLAG_CROP
        crop_limit = bw / 2 - float(triplane_crop)
    if binarize_clouds:
        flags |= _lib.P3D_FLAG_BINARIZE
        thr = float(binarize_clouds)
    elif cull_clouds:
        flags |= _lib.P3D_FLAG_CULL
        thr = float(cull_clouds)
    if force_sigmoid:
        flags |= _lib.P3D_FLAG_FORCE_SIGMOID
    if ro.get("white_back", False):
        flags |= _lib.P3D_FLAG_WHITE_BACK
    if not early_out:  # decode every sample even where the result provably cannot matter (measurement / tests)
        flags |= _lib.P3D_FLAG_NO_EARLY_OUT
    if not small_launch_kernel:  # keep small launches on the 32-rays-per-wave kernel (tests)
        flags |= _lib.P3D_FLAG_NO_PAIR
    elif small_launch_kernel == "pair":  # ... or force the 16 rays x 2 samples kernel / the 8 rays x 4 samples one (tests, A/B);
        flags |= _lib.P3D_FLAG_PAIR16    # True: the library's size heuristic picks (p3d_render_f32)
    elif small_launch_kernel == "quad":
        flags |= _lib.P3D_FLAG_QUAD8
    if fast_color:  # opt-in tolerance mode of the final pass (include/panic3d_hip.h P3D_FLAG_FAST_COLOR)
        flags |= _lib.P3D_FLAG_FAST_COLOR
    rs, re = (0.0, 0.0) if auto else (float(ro["ray_start"]), float(ro["ray_end"]))
    if disparity:  # the kernel receives the reciprocals the reference forms in binary64 and multiplies as binary32 scalars
        flags |= _lib.P3D_FLAG_DISPARITY
        return Opts(np.float32(2.0 / bw), np.float32(1.0 / rs), np.float32(1.0 / re), np.float32(1 / max(Sc - 1, 1)),
                    np.float32(crop_limit), np.float32(thr), Sc, Sf, int(bool(ro.get("use_triplane", False))), flags)
    return Opts(np.float32(2.0 / bw), np.float32(rs), np.float32(re), np.float32((re - rs) / max(Sc - 1, 1)),
                np.float32(crop_limit), np.float32(thr), Sc, Sf, int(bool(ro.get("use_triplane", False))), flags)


def _with_flag(opts, flag):
    o = Opts.from_buffer_copy(opts)
    o.flags |= flag
    return o


def prescale_mlp(w0, b0, w1, b1, weight_gain0, bias_gain0, weight_gain1, bias_gain1):
    """FullyConnectedLayer.forward's `w * weight_gain`, `b * bias_gain` (networks_stylegan2.py:121-127), in float32."""
    w0s = (w0.detach().float() * float(weight_gain0)).contiguous()
    w1s = (w1.detach().float() * float(weight_gain1)).contiguous()
    b0s = b0.detach().float()
    b1s = b1.detach().float()
    if bias_gain0 != 1:
        b0s = b0s * float(bias_gain0)
    if bias_gain1 != 1:
        b1s = b1s * float(bias_gain1)
    return w0s, b0s.contiguous(), w1s, b1s.contiguous()


def planes_to_nhwc(planes):
    """[N,3,32,H,W] (training/triplane.py:200-206) -> channels-last [N,3,H,W,32]."""
    planes = _chk(planes, "planes")
    if planes.dim() != 5 or planes.shape[1] != 3 or planes.shape[2] != 32:
        raise RuntimeError(f"planes must be [N,3,32,H,W], got {tuple(planes.shape)}")
    N, _, Cc, H, W = planes.shape
    out = torch.empty((N, 3, H, W, Cc), dtype=torch.float32, device=planes.device)
    with _on(planes.device):
        _lib.check(_lib.lib().p3d_planes_to_nhwc_f32(_p(planes), N * 3, Cc, H, W, _p(out), _stream()), "p3d_planes_to_nhwc_f32")
    return out


def _chk_mlp(mlp):
    w0, b0, w1, b1 = (_chk(t, n) for t, n in zip(mlp, ("w0", "b0", "w1", "b1")))
    if tuple(w0.shape) != (64, 32) or tuple(b0.shape) != (64,) or tuple(w1.shape) != (33, 64) or tuple(b1.shape) != (33,):
        raise RuntimeError("decoder must be OSGDecoder-shaped: 32 -> 64 -> 33 (training/triplane.py:521-526)")
    return w0, b0, w1, b1


def triplane_decode(planes_nhwc, coords, mlp, opts, density_only=False):
    """run_model (renderer.py:266-280) on coords [N,M,3] -> sigma [N,M,1], rgb [N,M,32] (None if density_only).
    Masks are applied iff opts.flags carries CROP/CULL/BINARIZE."""
    planes_nhwc = _chk(planes_nhwc, "planes_nhwc")
    coords = _chk(coords, "coords")
    N, three, H, W, Cc = planes_nhwc.shape
    if N == 1 and coords.dim() == 3 and coords.shape[0] > 1:  # one subject, several point batches: planes are shared
        N, opts = coords.shape[0], _with_flag(opts, _lib.P3D_FLAG_SHARED_PLANES)
    if three != 3 or Cc != 32 or coords.dim() != 3 or coords.shape[0] != N or coords.shape[2] != 3:
        raise RuntimeError("planes_nhwc must be [N,3,H,W,32] (or [1,...] shared) and coords [N,M,3]")
    w0, b0, w1, b1 = _chk_mlp(mlp)
    M = coords.shape[1]
    sigma = torch.empty((N, M, 1), dtype=torch.float32, device=coords.device)
    rgb = None if density_only else torch.empty((N, M, 32), dtype=torch.float32, device=coords.device)
    with _on(coords.device):
        rc = _lib.lib().p3d_triplane_decode_f32(_p(planes_nhwc), N, H, W, _p(coords), M, _p(w0), _p(b0), _p(w1), _p(b1),
                                                C.byref(opts), _p(sigma), _p(rgb), _stream())
    _lib.check(rc, "p3d_triplane_decode_f32")
    return sigma, rgb


def decode_features(feats, mlp, force_sigmoid=True):
    """OSGDecoder.forward (training/triplane.py:528-544) on sampled features [N,3,M,32] -> sigma [N,M,1], rgb [N,M,32]."""
    feats = _chk(feats, "sampled_features")
    if feats.dim() != 4 or feats.shape[1] != 3 or feats.shape[3] != 32:
        raise RuntimeError("sampled_features must be [N,3,M,32]")
    N, _, M, _ = feats.shape
    w0, b0, w1, b1 = _chk_mlp(mlp)
    sigma = torch.empty((N, M, 1), dtype=torch.float32, device=feats.device)
    rgb = torch.empty((N, M, 32), dtype=torch.float32, device=feats.device)
    with _on(feats.device):
        rc = _lib.lib().p3d_decode_features_f32(_p(feats), N, M, _p(w0), _p(b0), _p(w1), _p(b1), int(bool(force_sigmoid)), _p(sigma),
                                                _p(rgb), _stream())
    _lib.check(rc, "p3d_decode_features_f32")
    return sigma, rgb


def grid_density(planes_nhwc, grid_n, lo, hi, voxel_size, offsets, mlp, opts, crop_limit=None, skip_cropped=False, staged=None, fast=False):
    """Density-only decode of flat indices [lo, hi) of the reference's grid_n^3 sample grid (create_samples), the points
    generated inside the kernel.  planes_nhwc [1,3,H,W,32] -> sigma [1, hi-lo, 1]; with crop_limit also the bool mask
    [1, hi-lo, 1] of triplane_crop_mask (|x| or |z| beyond the limit) evaluated on the same generated points.
    skip_cropped: do not decode masked points (sigma = -1000 there): exact for the densities, which are overwritten anyway."""
    if skip_cropped and crop_limit is not None:
        opts = _with_flag(opts, _lib.P3D_FLAG_SKIP_CROPPED)
    if fast:  # tolerance-mode decoder (f16 two-term MFMA + hardware transcendentals): sigma to ~1e-6 of the exact contract
        opts = _with_flag(opts, _lib.P3D_FLAG_FAST_COLOR)
    if staged is not None:  # default: direct (quad-cooperative / per-lane) gathers; staged=True: texel boxes through LDS (same bits)
        opts = _with_flag(opts, (_lib.P3D_FLAG_FORCE_STAGING if staged else _lib.P3D_FLAG_NO_STAGING))
    planes_nhwc = _chk(planes_nhwc, "planes_nhwc")
    if planes_nhwc.shape[0] != 1:
        raise RuntimeError("grid_density renders one subject at a time")
    _, _, H, W, _ = planes_nhwc.shape
    w0, b0, w1, b1 = _chk_mlp(mlp)
    sigma = torch.empty((1, hi - lo, 1), dtype=torch.float32, device=planes_nhwc.device)
    msk = torch.empty((1, hi - lo, 1), dtype=torch.uint8, device=planes_nhwc.device) if crop_limit is not None else None
    with _on(planes_nhwc.device):
        rc = _lib.lib().p3d_grid_density_f32(_p(planes_nhwc), H, W, int(grid_n), int(lo), int(hi), np.float32(voxel_size),
                                              np.float32(offsets[0]), np.float32(offsets[1]), np.float32(offsets[2]), _p(w0),
                                              _p(b0), _p(w1), _p(b1), C.byref(opts), _p(sigma), _p(msk),
                                              np.float32(crop_limit if crop_limit is not None else 0.0), _stream())
    _lib.check(rc, "p3d_grid_density_f32")
    return (sigma, msk.view(torch.bool)) if crop_limit is not None else sigma  # the kernel writes 0 / 1 bytes: no conversion pass


def sigma2density(sigma, cropmask=None, cull=None):
    """get_eg3d_volume's activation and masks in one pass (eg3d_metrics3d.py:65-69,153-163): 1 - exp(-softplus(sigma - 1)),
    -1000 where cropmask, then -1000 where the cull mask — evaluated on the densities, as the reference does — fires."""
    sigma = _chk(sigma, "sigma")
    out = torch.empty_like(sigma)
    cm = None
    if cropmask is not None:
        cm = cropmask.contiguous()
        cm = cm.view(torch.uint8) if cm.dtype == torch.bool else cm.to(torch.uint8)  # bool is one 0 / 1 byte: reinterpret
        if cm.numel() != sigma.numel() or not cm.is_cuda:
            raise RuntimeError("cropmask must be a CUDA tensor with one entry per sigma")
    with _on(sigma.device):
        rc = _lib.lib().p3d_sigma2density_f32(_p(sigma), _p(cm), sigma.numel(), np.float32(-1.0 if cull is None else cull), _p(out),
                                              _stream())
    _lib.check(rc, "p3d_sigma2density_f32")
    return out


def drop_degenerate_faces(verts, faces, normals, values):
    """skimage's `allow_degenerate=False` (the reference: _util/eg3d_metrics3d.py:189-194): a grid value exactly on the level puts
    several edge crossings on the same grid point, i.e. zero-area triangles.  As skimage does: a face with two coincident
    vertices is dropped, the coincident vertices are merged (the higher index follows the lower), vertices no face uses any
    more are removed and the faces re-indexed.  Index compaction on the device; nothing is downloaded."""
    if faces.shape[0] == 0:
        return verts, faces, normals, values
    f = faces.long()
    tri = verts[f]  # [F,3,3]
    vmap = torch.arange(verts.shape[0], device=verts.device)
    deg = torch.zeros(f.shape[0], dtype=torch.bool, device=verts.device)
    for a, b in ((0, 1), (0, 2), (1, 2)):
        same = (tri[:, a] == tri[:, b]).all(dim=1)
        deg |= same
        hi, lo = torch.maximum(f[same, a], f[same, b]), torch.minimum(f[same, a], f[same, b])
        vmap.scatter_reduce_(0, hi, lo, reduce="amin")  # deterministic for repeated indices (a plain indexed store is not)
    for _ in range(4):  # follow chains a -> b -> c (coincident vertices of one grid point: at most a handful)
        vmap = vmap[vmap]
    f = vmap[f[~deg]]
    used = torch.zeros(verts.shape[0], dtype=torch.bool, device=verts.device)
    used[f.reshape(-1)] = True
    new_index = torch.cumsum(used, 0) - 1
    return verts[used], new_index[f].to(torch.int32), normals[used], values[used]


def marching_cubes(vol, level, flip0=False, allow_degenerate=True):
    """Iso-surface of vol [n,n,n] (device, f32) at `level`, on the device (csrc/p3d_mcubes.hip; specification: DESIGN.md §4.5,
    case table include/p3d_mc_table.h).  flip0: vol is the un-flipped flat grid of grid_density (axis 0 is read reversed).
    Returns verts [V,3] (index space, axis 0/1/2 order), faces [F,3] int32, normals [V,3], values [V] — device tensors.
    One 16-byte D2H read (the counts) sits between the two launches groups because the caller owns the output buffers.
    allow_degenerate=False: zero-area triangles are removed like skimage does (drop_degenerate_faces)."""
    vol = _chk(vol, "vol")
    n = vol.shape[0]
    if vol.dim() != 3 or vol.shape != (n, n, n):
        raise RuntimeError("vol must be [n,n,n]")
    L = _lib.lib()
    wsb = L.p3d_mc_workspace_bytes(n)
    if wsb == 0:
        raise RuntimeError("marching_cubes: n must be in [2, 1024]")
    dev = vol.device
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    with _on(dev):
        _lib.check(L.p3d_mc_count_f32(_p(vol), n, int(bool(flip0)), np.float32(level), _p(ws), wsb, _p(counts), _stream()),
                   "p3d_mc_count_f32")
        V, F = (int(x) for x in counts.tolist())
        verts = torch.empty((V, 3), dtype=torch.float32, device=dev)
        normals = torch.empty((V, 3), dtype=torch.float32, device=dev)
        values = torch.empty((V,), dtype=torch.float32, device=dev)
        faces = torch.empty((F, 3), dtype=torch.int32, device=dev)
        _lib.check(L.p3d_mc_emit_f32(_p(vol), n, int(bool(flip0)), np.float32(level), _p(ws), wsb, V, F, _p(verts), _p(normals),
                                     _p(values), _p(faces), _stream()), "p3d_mc_emit_f32")
    if not allow_degenerate:
        return drop_degenerate_faces(verts, faces, normals, values)
    return verts, faces, normals, values


DUMP_KEYS = ("depths_coarse", "sigma_coarse", "weights_coarse", "depths_fine", "inds", "depths_sorted", "sigma_sorted",
             "depth_unclamped", "tminmax")


def render(planes_nhwc, rays_o, rays_d, jitter, u, mlp, opts, ray_tile_w=0, dumps=False, stats=None, per_view_clamp=False,
           ray_limits=None, rng_seed=None, weights_only=False):
    """ImportanceRenderer.forward (renderer.py:162-264) with the two random draws passed in:
    jitter [N,R,Sc(,1)] (torch.rand_like, :324) and u [N*R,Sf] (torch.rand, :371).
    Returns (feat [N,R,32], depth [N,R,1], wsum [N,R,1], xyz [N,R,3]) (+ dict of per-stage dumps).
    `stats`: pass a dict to receive the number of decode steps the launch executed (exact early-outs, see k_render) and which
    gather set-up it ran (`interior_taps`, include/panic3d_hip.h p3d_render_taps_info).
    per_view_clamp: clamp each image's depth to its own sample range (N batched views = N calls of the reference).
    ray_limits: (ray_start, ray_end) per ray [N,R(,1)] for rendering_options['ray_start'] == ['ray_end'] == 'auto'
    (renderer.py:165-171; cameras.ray_limits_box + cameras.patch_ray_limits compute them).
    rng_seed (int, with jitter = u = None): the two draws are made inside the kernel by the counter-based generator of
    include/p3d_numerics.h (p3d_render_rng_f32) — no draw tensors exist.
    weights_only: the caller wants wsum and depth only (P3D_FLAG_WEIGHTS_ONLY: paste_front's occlusion pass) — returns
    (None, depth, wsum, None); where the library has a weights-only kernel the colours are never decoded, elsewhere the full
    kernel runs: wsum / depth are the full launch's bits either way."""
    if weights_only:
        if dumps:
            raise RuntimeError("render: weights_only and dumps exclude each other")
        opts = _with_flag(opts, _lib.P3D_FLAG_WEIGHTS_ONLY)
    if per_view_clamp:
        opts = _with_flag(opts, _lib.P3D_FLAG_PER_VIEW_CLAMP)
    planes_nhwc = _chk(planes_nhwc, "planes_nhwc")
    if rng_seed is not None and (jitter is not None or u is not None):
        raise RuntimeError("render: pass either the two draws (jitter, u) or rng_seed, not both")
    rays_o, rays_d = _chk(rays_o, "ray_origins"), _chk(rays_d, "ray_directions")
    if rng_seed is None:
        jitter = _chk(jitter, "jitter")
    N, three, H, W, Cc = planes_nhwc.shape
    if N == 1 and rays_o.dim() == 3 and rays_o.shape[0] > 1:  # many views of ONE subject in one launch: planes are shared
        N, opts = rays_o.shape[0], _with_flag(opts, _lib.P3D_FLAG_SHARED_PLANES)
    if three != 3 or Cc != 32 or rays_o.dim() != 3 or rays_o.shape[0] != N or rays_o.shape[2] != 3 or rays_d.shape != rays_o.shape:
        raise RuntimeError("planes_nhwc must be [N,3,H,W,32] (or [1,...] shared by all views); ray_origins / ray_directions [N,R,3]")
    R = rays_o.shape[1]
    Sc, Sf = opts.Sc, opts.Sf
    if rng_seed is None and jitter.numel() != N * R * Sc:
        raise RuntimeError(f"jitter must hold N*R*Sc = {N * R * Sc} values")
    if Sf > 0 and rng_seed is None:
        u = _chk(u, "u")
        if u.numel() != N * R * Sf:
            raise RuntimeError(f"u must hold N*R*Sf = {N * R * Sf} values")
    else:
        u = None
    w0, b0, w1, b1 = _chk_mlp(mlp)
    dev = rays_o.device
    feat = torch.empty((N, R, 32), dtype=torch.float32, device=dev)
    depth = torch.empty((N, R, 1), dtype=torch.float32, device=dev)
    wsum = torch.empty((N, R, 1), dtype=torch.float32, device=dev)
    xyz = torch.empty((N, R, 3), dtype=torch.float32, device=dev)
    L = _lib.lib()
    wsb = L.p3d_render_workspace_bytes(N, R, Sc, Sf)
    ws = torch.empty((wsb,), dtype=torch.uint8, device=dev)
    d, dm = None, None
    if dumps:
        NR, S = N * R, Sc + Sf
        f32 = dict(dtype=torch.float32, device=dev)
        shapes = dict(depths_coarse=(NR, Sc), sigma_coarse=(NR, Sc), weights_coarse=(NR, Sc - 1), depths_fine=(NR, Sf), inds=(NR, Sf),
                      depths_sorted=(NR, S), sigma_sorted=(NR, S), depth_unclamped=(NR,), tminmax=(2,))
        keys = DUMP_KEYS if dumps is True else tuple(dumps)  # a collection of names: only those stages are dumped
        if any(k not in shapes for k in keys):
            raise RuntimeError(f"render: unknown dump names {sorted(set(keys) - set(shapes))}")
        d = {k: torch.empty(shapes[k], dtype=torch.int32, device=dev) if k == "inds" else torch.empty(shapes[k], **f32) for k in keys}
        dm = Dumps(*[_p(d.get(k)) for k in DUMP_KEYS])
    rs_t = re_t = None
    if ray_limits is not None and (opts.flags & _lib.P3D_FLAG_DISPARITY):
        raise NotImplementedError("disparity_space_sampling with per-ray limits")
    if ray_limits is None and not (opts.flags & _lib.P3D_FLAG_DISPARITY) and not (opts.ray_end > opts.ray_start):
        raise RuntimeError("empty depth range: rendering_options with ray_start = ray_end = 'auto' need ray_limits (per-ray limits)")
    if ray_limits is not None:  # ray_start = ray_end = 'auto' (renderer.py:165-171): per-ray limits [N,R(,1)], already patched
        rs_t, re_t = _chk(ray_limits[0], "ray_limits[0]"), _chk(ray_limits[1], "ray_limits[1]")
        if rs_t.numel() != N * R or re_t.numel() != N * R:
            raise RuntimeError(f"ray_limits must hold N*R = {N * R} values each")
    with _on(dev):
        if rng_seed is not None:
            rc = L.p3d_render_rng_f32(_p(planes_nhwc), N, H, W, _p(rays_o), _p(rays_d), R, int(ray_tile_w), int(rng_seed) & (2 ** 64 - 1),
                                      _p(w0), _p(b0), _p(w1), _p(b1), _p(rs_t), _p(re_t), C.byref(opts), _p(feat), _p(depth),
                                      _p(wsum), _p(xyz), _p(ws), wsb, C.byref(dm) if dm is not None else None, _stream())
        else:
            rc = L.p3d_render_limits_f32(_p(planes_nhwc), N, H, W, _p(rays_o), _p(rays_d), R, int(ray_tile_w), _p(jitter), _p(u),
                                         _p(w0), _p(b0), _p(w1), _p(b1), _p(rs_t), _p(re_t), C.byref(opts), _p(feat), _p(depth),
                                         _p(wsum), _p(xyz), _p(ws), wsb, C.byref(dm) if dm is not None else None, _stream())
    _lib.check(rc, "p3d_render_rng_f32" if rng_seed is not None else "p3d_render_limits_f32")
    if stats is not None:  # synchronises: wave-level decode steps executed (32 samples each) vs the full count
        steps = int(ws[8:16].view(torch.int64).item())
        slots, tiles, full = render_plan_info(N, R, ray_tile_w, opts, dm is not None, rs_t is not None)[:3]
        kind = {1: None, 2: "pair", 4: "quad"}[slots]  # samples per wave-step, of 32 // slots rays each
        stats.update(decode_steps=steps, decode_steps_full=full, tiles=tiles, small_launch_kernel=kind is not None, small_launch_kind=kind)
        # which gather set-up the launch ran: the interior form (crop keeps the x / z taps inside the planes) or the generic one
        taps = L.p3d_render_taps_info(N, H, W, R, int(ray_tile_w or 0), C.byref(opts), int(dm is not None), int(rs_t is not None))
        _lib.check(min(taps, 0), "p3d_render_taps_info")
        stats.update(interior_taps=taps == 1)
    if weights_only:  # (feat / xyz may have been left unwritten)
        return None, depth, wsum, None
    return (feat, depth, wsum, xyz, d) if dumps else (feat, depth, wsum, xyz)


def render_plan_info(N, R, ray_tile_w, opts, has_dumps=False, has_ray_limits=False):
    """The launch render() makes for these arguments, as the library chose it (include/panic3d_hip.h p3d_render_plan_info):
    (samples per wave-step: 1 = k_render, 2 / 4 = k_render_slots; tiles; full decode steps; grid; block; dynamic LDS bytes)."""
    out = (C.c_int64 * 6)()
    _lib.check(_lib.lib().p3d_render_plan_info(N, R, int(ray_tile_w or 0), C.byref(opts), int(has_dumps), int(has_ray_limits), out, 6),
               "p3d_render_plan_info")
    return tuple(out)


def _grad_out(t, name, shape):
    if t is None:
        return None
    t = _chk(t, name)
    if t.numel() != int(np.prod(shape)):
        raise RuntimeError(f"{name} must hold {int(np.prod(shape))} values ({list(shape)})")
    return t


def _grad_buffers(planes_nhwc, dev, want_planes=True):
    dplanes = torch.zeros(planes_nhwc.shape, dtype=torch.float32, device=dev) if want_planes else None
    dmlp = (torch.empty((64, 32), dtype=torch.float32, device=dev), torch.empty((64,), dtype=torch.float32, device=dev),
            torch.empty((33, 64), dtype=torch.float32, device=dev), torch.empty((33,), dtype=torch.float32, device=dev))
    return dplanes, dmlp


def render_backward(planes_nhwc, rays_o, rays_d, depths_sorted, mlp, opts, grads, per_view_clamp=False, stats=None, want_planes=True):
    """Backward of render() (include/p3d_render_grad.h p3d_render_backward_f32) at the forward's merged depths
    (render(..., dumps=("depths_sorted",))).  grads = (g_feat [N,R,32], g_depth [N,R,1], g_wsum [N,R,1], g_xyz [N,R,3]), any
    None.  Returns (d_planes_nhwc shaped like planes_nhwc, (d_w0, d_b0, d_w1, d_b1)) — gradients of the pre-scaled decoder
    tensors.  opts: the forward's (per_view_clamp as passed to render).  stats: a dict receives the number of samples that ran
    the MLP backward (synchronises).  want_planes=False: decoder gradients only (d_planes_nhwc is None, no scatter)."""
    if per_view_clamp:
        opts = _with_flag(opts, _lib.P3D_FLAG_PER_VIEW_CLAMP)
    planes_nhwc = _chk(planes_nhwc, "planes_nhwc")
    rays_o, rays_d = _chk(rays_o, "ray_origins"), _chk(rays_d, "ray_directions")
    N, three, H, W, Cc = planes_nhwc.shape
    if N == 1 and rays_o.dim() == 3 and rays_o.shape[0] > 1:
        N, opts = rays_o.shape[0], _with_flag(opts, _lib.P3D_FLAG_SHARED_PLANES)
    if three != 3 or Cc != 32 or rays_o.dim() != 3 or rays_o.shape[0] != N or rays_o.shape[2] != 3 or rays_d.shape != rays_o.shape:
        raise RuntimeError("planes_nhwc must be [N,3,H,W,32] (or [1,...] shared by all views); ray_origins / ray_directions [N,R,3]")
    R, S = rays_o.shape[1], opts.Sc + opts.Sf
    depths_sorted = _grad_out(depths_sorted, "depths_sorted", (N * R, S))
    if depths_sorted is None:
        raise RuntimeError("render_backward needs the forward's depths_sorted dump")
    g_feat, g_depth, g_wsum, g_xyz = (_grad_out(g, n, sh) for g, n, sh in zip(
        grads, ("grad feat", "grad depth", "grad wsum", "grad xyz"), ((N, R, 32), (N, R, 1), (N, R, 1), (N, R, 3))))
    w0, b0, w1, b1 = _chk_mlp(mlp)
    dev = rays_o.device
    dplanes, dmlp = _grad_buffers(planes_nhwc, dev, want_planes)
    L = _lib.lib()
    wsb = L.p3d_render_backward_workspace_bytes(N, R, opts.Sc, opts.Sf)
    ws = torch.empty((wsb,), dtype=torch.uint8, device=dev)
    with _on(dev):
        rc = L.p3d_render_backward_f32(_p(planes_nhwc), N, H, W, _p(rays_o), _p(rays_d), R, _p(depths_sorted), _p(w0), _p(b0), _p(w1),
                                       _p(b1), C.byref(opts), _p(g_feat), _p(g_depth), _p(g_wsum), _p(g_xyz), _p(dplanes),
                                       *(_p(t) for t in dmlp), _p(ws), wsb, _stream())
    _lib.check(rc, "p3d_render_backward_f32")
    if stats is not None:
        stats.update(executed_samples=int(ws[:8].view(torch.int64).item()), samples=N * R * S)
    return dplanes, dmlp


def triplane_decode_backward(planes_nhwc, coords, mlp, opts, g_sigma, g_rgb, stats=None, want_planes=True):
    """Backward of triplane_decode() (p3d_triplane_decode_backward_f32): g_sigma [N,M,1], g_rgb [N,M,32] (either None) ->
    (d_planes_nhwc, (d_w0, d_b0, d_w1, d_b1)).  Masks of opts.flags zero the density gradient where they overwrite it."""
    planes_nhwc = _chk(planes_nhwc, "planes_nhwc")
    coords = _chk(coords, "coords")
    N, three, H, W, Cc = planes_nhwc.shape
    if N == 1 and coords.dim() == 3 and coords.shape[0] > 1:
        N, opts = coords.shape[0], _with_flag(opts, _lib.P3D_FLAG_SHARED_PLANES)
    if three != 3 or Cc != 32 or coords.dim() != 3 or coords.shape[0] != N or coords.shape[2] != 3:
        raise RuntimeError("planes_nhwc must be [N,3,H,W,32] (or [1,...] shared) and coords [N,M,3]")
    M = coords.shape[1]
    g_sigma = _grad_out(g_sigma, "grad sigma", (N, M, 1))
    g_rgb = _grad_out(g_rgb, "grad rgb", (N, M, 32))
    w0, b0, w1, b1 = _chk_mlp(mlp)
    dev = coords.device
    dplanes, dmlp = _grad_buffers(planes_nhwc, dev, want_planes)
    L = _lib.lib()
    wsb = L.p3d_triplane_decode_backward_workspace_bytes(N, M)
    ws = torch.empty((wsb,), dtype=torch.uint8, device=dev)
    with _on(dev):
        rc = L.p3d_triplane_decode_backward_f32(_p(planes_nhwc), N, H, W, _p(coords), M, _p(w0), _p(b0), _p(w1), _p(b1), C.byref(opts),
                                                _p(g_sigma), _p(g_rgb), _p(dplanes), *(_p(t) for t in dmlp), _p(ws), wsb, _stream())
    _lib.check(rc, "p3d_triplane_decode_backward_f32")
    if stats is not None:
        stats.update(executed_samples=int(ws[:8].view(torch.int64).item()), samples=N * M)
    return dplanes, dmlp


def sample_stratified(ray_start, ray_end, S, jitter):
    """sample_stratified (renderer.py:320-324): jitter [...,S(,1)] -> depths, same shape."""
    jitter = _chk(jitter, "jitter")
    out = torch.empty_like(jitter)
    NR = jitter.numel() // S
    with _on(jitter.device):
        rc = _lib.lib().p3d_sample_stratified_f32(np.float32(ray_start), np.float32(ray_end),
                                                  np.float32((float(ray_end) - float(ray_start)) / (S - 1)), int(S),
                                                  _p(jitter), NR, _p(out), _stream())
    _lib.check(rc, "p3d_sample_stratified_f32")
    return out


def composite(colors, densities, depths, white_back=True):
    """MipRayMarcher2.run_forward (ray_marcher.py:25-57): colors [N,R,S,K], densities [N,R,S,1], depths [N,R,S,1] ->
    (rgb [N,R,K], depth [N,R,1], weights [N,R,S-1,1])."""
    colors, densities, depths = _chk(colors, "colors"), _chk(densities, "densities"), _chk(depths, "depths")
    lead = colors.shape[:-2]
    S, K = colors.shape[-2], colors.shape[-1]
    NR = colors.numel() // (S * K)
    if densities.numel() != NR * S or depths.numel() != NR * S:
        raise RuntimeError("densities / depths must be [...,S,1] matching colors [...,S,K]")
    dev = colors.device
    rgb = torch.empty(lead + (K,), dtype=torch.float32, device=dev)
    depth = torch.empty(lead + (1,), dtype=torch.float32, device=dev)
    w = torch.empty(lead + (S - 1, 1), dtype=torch.float32, device=dev)
    ws = torch.empty((_lib.lib().p3d_composite_workspace_bytes(NR, S, K),), dtype=torch.uint8, device=dev)
    with _on(dev):
        rc = _lib.lib().p3d_composite_f32(_p(colors), _p(densities), _p(depths), NR, S, K, int(bool(white_back)), _p(rgb),
                                          _p(depth), _p(w), _p(ws), _stream())
    _lib.check(rc, "p3d_composite_f32")
    return rgb, depth, w


def paste_front(weights, xyz, occ, rays_o, rays_d, front, image, thresh_weight, thresh_edges, thresh_occ, thresh_dxyz, box_warp,
                normalize_images):
    """paste_front's masks + illustration sampling + lerp in one launch (p3d_paste_front_f32; training/triplane.py:607-691).
    weights / occ [N,1,r,r], xyz / rays_o / rays_d [N,3,r,r], front [N or 1,3,S,S], image [N,3,S,S] ->
    dict(image, paste, mask, mask_weights, mask_edges, mask_occ, mask_dxyz) at S x S."""
    weights, xyz, occ = _chk(weights, "weights"), _chk(xyz, "xyz"), _chk(occ, "occ")
    rays_o, rays_d, front, image = _chk(rays_o, "rays_o"), _chk(rays_d, "rays_d"), _chk(front, "front"), _chk(image, "image")
    if xyz.dim() != 4 or xyz.shape[1] != 3:  # (the kernel reads three channels of r x r whatever the tensor holds)
        raise RuntimeError("paste_front: xyz must be [N,3,r,r]")
    N, _, r, r2 = xyz.shape
    S = image.shape[-1]
    if (r != r2 or tuple(weights.shape) != (N, 1, r, r) or tuple(occ.shape) != (N, 1, r, r) or tuple(rays_o.shape) != (N, 3, r, r)
            or tuple(rays_d.shape) != (N, 3, r, r) or tuple(image.shape) != (N, 3, S, S) or front.shape[0] not in (1, N)
            or tuple(front.shape[1:]) != (3, S, S)):
        raise RuntimeError("paste_front: weights/occ [N,1,r,r], xyz/rays [N,3,r,r], front [N|1,3,S,S], image [N,3,S,S]")
    dev = image.device
    new = lambda c: torch.empty((N, c, S, S), dtype=torch.float32, device=dev)
    out = dict(image=new(3), paste=new(3), mask=new(1), mask_weights=new(1), mask_edges=new(1), mask_occ=new(1), mask_dxyz=new(1))
    a = _lib.PasteArgs(_p(weights).value, _p(xyz).value, _p(occ).value, _p(rays_o).value, _p(rays_d).value, _p(front).value,
                       _p(image).value, *[_p(out[k]).value for k in ("image", "paste", "mask", "mask_weights", "mask_edges", "mask_occ", "mask_dxyz")],
                       N, r, S, int(front.shape[0] == 1 and N > 1), int(bool(normalize_images)),
                       np.float32(thresh_weight), np.float32(thresh_edges), np.float32(thresh_occ), np.float32(thresh_dxyz), np.float32(box_warp))
    with _on(dev):
        rc = _lib.lib().p3d_paste_front_f32(C.byref(a), _stream())
    _lib.check(rc, "p3d_paste_front_f32")
    return out


def paste_front_backward(g_out, g_paste, mask, xyz, front, box_warp, normalize_images, grad_sample, want_image=True, want_xyz=False,
                         want_front=False):
    """p3d_paste_front_backward_f32 (include/p3d_paste_grad.h): the cotangents of the pasted image and of the returned paste (either
    may be None) -> (g_image [N,3,S,S], g_xyz [N,3,r,r], g_front like front), each None unless asked for.  g_xyz / g_front exist
    only with grad_sample (otherwise the paste is a constant)."""
    mask, xyz, front = _chk(mask, "mask"), _chk(xyz, "xyz"), _chk(front, "front")
    g_out = _chk(g_out, "g_out") if g_out is not None else None
    g_paste = _chk(g_paste, "g_paste") if g_paste is not None else None
    N, _, r, r2 = xyz.shape
    S = mask.shape[-1]
    if (r != r2 or xyz.shape[1] != 3 or tuple(mask.shape) != (N, 1, S, S) or front.shape[0] not in (1, N) or tuple(front.shape[1:]) != (3, S, S)
            or any(g is not None and tuple(g.shape) != (N, 3, S, S) for g in (g_out, g_paste))):
        raise RuntimeError("paste_front_backward: g_out/g_paste [N,3,S,S], mask [N,1,S,S], xyz [N,3,r,r], front [N|1,3,S,S]")
    if g_out is None and g_paste is None:
        raise RuntimeError("paste_front_backward: no cotangent")
    if (want_xyz or want_front) and not grad_sample:
        raise RuntimeError("paste_front_backward: g_xyz / g_front exist only with grad_sample")
    dev = mask.device
    g_image = torch.empty((N, 3, S, S), dtype=torch.float32, device=dev) if want_image else None
    g_xyz = torch.empty((N, 3, r, r), dtype=torch.float32, device=dev) if want_xyz else None
    g_front = torch.empty(tuple(front.shape), dtype=torch.float32, device=dev) if want_front else None
    if g_image is None and g_xyz is None and g_front is None:
        return None, None, None
    L = _lib.lib()
    ws = _sg_workspace(dev, L.p3d_paste_front_backward_workspace_bytes(N, S)) if want_xyz else None
    a = _lib.PasteGradArgs(_p(g_out).value, _p(g_paste).value, _p(mask).value, _p(xyz).value, _p(front).value, _p(g_image).value,
                           _p(g_xyz).value, _p(g_front).value, _p(ws).value, ws.numel() if ws is not None else 0,
                           N, r, S, int(front.shape[0] == 1 and N > 1), int(bool(normalize_images)), int(bool(grad_sample)), np.float32(box_warp))
    with _on(dev):
        rc = L.p3d_paste_front_backward_f32(C.byref(a), _stream())
    _lib.check(rc, "p3d_paste_front_backward_f32")
    return g_image, g_xyz, g_front


class _PasteFrontFn(torch.autograd.Function):
    """paste_front's one launch forward (the no-grad call's bits) with the HIP backward of include/p3d_paste_grad.h.  Differentiable
    inputs: image, and with grad_sample xyz and the illustration; the masks are constants, as in the reference (they are computed
    under no_grad there).  Returns (image, paste) and hands the masks out through `res`."""

    @staticmethod
    def forward(ctx, image, xyz, front, call, res):
        out = paste_front(call["weights"], xyz, call["occ"], call["rays_o"], call["rays_d"], front, image, *call["thresholds"],
                          call["box_warp"], call["normalize_images"])
        res.update(out)
        ctx.save_for_backward(out["mask"], xyz, front)
        ctx.call = call
        ctx.set_materialize_grads(False)  # an output nobody differentiates arrives as None, not as a tensor of zeros
        return out["image"], out["paste"]

    @staticmethod
    def backward(ctx, g_image, g_paste):
        mask, xyz, front = ctx.saved_tensors
        call = ctx.call
        gs = bool(call["grad_sample"])
        if not gs:
            g_paste = None  # the paste is a constant: its cotangent reaches nothing
        if g_image is None and g_paste is None:
            return None, None, None, None, None
        gi, gx, gf = paste_front_backward(g_image, g_paste, mask, xyz, front, call["box_warp"], call["normalize_images"], gs,
                                          want_image=ctx.needs_input_grad[0] and g_image is not None,
                                          want_xyz=gs and ctx.needs_input_grad[1], want_front=gs and ctx.needs_input_grad[2])
        return gi, gx, gf, None, None


def paste_front_grad(weights, xyz, occ, rays_o, rays_d, front, image, thresh_weight, thresh_edges, thresh_occ, thresh_dxyz, box_warp,
                     normalize_images, grad_sample=False):
    """ops.paste_front under autograd: the same launch and the same dict; `image` (and `paste`, with grad_sample) carry the HIP backward."""
    res = {}
    call = dict(weights=weights.detach(), occ=occ.detach(), rays_o=rays_o.detach(), rays_d=rays_d.detach(),
                thresholds=(thresh_weight, thresh_edges, thresh_occ, thresh_dxyz), box_warp=box_warp, normalize_images=normalize_images,
                grad_sample=grad_sample)
    img, paste = _PasteFrontFn.apply(image, xyz if grad_sample else xyz.detach(), front if grad_sample else front.detach(), call, res)
    res["image"], res["paste"] = img, paste if grad_sample else paste.detach()
    return res


def depth_minmax(depths):
    """torch.min(depths), torch.max(depths) of ray_marcher.py:50 as one op -> float32 tensor [2] on the device."""
    depths = _chk(depths, "depths")
    out = torch.empty((2,), dtype=torch.float32, device=depths.device)
    ws = torch.empty((16,), dtype=torch.uint8, device=depths.device)
    with _on(depths.device):
        rc = _lib.lib().p3d_depth_minmax_f32(_p(depths), depths.numel(), _p(out), _p(ws), 16, _stream())
    _lib.check(rc, "p3d_depth_minmax_f32")
    return out


def importance(depths, weights, u, return_inds=False):
    """sample_importance (renderer.py:328-346): depths [N,R,Sc,1], weights [N,R,Sc-1,1], u [N*R,Sf] -> [N,R,Sf,1]."""
    depths, weights, u = _chk(depths, "depths"), _chk(weights, "weights"), _chk(u, "u")
    Sf = u.shape[-1]
    NR = u.numel() // Sf
    Sc = depths.numel() // NR
    if weights.numel() != NR * (Sc - 1):
        raise RuntimeError("weights must hold Sc-1 values per ray")
    out = torch.empty(tuple(depths.shape[:2]) + (Sf, 1) if depths.dim() == 4 else (NR, Sf), dtype=torch.float32, device=u.device)
    inds = torch.empty((NR, Sf), dtype=torch.int32, device=u.device) if return_inds else None
    with _on(u.device):
        rc = _lib.lib().p3d_importance_f32(_p(depths), _p(weights), NR, Sc, Sf, _p(u), _p(out), _p(inds), _stream())
    _lib.check(rc, "p3d_importance_f32")
    return (out, inds) if return_inds else out


def unify_perm(depths_coarse, depths_fine):
    """The sort of unify_samples (renderer.py:295): stable ascending permutation of cat([coarse, fine]) per ray -> int32 [NR,S]."""
    dc, df = _chk(depths_coarse, "depths_coarse"), _chk(depths_fine, "depths_fine")
    NR = dc.shape[0] if dc.dim() == 2 else dc.numel() // dc.shape[-2]
    Sc, Sf = dc.numel() // NR, df.numel() // NR
    perm = torch.empty((NR, Sc + Sf), dtype=torch.int32, device=dc.device)
    with _on(dc.device):
        rc = _lib.lib().p3d_unify_perm_f32(_p(dc), _p(df), NR, Sc, Sf, _p(perm), _stream())
    _lib.check(rc, "p3d_unify_perm_f32")
    return perm


# ======================================================================================================================
# StyleGAN2 synthesis operators (torch_utils/ops/{bias_act,upfirdn2d,conv2d_resample}.py, networks_stylegan2.py:40-97)
# ======================================================================================================================
_ACTS = {"linear": (0, 0.0, 1.0), "lrelu": (1, 0.2, float(np.sqrt(2)))}  # bias_act.py:23-33: index, def_alpha, def_gain


def bias_act(x, b=None, dim=1, act="linear", alpha=None, gain=None, clamp=None):
    """bias_act.bias_act (bias_act.py:54-88): clamp(act(x + b) * gain).  Only 'linear' and 'lrelu' are on the hot path."""
    x = _chk(x, "x")
    if act not in _ACTS:
        raise NotImplementedError(f"activation {act!r} is not used by the PAniC-3D generator")
    assert clamp is None or clamp >= 0  # bias_act.py:98
    idx, da, dg = _ACTS[act]
    alpha = float(alpha if alpha is not None else da)
    gain = float(gain if gain is not None else dg)
    clamp = float(clamp if clamp is not None else -1)
    if b is not None:
        b = _chk(b, "b")
        assert b.ndim == 1 and 0 <= dim < x.ndim and b.shape[0] == x.shape[dim]  # bias_act.py:105-107
    C = x.shape[dim]
    outer = int(np.prod(x.shape[:dim])) if dim > 0 else 1
    inner = int(np.prod(x.shape[dim + 1:])) if dim + 1 < x.ndim else 1
    y = torch.empty_like(x)
    with _on(x.device):
        rc = _lib.lib().p3d_bias_act_f32(_p(x), _p(b), outer, C, inner, idx, alpha, gain, clamp, _p(y), _stream())
    _lib.check(rc, "p3d_bias_act_f32")
    return y


def setup_filter(f=(1, 3, 3, 1), device=None):
    """upfirdn2d.setup_filter (upfirdn2d.py:72-117) for the non-separable case: outer product, normalised to DC gain 1."""
    f = torch.as_tensor(f, dtype=torch.float32)
    if f.ndim == 1:
        f = f.ger(f)
    f = f / f.sum()
    return f.to(device) if device is not None else f


def _parse_padding(padding):
    if isinstance(padding, int):
        padding = [padding, padding]
    padding = list(padding)
    if len(padding) == 2:
        padding = [padding[0], padding[0], padding[1], padding[1]]
    return [int(v) for v in padding]


_FIR_CACHE = {}
# A list while TriPlaneGenerator captures a view into a hipGraph (generator._capture_view), else None: every device tensor that a
# process-wide cache below hands to the captured launches is appended, and the capture keeps it alive.  A cache may drop its
# tensor later (a bigger workspace, _FIR_CACHE.clear()), and torch.cuda.graph empties the allocator's cache before every capture:
# a block that only the cache held can go back to the device while a capture still has its address baked into its launches.
CAPTURE_KEEP = None


def _kept(t):
    if CAPTURE_KEEP is not None:
        CAPTURE_KEEP.append(t)
    return t


def prepared_filter(f, device, gain=1.0, flip_filter=False):
    """`f * gain`, flipped for convolution unless flip_filter (upfirdn2d.py:193-196), float32 contiguous on `device` — made
    once per (filter tensor object, version, gain, flip): the reference rebuilds it on every call (three tiny launches)."""
    key = (id(f), device, float(gain), bool(flip_filter))
    hit = _FIR_CACHE.get(key)
    if memo.enabled() and hit is not None and hit[0]() is f and hit[1] == f._version:
        return _kept(hit[2])
    ff = f.detach().to(device, torch.float32) * float(gain)
    if not flip_filter:
        ff = ff.flip([0, 1])
    ff = ff.contiguous()
    if len(_FIR_CACHE) > 256:
        _FIR_CACHE.clear()
    _FIR_CACHE[key] = (weakref.ref(f), f._version, ff)
    return _kept(ff)


def upfirdn2d(x, f, up=1, down=1, padding=0, flip_filter=False, gain=1):
    """upfirdn2d.upfirdn2d (upfirdn2d.py:120-167), 2-D filter, same up/down factor in x and y."""
    x = _chk(x, "x")
    if x.ndim != 4 or f is None or f.ndim != 2:
        raise NotImplementedError("upfirdn2d: [N,C,H,W] input and a 2-D filter are what the generator uses")
    px0, px1, py0, py1 = _parse_padding(padding)
    ff = prepared_filter(f, x.device, gain, flip_filter)
    N, Cc, H, W = x.shape
    fh, fw = ff.shape
    if H * up + py0 + py1 < fh or W * up + px0 + px1 < fw:
        raise RuntimeError(f"upfirdn2d: the padded input ({H * up + py0 + py1} x {W * up + px0 + px1}) is smaller than the "
                           f"{fh} x {fw} filter: no output")
    OH = (H * up + py0 + py1 - fh) // down + 1
    OW = (W * up + px0 + px1 - fw) // down + 1
    y = torch.empty((N, Cc, OH, OW), dtype=torch.float32, device=x.device)
    with _on(x.device):
        rc = _lib.lib().p3d_upfirdn2d_f32(_p(x), N * Cc, H, W, _p(ff), fh, fw, int(up), int(down), px0, px1, py0, py1, _p(y), _stream())
    _lib.check(rc, "p3d_upfirdn2d_f32")
    return y


def upsample2d(x, f, up=2, padding=0, flip_filter=False, gain=1):
    """upfirdn2d.upsample2d (upfirdn2d.py:315-350).  Differentiable in x under autograd (the adjoint is upfirdn2d with the flipped
    filter, upfirdn2d.py:236-245)."""
    if _wants_grad(x):
        return _Upsample2dFn.apply(x, (f, up, padding, flip_filter, gain))
    return _upsample2d_impl(x, f, up, padding, flip_filter, gain)


def _upsample2d_impl(x, f, up=2, padding=0, flip_filter=False, gain=1):
    px0, px1, py0, py1 = _parse_padding(padding)
    fh, fw = f.shape
    p = [px0 + (fw + up - 1) // 2, px1 + (fw - up) // 2, py0 + (fh + up - 1) // 2, py1 + (fh - up) // 2]
    return upfirdn2d(x, f, up=up, padding=p, flip_filter=flip_filter, gain=gain * up * up)


def upsample2d_add(x, f, add=None):
    """`upsample2d(x, f)` (up = 2, the 4x4 resample filter) fused with the `img.add_(y)` that follows it in SynthesisBlock.forward
    (networks_stylegan2.py:476-478): returns upsample2d(x, f) + add in one launch (polyphase FIR, same bits as upfirdn2d)."""
    x = _chk(x, "x")
    N, Cc, H, W = x.shape
    if add is not None:
        add = _chk(add, "add")
        if tuple(add.shape) != (N, Cc, 2 * H, 2 * W):
            raise RuntimeError("add must be [N,C,2H,2W]")
    # the fused kernel moves float4 rows: a 2W that is no multiple of 4, or an `add` that is not 16-byte aligned (a contiguous view at
    # a storage offset), takes the generic operator (the library's P3D_E_RANGE says the same)
    if tuple(f.shape) != (4, 4) or (2 * W) % 4 != 0 or (add is not None and add.data_ptr() % 16 != 0):
        y = upsample2d(x, f)
        return y if add is None else y.add_(add)
    ff = prepared_filter(f, x.device, 4.0, False)
    y = torch.empty((N, Cc, 2 * H, 2 * W), dtype=torch.float32, device=x.device)
    with _on(x.device):
        rc = _lib.lib().p3d_upsample2d_add_f32(_p(x), N * Cc, H, W, _p(ff), _p(add), _p(y), _stream())
    _lib.check(rc, "p3d_upsample2d_add_f32")
    return y


def torgb_weights(weight):
    """ToRGB weights [O,I,1,1] -> the transposed, channel-padded [I, 32 or 96] copy p3d_torgb_f32 streams (made once per layer).
    Under autograd (weight requires grad) the copy carries the gradient back to weight."""
    if _wants_grad(weight):
        return _TorgbWeightsFn.apply(weight)
    return _torgb_weights_impl(weight)


def _torgb_weights_impl(weight):
    weight = _chk(weight, "weight")
    O, I = weight.shape[0], weight.shape[1]
    if weight.shape[2:] != (1, 1) or O > 96:
        raise RuntimeError("torgb_weights: [O <= 96, I, 1, 1]")
    wt = torch.empty((I, 32 if O <= 32 else 96), dtype=torch.float32, device=weight.device)
    with _on(weight.device):
        _lib.check(_lib.lib().p3d_torgb_weights_f32(_p(weight), O, I, _p(wt), _stream()), "p3d_torgb_weights_f32")
    return wt


def torgb(x, weight_t, out_channels, styles, bias=None, clamp=None, skip=None, skip_filter=None):
    """ToRGBLayer.forward (networks_stylegan2.py:366-380) + the skip connection of SynthesisBlock.forward (:476-478) in ONE launch:
    `upsample2d(skip, skip_filter) + (conv1x1(x * styles) + bias)`.  weight_t from torgb_weights; styles [N,I] already multiplied
    by the layer's weight_gain; skip [N,O,H/2,W/2] or None.  Differentiable under autograd (_TorgbFn: the HIP backward)."""
    if _wants_grad(x, weight_t, styles, bias, skip):
        return _TorgbFn.apply(x, weight_t, styles, bias, skip, (int(out_channels), clamp, skip_filter))
    return _torgb_impl(x, weight_t, out_channels, styles, bias, clamp, skip, skip_filter)


def _torgb_impl(x, weight_t, out_channels, styles, bias=None, clamp=None, skip=None, skip_filter=None):
    x, weight_t, styles = _chk(x, "x"), _chk(weight_t, "weight_t"), _chk(styles, "styles")
    N, I, H, W = x.shape
    O = int(out_channels)
    if tuple(weight_t.shape) != (I, 32 if O <= 32 else 96) or tuple(styles.shape) != (N, I):
        raise RuntimeError("torgb: x [N,I,H,W], weight_t [I,32|96] (torgb_weights), styles [N,I]")
    if bias is not None:
        bias = _chk(bias, "bias")
    skipf = None
    if skip is not None:
        skip = _chk(skip, "skip")
        if tuple(skip.shape) != (N, O, H // 2, W // 2) or H % 2 or W % 2:
            raise RuntimeError("skip must be [N,O,H/2,W/2] (the previous block's image)")
        skipf = prepared_filter(skip_filter, x.device, 4.0, False)  # upsample2d: up 2, gain up^2 (upfirdn2d.py:341-350)
        if tuple(skipf.shape) != (4, 4):
            raise NotImplementedError("skip_filter must be the 4x4 [1,3,3,1] filter")
    y = torch.empty((N, O, H, W), dtype=torch.float32, device=x.device)
    with _on(x.device):
        rc = _lib.lib().p3d_torgb_f32(_p(x), N, I, H, W, _p(weight_t), O, _p(styles), _p(bias), float(clamp if clamp is not None else -1),
                                      _p(skip), _p(skipf), _p(y), _stream())
    _lib.check(rc, "p3d_torgb_f32")
    return y


_FUSES_TORGB = {}


def conv_fuses_torgb(N, I, O, H, W, rgb_channels):
    """The LIBRARY's rule (p3d_conv_fuses_torgb) for when a plain 3x3 layer of this shape takes its block's ToRGB layer along
    (modulated_conv2d(..., rgb_weight=, rgb_styles=)); asked, not restated; memoised like takes_image."""
    key = (int(N), int(I), int(O), int(H), int(W), int(rgb_channels))
    r = _FUSES_TORGB.get(key)
    if r is None:
        r = _FUSES_TORGB[key] = bool(_lib.lib().p3d_conv_fuses_torgb(*key))
    return r


def torgb_combine(partial, bias=None, clamp=None, skip=None, skip_filter=None, x=None, weight=None, styles=None):
    """The second half of a ToRGB layer whose channel sums came out of conv1's launch (modulated_conv2d(..., rgb_weight=...)):
    partial [tiles,N,O,H,W] -> `upsample2d(skip, skip_filter) + (sum over tiles + bias)` [N,O,H,W] (p3d_torgb_combine_f32).
    Under autograd the layer's own inputs say what the shares were made of — x (conv1's fp32 result [N,I,H,W]), weight (the ToRGB
    parameter [O,I,1,1]) and styles [N,I] — and the HIP backward is recorded (_TorgbCombineFn); the shares themselves carry no
    gradient."""
    if x is not None and _wants_grad(x, weight, styles, bias, skip):
        return _TorgbCombineFn.apply(x, weight, styles, bias, skip, partial, (clamp, skip_filter))
    return _torgb_combine_impl(partial, bias, clamp, skip, skip_filter)


def _torgb_combine_impl(partial, bias=None, clamp=None, skip=None, skip_filter=None):
    partial = _chk(partial, "partial")
    T, N, O, H, W = partial.shape
    if bias is not None:
        bias = _chk(bias, "bias")
    skipf = None
    if skip is not None:
        skip = _chk(skip, "skip")
        if tuple(skip.shape) != (N, O, H // 2, W // 2) or H % 2 or W % 2:
            raise RuntimeError("skip must be [N,O,H/2,W/2] (the previous block's image)")
        skipf = prepared_filter(skip_filter, partial.device, 4.0, False)
        if tuple(skipf.shape) != (4, 4):
            raise NotImplementedError("skip_filter must be the 4x4 [1,3,3,1] filter")
    y = torch.empty((N, O, H, W), dtype=torch.float32, device=partial.device)
    with _on(partial.device):
        rc = _lib.lib().p3d_torgb_combine_f32(_p(partial), T, N, O, H, W, _p(bias), float(clamp if clamp is not None else -1), _p(skip),
                                              _p(skipf), _p(y), _stream())
    _lib.check(rc, "p3d_torgb_combine_f32")
    return y


def torgb_combine_backward(partial, g_img, bias=None, clamp=None, skip_filter=None, want_bias=True):
    """p3d_torgb_combine_backward_f32: (g_y [N,O,H,W] = g_img where the forward's own pre-clamp sums passed the clamp, else 0;
    g_bias [O] or None; g_skip [N,O,H/2,W/2] — the adjoint of the up-sampled skip image — when skip_filter is given, else None)."""
    partial, g_img = _chk(partial, "partial"), _chk(g_img, "g_img")
    T, N, O, H, W = partial.shape
    if tuple(g_img.shape) != (N, O, H, W):
        raise RuntimeError("torgb_combine_backward: g_img [N,O,H,W] of partial [tiles,N,O,H,W]")
    if bias is not None:
        bias = _chk(bias, "bias")
    g_y = torch.empty_like(g_img)
    g_b = torch.empty((O,), dtype=torch.float32, device=g_img.device) if want_bias else None
    skipf = g_skip = None
    if skip_filter is not None:
        skipf = prepared_filter(skip_filter, g_img.device, 4.0, False)  # the forward's filter: the kernel applies its adjoint
        if tuple(skipf.shape) != (4, 4):
            raise NotImplementedError("skip_filter must be the 4x4 [1,3,3,1] filter")
        g_skip = torch.empty((N, O, H // 2, W // 2), dtype=torch.float32, device=g_img.device)
    with _on(g_img.device):
        rc = _lib.lib().p3d_torgb_combine_backward_f32(_p(partial), T, N, O, H, W, _p(bias), float(clamp if clamp is not None else -1),
                                                       _p(g_img), _p(g_y), _p(g_b), _p(skipf), _p(g_skip), _stream())
    _lib.check(rc, "p3d_torgb_combine_backward_f32")
    return g_y, g_b, g_skip


class WeightOperand(torch.Tensor):
    """The two-term copy of a layer's weights in one of the image layouts (P3D_WLAYOUT_PLAIN / _UP: the consuming kernel's LDS image per
    chunk and channel tile, include/panic3d_hip.h): the same [2,O,9,I] float16 storage size, ANOTHER element order — the subclass
    carries which one (`p3d_layout`) so that modulated_conv2d can tell the library."""
    p3d_layout = 0


_WLAYOUT = {}


def conv_weight_layout(I, O, W, up):
    """The layout of the two-term weight copy the LIBRARY wants for a 3x3 layer of this shape (p3d_conv_weight_layout; W: the input
    map's width): asked, not restated; fixed for the life of the process."""
    key = (int(I), int(O), int(W), int(up))
    r = _WLAYOUT.get(key)
    if r is None:
        r = _WLAYOUT[key] = int(_lib.lib().p3d_conv_weight_layout(*key))
    return r


def conv_weights_to_f16(weight, split=False, layout=0):
    """[O,I,k,k] f32 -> the [O,k*k,I] f16 operand copy of the f16-operand convolution (made once per layer); split: the
    [2,O,k*k,I] hi / lo pair of the two-term variant (hi = f16(w), lo = f16(w - hi)).  layout (split, 3x3): conv_weight_layout(...) of
    the layer the copy is for — non-zero: a WeightOperand in that image layout (same bytes, the pipelined kernels' own order)."""
    weight = _chk(weight, "weight")
    O, I, kh, kw = weight.shape
    wh = torch.empty((2, O, kh * kw, I) if split else (O, kh * kw, I), dtype=torch.float16, device=weight.device)
    if layout:
        if not split:
            raise RuntimeError("conv_weights_to_f16: the image layouts are two-term layouts (split=True)")
        with _on(weight.device):
            _lib.check(_lib.lib().p3d_conv_weights_to_f16x2_layout(_p(weight), O, I, kh, int(layout), _p(wh), _stream()), "p3d_conv_weights_to_f16x2_layout")
        wh = wh.as_subclass(WeightOperand)
        wh.p3d_layout = int(layout)
        return wh
    with _on(weight.device):
        if split:
            _lib.check(_lib.lib().p3d_conv_weights_to_f16x2(_p(weight), O, I, kh, _p(wh), _stream()), "p3d_conv_weights_to_f16x2")
        else:
            _lib.check(_lib.lib().p3d_conv_weights_to_f16(_p(weight), O, I, kh, _p(wh), _stream()), "p3d_conv_weights_to_f16")
    return wh


def conv_domain_flag(device):
    """A caller-owned flag word for the two-term f16 convolutions (`saturated` argument of p3d_modconv2d_f16x2mma_f32, ABI 5): the
    kernels OR it with 1 when a modulated activation leaves the domain |s*x| <= 4094 (or is NaN).  Zeroed here."""
    return torch.zeros(1, dtype=torch.int32, device=device)


def conv_domain_violated(flag, reset=True):
    """Read a conv_domain_flag (synchronises the stream); reset: zero it again."""
    hit = bool(flag.item() != 0)
    if hit and reset:
        flag.zero_()
    return hit


def demod_coefs(w2_all, styles_all, table, L, N, total_waves, out):
    """Demodulation coefficients of L layers in one launch (p3d_demod_coefs_f32); see stylegan2.StylePlan."""
    with _on(out.device):
        rc = _lib.lib().p3d_demod_coefs_f32(_p(w2_all), _p(styles_all), _p(table), int(L), int(N), int(total_waves), _p(out), _stream())
    _lib.check(rc, "p3d_demod_coefs_f32")
    return out


_CONV_SCRATCH = {}  # (device index, stream handle) -> workspace tensor
_WSB = {}           # (N, I, O, H, W, up) -> p3d_modconv2d_workspace_bytes (a pure function of the shape)


def _conv_scratch(device, nbytes):
    """The convolution workspace (demodulation coefficients, the transposed-conv intermediate, split-K partial sums), per
    (device, stream): launches on one stream are ordered, so consecutive convolutions share ONE workspace instead of allocating
    one per call (the batch-1 backbone is host-bound in its 4^2 .. 32^2 layers)."""
    idx = device.index if device.index is not None else _cur_device()
    key = (idx, _raw_stream(idx))
    ws = _CONV_SCRATCH.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty((int(nbytes * 1.25) + 4096,), dtype=torch.uint8, device=device)
        _CONV_SCRATCH[key] = ws
    return _kept(ws)


class ActImage:
    """The operand of a plain 3x3 two-term layer prepared by the layer in front of it (include/panic3d_hip.h, "activation IMAGE"):
    data = float16 [2 (hi | lo), N, C/8, H, W, 8] holding split(16 * styles * x) for the CONSUMER's styles.  Produced by an
    up-sampling modulated_conv2d called with next_styles=... (or act_to_image); consumed by modulated_conv2d in place of x."""
    __slots__ = ("data", "shape")

    def __init__(self, data, shape):
        self.data, self.shape = data, tuple(shape)

    @staticmethod
    def empty(N, C, H, W, device):
        if C % 8:
            raise RuntimeError("ActImage: C % 8 != 0")
        return ActImage(torch.empty((2, N, C // 8, H, W, 8), dtype=torch.float16, device=device), (N, C, H, W))

    @property
    def device(self):
        return self.data.device

    def float(self):
        """(hi + lo) / 16 as fp32 [N,C,H,W]: the MODULATED activation styles * x (tests)."""
        N, C, H, W = self.shape
        v = (self.data[0].float() + self.data[1].float()) * (1.0 / 16.0)
        return v.permute(0, 1, 4, 2, 3).reshape(N, C, H, W).contiguous()


_TAKES_IMAGE = {}


def takes_image(I, O, W, up):
    """The LIBRARY's rule for when a 3x3 layer with these sizes stages its input from an ActImage (p3d_conv_takes_image: k_modconv_w3 for
    up = 1, k_modconv_up3 for up = 2) — asked, not restated, so that the host's choice of hand-overs and the library's acceptance of
    x_img cannot drift apart; fixed for the life of the process, hence memoised."""
    key = (int(I), int(O), int(W), int(up))
    r = _TAKES_IMAGE.get(key)
    if r is None:
        r = _TAKES_IMAGE[key] = bool(_lib.lib().p3d_conv_takes_image(*key))
    return r


def takes_image_up(I, O, W):
    """An up-sampling 3x3 layer with these sizes stages its input from an ActImage (k_modconv_up3)."""
    return takes_image(I, O, W, 2)


def act_to_image(x, styles=None, saturated=None):
    """p3d_act_to_image_f32: fp32 [N,C,H,W] (* styles [N,C]) -> ActImage."""
    x = _chk(x, "x")
    N, C, H, W = x.shape
    if styles is not None:
        styles = _chk(styles, "styles")
        if tuple(styles.shape) != (N, C):
            raise RuntimeError("act_to_image: styles [N,C]")
    img = ActImage.empty(N, C, H, W, x.device)
    with _on(x.device):
        _lib.check(_lib.lib().p3d_act_to_image_f32(_p(x), _p(styles), N, C, H, W, _p(img.data), _p(saturated), _stream()), "p3d_act_to_image_f32")
    return img


def act_to_image_add(x, styles, add, c0, saturated=None):
    """p3d_act_to_image_add_f32: `x[:, c0 : c0 + add.shape[1]] += add` IN PLACE (add [1 or N, Ca, H, W]) and the ActImage of the updated
    x for a consumer with `styles` — the conditioning add between two synthesis blocks and the conversion pass in one launch."""
    if not (isinstance(x, torch.Tensor) and x.is_contiguous()):
        raise RuntimeError("act_to_image_add: x is updated in place and must be contiguous")
    x, styles, add = _chk(x, "x"), _chk(styles, "styles"), _chk(add, "add")
    N, C, H, W = x.shape
    if add.ndim != 4 or tuple(add.shape[2:]) != (H, W) or add.shape[0] not in (1, N) or tuple(styles.shape) != (N, C):
        raise RuntimeError("act_to_image_add: x [N,C,H,W], styles [N,C], add [1|N,Ca,H,W]")
    img = ActImage.empty(N, C, H, W, x.device)
    with _on(x.device):
        _lib.check(_lib.lib().p3d_act_to_image_add_f32(_p(x), _p(styles), N, C, H, W, _p(add), int(c0), int(add.shape[1]), int(add.shape[0]),
                                                       _p(img.data), _p(saturated), _stream()), "p3d_act_to_image_add_f32")
    return img


def modulated_conv2d(x, weight, styles, noise=None, up=1, padding=0, resample_filter=None, demodulate=True,
                     bias=None, act="linear", gain=None, clamp=None, weight_f16=None, dcoef=None, saturated=None,
                     next_styles=None, rgb_weight=None, rgb_styles=None, want_y=True):
    """modulated_conv2d (networks_stylegan2.py:40-97) FUSED with the bias_act that follows it in SynthesisLayer.forward
    (:350-352) / ToRGBLayer.forward (:379).  Supported shapes are the generator's: 3x3 / padding 1 / up 1 or 2, and 1x1.
    noise: None, [H,W] / [1,1,H,W] (noise_const * strength, shared) or [N,1,H,W] (random * strength); other shapes raise.
    weight_f16 (from conv_weights_to_f16): run the matrix cores on f16 operands (fp32 accumulate, fp32 in/out) — what the
    reference's fp16 super-resolution blocks do on the GPU, with less rounding; needs I % 16 == 0.  A [2,O,k*k,I] tensor
    (conv_weights_to_f16(split=True)) selects the two-term variant: fp32-class results on the f16 matrix cores; `saturated`: an
    int32 [1] device tensor of the caller (conv_domain_flag) that the two-term kernels OR with 1 when |s*x| > 4094.
    x may be an ActImage (3x3, up 1, two-term weights, dcoef given: styles are already in it).  next_styles [N,O] (up 2 only):
    return the result as the ActImage of a following layer with those styles instead of an fp32 tensor.
    rgb_weight [R<=4,O] + rgb_styles [N,O] (plain 3x3 layer with an ActImage input, only where conv_fuses_torgb(...) says so): the
    block's ToRGB layer rides on this launch — the call returns (y, image or None, partial [O/64,N,R,H,W]) and torgb_combine(partial,
    ...) finishes the ToRGB layer; want_y=False: y is not written (None is returned in its place).  With rgb_weight, x may also be the
    fp32 tensor: the layer then stages it as its own activation image first (act_to_image with its styles: the hand-over's bits)."""
    if rgb_weight is not None and isinstance(x, torch.Tensor):
        if _wants_grad(x, weight, styles, noise, bias, dcoef):
            # under autograd (the super-resolution's riding ToRGB): y is written for the backward; the shares carry no gradient —
            # torgb_combine(..., x=y, weight=, styles=) records the ToRGB layer's own backward
            y, part = _ModConvFn.apply(x, weight, styles, dcoef, bias, noise,
                                       dict(up=int(up), padding=padding, resample_filter=resample_filter, demodulate=bool(demodulate), act=act,
                                            gain=gain, clamp=clamp, weight_f16=weight_f16, saturated=saturated,
                                            ride=(rgb_weight.detach(), rgb_styles.detach())))
            return y, None, part
        x = act_to_image(x, styles, saturated=saturated)
    if _wants_grad(x if isinstance(x, torch.Tensor) else None, weight, styles, noise, bias, dcoef):
        # under autograd: the HIP backward (_ModConvFn); the hand-overs below are inference-only
        if isinstance(x, ActImage) or next_styles is not None:
            raise RuntimeError("modulated_conv2d: activation images and next_styles are inference-only (call under torch.no_grad())")
        return _ModConvFn.apply(x, weight, styles, dcoef, bias, noise,
                                dict(up=int(up), padding=padding, resample_filter=resample_filter, demodulate=bool(demodulate), act=act, gain=gain,
                                     clamp=clamp, weight_f16=weight_f16, saturated=saturated))
    return _modulated_conv2d_impl(x, weight, styles, noise, up, padding, resample_filter, demodulate, bias, act, gain, clamp, weight_f16,
                                  dcoef, saturated, next_styles, rgb_weight, rgb_styles, want_y)


def _modulated_conv2d_impl(x, weight, styles, noise=None, up=1, padding=0, resample_filter=None, demodulate=True,
                           bias=None, act="linear", gain=None, clamp=None, weight_f16=None, dcoef=None, saturated=None,
                           next_styles=None, rgb_weight=None, rgb_styles=None, want_y=True):
    ximg = x if isinstance(x, ActImage) else None
    if ximg is not None:
        if up == 2 and not takes_image_up(ximg.shape[1], weight.shape[0], ximg.shape[3]):
            raise RuntimeError("modulated_conv2d: the library does not stage this up-sampling layer from an ActImage (p3d_conv_takes_image: I % 16 == 0, O % 32 == 0, W >= 4)")
        if weight_f16 is None or weight_f16.ndim != 4 or (demodulate and dcoef is None):
            raise RuntimeError("modulated_conv2d: an ActImage input needs two-term weights (conv_weights_to_f16(split=True)) and precomputed dcoef")
        x = None
        weight = _chk(weight, "weight")
        N, I, H, W = ximg.shape
    else:
        x, weight, styles = _chk(x, "x"), _chk(weight, "weight"), _chk(styles, "styles")
        N, I, H, W = x.shape
    O, I2, kh, kw = weight.shape
    if I2 != I or (ximg is None and tuple(styles.shape) != (N, I)):
        raise RuntimeError("modulated_conv2d: x [N,I,H,W], weight [O,I,k,k], styles [N,I]")
    dev_ = ximg.device if ximg is not None else x.device
    if not ((kh == kw == 3 and padding == 1 and up in (1, 2)) or (kh == kw == 1 and padding == 0 and up == 1)):
        raise NotImplementedError("modulated_conv2d: only 3x3/pad 1/up 1|2 and 1x1 are on the hot path")
    idx, da, dg = _ACTS[act]
    gain = float(gain if gain is not None else dg)
    clampv = float(clamp if clamp is not None else -1)
    nps = 0
    if noise is not None:
        noise = _chk(noise, "noise")
        # exactly the documented shapes: any other layout with N*H*W elements would be read as ONE shared map
        if tuple(noise.shape) not in ((H * up, W * up), (1, 1, H * up, W * up), (N, 1, H * up, W * up)):
            raise RuntimeError("noise must be [H*up, W*up], [1,1,H*up,W*up] or [N,1,H*up,W*up]")
        nps = 1 if noise.shape[0] == N and noise.ndim == 4 and N > 1 else 0
    fir = None
    if up == 2:
        fir = prepared_filter(resample_filter, dev_, 4.0, False)  # upfirdn2d.py:193-196, gain = up^2
        if tuple(fir.shape) != (4, 4):
            raise NotImplementedError("resample_filter must be the 4x4 [1,3,3,1] filter")
    if bias is not None:
        bias = _chk(bias, "bias")
    if dcoef is not None:
        dcoef = _chk(dcoef, "dcoef")
        if dcoef.numel() != N * O:
            raise RuntimeError("dcoef must hold N*O demodulation coefficients")
    out_image = next_styles is not None
    if out_image:
        next_styles = _chk(next_styles, "next_styles")
        if tuple(next_styles.shape) != (N, O) or kh != 3:
            raise RuntimeError("next_styles [N,O] goes with a 3x3 layer")
    both = out_image and up == 1  # a plain layer writes the image NEXT TO the fp32 result (ToRGB reads the one, the next conv0 the other)
    rgb = rgb_weight is not None
    rgbp = None
    if rgb:
        rgb_weight, rgb_styles = _chk(rgb_weight, "rgb_weight"), _chk(rgb_styles, "rgb_styles")
        R = rgb_weight.shape[0]
        if ximg is None or up != 1 or kh != 3 or tuple(rgb_weight.shape) != (R, O) or tuple(rgb_styles.shape) != (N, O) \
                or not conv_fuses_torgb(N, I, O, H, W, R):
            raise RuntimeError("modulated_conv2d: rgb_weight [R,O] / rgb_styles [N,O] go with a plain 3x3 layer fed by an ActImage whose "
                               "shape conv_fuses_torgb accepts")
        rgbp = torch.empty((O // 64, N, R, H, W), dtype=torch.float32, device=dev_)
    y = None if ((out_image and not both) or (rgb and not want_y)) else torch.empty((N, O, H * up, W * up), dtype=torch.float32, device=dev_)
    yimg = ActImage.empty(N, O, H * up, W * up, dev_) if out_image else None
    L = _lib.lib()
    mma = _lib.P3D_CONV_MMA_F32
    if weight_f16 is not None:
        split = weight_f16.ndim == 4
        if weight_f16.dtype != torch.float16 or tuple(weight_f16.shape)[-3:] != (O, kh * kw, I) or not weight_f16.is_contiguous() \
                or (split and weight_f16.shape[0] != 2):
            raise RuntimeError("weight_f16 must be the contiguous [O,k*k,I] / [2,O,k*k,I] float16 tensor of conv_weights_to_f16")
        mma = _lib.P3D_CONV_MMA_F16X2 if split else _lib.P3D_CONV_MMA_F16
        if split and saturated is not None and (saturated.dtype != torch.int32 or saturated.numel() != 1 or saturated.device != dev_):
            raise RuntimeError("saturated must be an int32 [1] tensor on x's device (ops.conv_domain_flag)")
    with _on(dev_):
        key = (N, I, O, H, W, up)
        wsb = _WSB.get(key)
        if wsb is None:
            wsb = _WSB[key] = L.p3d_modconv2d_workspace_bytes(N, I, O, H, W, up)
        ws = _conv_scratch(dev_, wsb)
        a = _lib.ConvArgs(x.data_ptr() if x is not None else None, weight.data_ptr(), weight_f16.data_ptr() if weight_f16 is not None else None,
                          styles.data_ptr() if styles is not None else None, dcoef.data_ptr() if dcoef is not None else None,
                          noise.data_ptr() if noise is not None else None, bias.data_ptr() if bias is not None else None,
                          fir.data_ptr() if fir is not None else None, y.data_ptr() if y is not None else None, ws.data_ptr(),
                          saturated.data_ptr() if (saturated is not None and (mma == _lib.P3D_CONV_MMA_F16X2 or yimg is not None)) else None,
                          ximg.data.data_ptr() if ximg is not None else None, yimg.data.data_ptr() if yimg is not None else None,
                          next_styles.data_ptr() if yimg is not None else None,
                          rgb_weight.data_ptr() if rgb else None, rgb_styles.data_ptr() if rgb else None, rgbp.data_ptr() if rgb else None,
                          ws.numel(), N, I, H, W, O, kh, int(up), int(bool(demodulate)), nps, idx, mma, float(da), gain, clampv,
                          int(rgb_weight.shape[0]) if rgb else 0, int(getattr(weight_f16, "p3d_layout", 0)))
        _lib.check(L.p3d_modconv2d_ex_f32(C.byref(a), _stream()), "p3d_modconv2d_ex_f32")
    if rgb:
        return y, yimg, rgbp
    return (y, yimg) if both else (yimg if out_image else y)


# ======================================================================================================================
# Backward of the synthesis layers (include/p3d_synthesis_grad.h).  The autograd Functions sit inside the
# operators above: a call under autograd with an input that requires grad runs the same forward launches and records the
# HIP backward; every other call is unchanged.
def _wants_grad(*ts):
    return torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in ts)


def _sg_workspace(device, nbytes):
    return torch.empty((max(int(nbytes), 256),), dtype=torch.uint8, device=device)


def bias_act_backward(y, g_y, act, alpha, gain, clamp, dscale=None, want_noise=False):
    """p3d_bias_act_backward_f32: (g_z * dscale [N,C,...], sum over pixels of g_z [N,C], channel sum of g_z [N,pixels] or None)."""
    y, g_y = _chk(y, "y"), _chk(g_y, "g_y")
    N, Cc = y.shape[0], y.shape[1]
    HW = y.numel() // (N * Cc)
    out = torch.empty_like(y)
    gb = torch.empty((N, Cc), dtype=torch.float32, device=y.device)
    gn = torch.empty((N, HW), dtype=torch.float32, device=y.device) if want_noise else None
    if dscale is not None:
        dscale = _chk(dscale, "dscale")
    with _on(y.device):
        rc = _lib.lib().p3d_bias_act_backward_f32(_p(y), _p(g_y), N, Cc, HW, int(act), float(alpha), float(gain),
                                                  float(clamp if clamp is not None else -1), _p(dscale), _p(out), _p(gb), _p(gn), _stream())
    _lib.check(rc, "p3d_bias_act_backward_f32")
    return out, gb, gn


def conv_dgrad(g, wk, Co, Ho, Wo, stride, pad):
    """p3d_conv_dgrad_f32: g [N,Ci,Hi,Wi], wk [taps,Ci,Co] -> [N,Co,Ho,Wo]."""
    g, wk = _chk(g, "g"), _chk(wk, "wk")
    N, Ci, Hi, Wi = g.shape
    out = torch.empty((N, int(Co), int(Ho), int(Wo)), dtype=torch.float32, device=g.device)
    with _on(g.device):
        rc = _lib.lib().p3d_conv_dgrad_f32(_p(g), N, Ci, Hi, Wi, _p(wk), int(wk.shape[0]), int(Co), int(Ho), int(Wo), int(stride), int(pad),
                                           _p(out), _stream())
    _lib.check(rc, "p3d_conv_dgrad_f32")
    return out


def mod_backward(x, s, g):
    """p3d_mod_backward_f32: returns g_s [N,C] = sum over pixels of x * g and multiplies g (contiguous, written in place) by s."""
    x, s = _chk(x, "x"), _chk(s, "s")
    if not g.is_contiguous():
        raise RuntimeError("mod_backward: g is updated in place and must be contiguous")
    N, Cc = x.shape[0], x.shape[1]
    gs = torch.empty((N, Cc), dtype=torch.float32, device=x.device)
    with _on(x.device):
        rc = _lib.lib().p3d_mod_backward_f32(_p(x), _p(s), N, Cc, x.numel() // (N * Cc), _p(g), _p(gs), _stream())
    _lib.check(rc, "p3d_mod_backward_f32")
    return gs


def conv_wgrad(g, gmap, x, s, xmap, taps, domain, wk=None, dscale=None):
    """p3d_conv_wgrad_f32: g [N,O,Hg,Wg] with its index map gmap = (stride, tap step, pad), x [N,I,Hx,Wx] * s [N,I] with xmap, over the
    pixel domain (Hd, Wd) -> (dw [taps,O,I], g_d [N,O] when wk [taps,O,I] and dscale [N,O] are given, else None)."""
    g, x = _chk(g, "g"), _chk(x, "x")
    N, O, Hg, Wg = g.shape
    I, Hx, Wx = x.shape[1], x.shape[2], x.shape[3]
    Hd, Wd = domain
    s = _chk(s, "s") if s is not None else None
    L = _lib.lib()
    wsb = L.p3d_conv_wgrad_workspace_bytes(N, O, I, int(taps), int(Hd), int(Wd))
    if wsb == 0:
        raise RuntimeError("conv_wgrad: sizes out of range")
    ws = _sg_workspace(g.device, wsb)
    dw = torch.empty((int(taps), O, I), dtype=torch.float32, device=g.device)
    gd = None
    if wk is not None:
        wk, dscale = _chk(wk, "wk"), _chk(dscale, "dscale")
        gd = torch.empty((N, O), dtype=torch.float32, device=g.device)
    with _on(g.device):
        rc = L.p3d_conv_wgrad_f32(_p(g), Hg, Wg, *(int(v) for v in gmap), _p(x), _p(s), Hx, Wx, *(int(v) for v in xmap), N, O, I, int(taps),
                                  int(Hd), int(Wd), _p(dw), _p(wk), _p(dscale), _p(gd), _p(ws), ws.numel(), _stream())
    _lib.check(rc, "p3d_conv_wgrad_f32")
    return dw, gd


def _upfirdn2d_adjoint(g, f, up, down, padding, flip_filter, gain, in_hw, op=None):
    """The adjoint of upfirdn2d(x [.., in_hw], f, up, down, padding, flip_filter, gain) applied to g (upfirdn2d.py:236-245); op: the
    operator to call in upfirdn2d's place (ops.fir when the call is to be recorded)."""
    px0, px1, py0, py1 = _parse_padding(padding)
    fh, fw = f.shape
    ih, iw = in_hw
    oh, ow = g.shape[-2:]
    p = [fw - px0 - 1, iw * up - ow * down + px0 - up + 1, fh - py0 - 1, ih * up - oh * down + py0 - up + 1]
    return (op or upfirdn2d)(g.contiguous(), f, up=down, down=up, padding=p, flip_filter=not flip_filter, gain=gain)


class _Upsample2dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, meta):
        f, up, padding, flip_filter, gain = meta
        ctx.meta, ctx.hw = meta, tuple(x.shape[-2:])
        return _upsample2d_impl(x, f, up, padding, flip_filter, gain)

    @staticmethod
    def backward(ctx, gy):
        f, up, padding, flip_filter, gain = ctx.meta
        px0, px1, py0, py1 = _parse_padding(padding)
        fh, fw = f.shape
        p = [px0 + (fw + up - 1) // 2, px1 + (fw - up) // 2, py0 + (fh + up - 1) // 2, py1 + (fh - up) // 2]
        return _upfirdn2d_adjoint(gy, f, up, 1, p, flip_filter, gain * up * up, ctx.hw), None


class _TorgbWeightsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, weight):
        ctx.shape = tuple(weight.shape)
        return _torgb_weights_impl(weight)

    @staticmethod
    def backward(ctx, gwt):
        O, I = ctx.shape[0], ctx.shape[1]
        return gwt[:, :O].t().reshape(ctx.shape).contiguous()


class _TorgbFn(torch.autograd.Function):
    """ToRGB (+ skip) backward: the clamp mask from the recomputed pre-clamp sums (the forward writes only the image), the skip
    image's adjoint on upfirdn2d (down 2, flipped filter), data and weight gradients on the matrix cores."""

    @staticmethod
    def forward(ctx, x, weight_t, styles, bias, skip, meta):
        O, clamp, skip_filter = meta
        ctx.meta = meta
        ctx.save_for_backward(x, weight_t, styles, bias)
        ctx.skip_hw = None if skip is None else tuple(skip.shape[-2:])
        return _torgb_impl(x, weight_t, O, styles, bias, clamp, skip, skip_filter)

    @staticmethod
    def backward(ctx, gimg):
        x, weight_t, styles, bias = ctx.saved_tensors
        O, clamp, skip_filter = ctx.meta
        x, styles, g = x.contiguous(), styles.contiguous(), gimg.contiguous()
        N, I, H, W = x.shape
        g_skip = None
        if ctx.skip_hw is not None and ctx.needs_input_grad[4]:
            g_skip = _upfirdn2d_adjoint(g, skip_filter, 2, 1, [2, 1, 2, 1], False, 4.0, ctx.skip_hw)
        ylin = _torgb_impl(x, weight_t, O, styles, bias, None, None, None) if clamp is not None else g
        gz, gb, _ = bias_act_backward(ylin, g, 0, 0.0, 1.0, clamp)
        w = weight_t[:, :O].t().contiguous().view(1, O, I)
        gx = conv_dgrad(gz, w, I, H, W, 1, 0)
        gs = mod_backward(x, styles, gx)
        dw, _ = conv_wgrad(gz, (1, 0, 0), x, styles, (1, 0, 0), 1, (H, W))
        gwt = torch.zeros_like(weight_t)
        gwt[:, :O] = dw[0].t()
        return gx, gwt, gs, (gb.sum(0) if bias is not None else None), g_skip, None


class _ModConvFn(torch.autograd.Function):
    """SynthesisLayer backward: bias_act from the output y (g_z * d), the FIR adjoint of an up-sampling layer,
    the data gradient (plain: flipped weights, stride 1; up: stride-2 correlation), the modulation (g_s, g_x = g_xs * s), the
    weight gradient split over pixels, and g_d[n,o] = sum W * dW_n / d."""

    @staticmethod
    def forward(ctx, x, weight, styles, dcoef, bias, noise, kw):
        k = dict(kw)
        ride = k.pop("ride", None)
        if k["demodulate"] and dcoef is None:
            raise RuntimeError("modulated_conv2d under autograd: pass the demodulation coefficients (dcoef)")
        if ride is not None:  # (the block's ToRGB rides on this launch: x staged as the layer's activation image, y written, the shares out)
            y, _, part = _modulated_conv2d_impl(act_to_image(x, styles, saturated=k["saturated"]), weight, styles, noise=noise, up=k["up"],
                                                padding=k["padding"], resample_filter=k["resample_filter"], demodulate=k["demodulate"], bias=bias,
                                                act=k["act"], gain=k["gain"], clamp=k["clamp"], weight_f16=k["weight_f16"], dcoef=dcoef,
                                                saturated=k["saturated"], rgb_weight=ride[0], rgb_styles=ride[1], want_y=True)
            ctx.mark_non_differentiable(part)
        else:
            y = _modulated_conv2d_impl(x, weight, styles, noise=noise, up=k["up"], padding=k["padding"], resample_filter=k["resample_filter"],
                                       demodulate=k["demodulate"], bias=bias, act=k["act"], gain=k["gain"], clamp=k["clamp"],
                                       weight_f16=k["weight_f16"], dcoef=dcoef, saturated=k["saturated"])
        ctx.kw = k
        ctx.noise_shape = None if noise is None else tuple(noise.shape)
        ctx.save_for_backward(x, weight, styles, dcoef, bias, y)
        return (y, part) if ride is not None else y

    @staticmethod
    def backward(ctx, gy, *_):
        x, weight, styles, dcoef, bias, y = ctx.saved_tensors
        k = ctx.kw
        if gy is None:
            gy = torch.zeros_like(y)
        x, styles = x.contiguous(), styles.contiguous()
        N, I, H, W = x.shape
        O, ks = weight.shape[0], weight.shape[-1]
        up, taps = k["up"], weight.shape[-1] * weight.shape[-2]
        idx, da, dg = _ACTS[k["act"]]
        gain = float(k["gain"] if k["gain"] is not None else dg)
        d = dcoef.reshape(N, O).contiguous() if k["demodulate"] else None
        want_noise = ctx.noise_shape is not None and ctx.needs_input_grad[5]
        gz, gb, gn = bias_act_backward(y, gy.contiguous(), idx, da, gain, k["clamp"], dscale=d, want_noise=want_noise)
        wk = weight.detach().permute(2, 3, 0, 1).reshape(taps, O, I).contiguous()  # [tap][o][i]
        if up == 2:
            G = _upfirdn2d_adjoint(gz, k["resample_filter"], 1, 1, 1, False, 4.0, (2 * H + 1, 2 * W + 1))  # [N,O,2H+1,2W+1]
            gx = conv_dgrad(G, wk, I, H, W, 2, 0)
            gmap, xmap = (2, 1, 0), (1, 0, 0)
        elif ks == 3:
            G = gz
            gx = conv_dgrad(G, wk.flip(0).contiguous(), I, H, W, 1, 1)
            gmap, xmap = (1, 0, 0), (1, 1, 1)
        else:
            G = gz
            gx = conv_dgrad(G, wk, I, H, W, 1, 0)
            gmap, xmap = (1, 0, 0), (1, 0, 0)
        gs = mod_backward(x, styles, gx)
        dw, gd = conv_wgrad(G, gmap, x, styles, xmap, taps, (H, W), wk=wk if d is not None else None, dscale=d)
        gw = dw.view(ks, ks, O, I).permute(2, 3, 0, 1).contiguous()
        g_noise = None
        if want_noise:
            ns = ctx.noise_shape  # one of the forward's three shapes: per sample only as [N,1,H,W] with N > 1
            g_noise = (gn if len(ns) == 4 and ns[0] == N and N > 1 else gn.sum(0)).reshape(ns)
        return (gx, gw, gs, (gd.view_as(dcoef) if gd is not None else None), (gb.sum(0) if bias is not None else None), g_noise, None)


class _TorgbCombineFn(torch.autograd.Function):
    """Backward of a ToRGB layer that rode on its conv1 launch (super-resolution): the clamp mask, the bias gradient and
    the skip image's adjoint from the forward's own shares (p3d_torgb_combine_backward_f32 — the stand-alone ToRGB kernel would sum the
    channels in another order, and a mask from other bits is a wrong gradient at the clamp edge); data, style and weight gradients
    against conv1's fp32 result on the same kernels as _TorgbFn (one tap)."""

    @staticmethod
    def forward(ctx, x, weight, styles, bias, skip, partial, meta):
        clamp, skip_filter = meta
        ctx.meta, ctx.has_skip = meta, skip is not None
        ctx.save_for_backward(x, weight, styles, bias, partial)
        return _torgb_combine_impl(partial, bias, clamp, skip, skip_filter)

    @staticmethod
    def backward(ctx, gimg):
        x, weight, styles, bias, partial = ctx.saved_tensors
        clamp, skip_filter = ctx.meta
        want_skip = ctx.has_skip and ctx.needs_input_grad[4]
        gz, gb, g_skip = torgb_combine_backward(partial, gimg.contiguous(), bias, clamp, skip_filter if want_skip else None,
                                                want_bias=bias is not None)
        x, styles = x.contiguous(), styles.contiguous()
        N, I, H, W = x.shape
        O = weight.shape[0]
        gx = conv_dgrad(gz, weight.detach().reshape(1, O, I).contiguous(), I, H, W, 1, 0)
        gs = mod_backward(x, styles, gx)
        dw, _ = conv_wgrad(gz, (1, 0, 0), x, styles, (1, 0, 0), 1, (H, W))
        return gx, dw.view(weight.shape), gs, gb, g_skip, None, None


# ======================================================================================================================
# The dual discriminator's operators (include/p3d_discriminator.h)
# ======================================================================================================================
def _conv2d_act_impl(x, wk, bias, act, gain, clamp, stride, pad, res, want_pre=False):
    x, wk = _chk(x, "x"), _chk(wk, "wk")
    if x.ndim != 4 or wk.ndim != 3 or wk.shape[1] != x.shape[1] or wk.shape[0] not in (1, 9):
        raise RuntimeError("conv2d_act: x [N,Ci,H,W] and wk [taps (1 or 9),Ci,Co]")
    if act not in _ACTS:
        raise NotImplementedError(f"activation {act!r} is not used by the PAniC-3D discriminator")
    idx, alpha, dg = _ACTS[act]
    N, Ci, Hi, Wi = x.shape
    taps, _, Co = wk.shape
    k = 3 if taps == 9 else 1
    Ho, Wo = (Hi + 2 * pad - k) // stride + 1, (Wi + 2 * pad - k) // stride + 1
    if Ho <= 0 or Wo <= 0:
        raise RuntimeError("conv2d_act: the input is smaller than the kernel")
    if bias is not None:
        bias = _chk(bias, "bias")
        if tuple(bias.shape) != (Co,):
            raise RuntimeError("conv2d_act: bias must be [Co]")
    if res is not None:
        res = _chk(res, "res")
        if tuple(res.shape) != (N, Co, Ho, Wo):
            raise RuntimeError("conv2d_act: res must have the output's shape")
    out = torch.empty((N, Co, Ho, Wo), dtype=torch.float32, device=x.device)
    pre = torch.empty_like(out) if want_pre else None
    with _on(x.device):
        rc = _lib.lib().p3d_conv2d_act_f32(_p(x), N, Ci, Hi, Wi, _p(wk), taps, Co, Ho, Wo, int(stride), int(pad), _p(bias), idx, float(alpha),
                                           float(gain if gain is not None else dg), float(clamp if clamp is not None else -1), _p(res),
                                           _p(pre), _p(out), _stream())
    _lib.check(rc, "p3d_conv2d_act_f32")
    return (out, pre) if want_pre else out


def conv2d_act(x, wk, bias=None, act="linear", gain=None, clamp=None, stride=1, pad=0, res=None, r1=False):
    """Conv2dLayer's forward after any resampling, in one launch: clamp(act(corr(x, wk) + bias) * gain) (+ res).  x [N,Ci,H,W];
    wk [taps,Ci,Co] = the layer's weight * weight_gain as weight.permute(2, 3, 1, 0); gain None = the activation's default.
    A plain call under no_grad; records the HIP backward when an input requires grad — same forward bits.  That backward is first order
    only unless r1 is set (DualDiscriminator.set_r1_grad): then a backward that autograd records (create_graph=True) is itself
    differentiable once more (the R1 penalty), and a plain backward is unchanged."""
    if _wants_grad(x, wk, bias, res):
        return _Conv2dActFn.apply(x, wk, bias, res, (act, gain, clamp, int(stride), int(pad)), bool(r1))
    return _conv2d_act_impl(x, wk, bias, act, gain, clamp, int(stride), int(pad), res)


R1_MESSAGE = ("the discriminator's HIP backward is first order only: the R1 penalty (r1_gamma > 0, the Dreg / Dboth phases) needs its "
              "double backward, which is not implemented")


def _first_order(backward):
    """once_differentiable, with the failure moved to where it is understood: a backward that autograd itself records
    (create_graph=True — the R1 penalty's torch.autograd.grad) raises at once instead of returning a graph that cannot be used."""
    inner = torch.autograd.function.once_differentiable(backward)

    def wrapper(ctx, *grads):
        if torch.is_grad_enabled():
            raise RuntimeError(R1_MESSAGE)
        return inner(ctx, *grads)
    return wrapper


R1_THIRD_ORDER_MESSAGE = ("the discriminator's recorded HIP backward (set_r1_grad) is second order only: the backward of the R1 penalty "
                          "cannot itself be recorded (create_graph=True); a third differentiation is not implemented")
_NO_WEIGHT_GRADIENTS = [False]


def _second_order(backward):
    """_first_order for the Functions of the recorded backward, which are themselves first order: a third differentiation raises."""
    inner = torch.autograd.function.once_differentiable(backward)

    def wrapper(ctx, *grads):
        if torch.is_grad_enabled():
            raise RuntimeError(R1_THIRD_ORDER_MESSAGE)
        return inner(ctx, *grads)
    return wrapper


class no_weight_gradients:
    """The reference's conv2d_gradfix.no_weight_gradients(): inside it, a recorded backward (r1) of the discriminator's convolution
    layers computes input gradients only.  ctx.needs_input_grad is fixed when the forward runs, so torch.autograd.grad(...,
    only_inputs=True) alone would still have every layer compute a weight and a bias gradient that nobody reads."""

    def __enter__(self):
        self.old, _NO_WEIGHT_GRADIENTS[0] = _NO_WEIGHT_GRADIENTS[0], True
        return self

    def __exit__(self, *exc):
        _NO_WEIGHT_GRADIENTS[0] = self.old


def _bias_act_backward_meta(pre, gy, meta):
    act, gain, clamp = meta[:3]
    idx, alpha, dg = _ACTS[act]
    gz, gb, _ = bias_act_backward(pre, gy, idx, alpha, float(gain if gain is not None else dg), clamp)
    return gz, gb


_ONE_TAP = {}


def _one_tap(device):
    f = _ONE_TAP.get(device)
    if f is None:
        f = _ONE_TAP[device] = torch.ones((1, 1), dtype=torch.float32, device=device)
    return f


def _conv_input_grad(gz, wk, in_shape, stride, pad):
    """The data gradient of one convolution layer from g_z (the cotangent after bias_act's backward): p3d_conv_dgrad_f32 with the
    flipped, transposed weights, a stride-2 layer's g_z zero-interleaved first."""
    _, Ci, Hi, Wi = in_shape
    k = 3 if wk.shape[0] == 9 else 1
    if k - 1 - pad < 0:
        raise NotImplementedError("conv2d_act backward: pad > kernel_size - 1")
    # gx[y] = sum_t gz[(y + pad - t) / stride] w[t] = sum_t' Z[y + t' - (k - 1 - pad)] w[k - 1 - t'], Z = gz with stride - 1 zeros
    # between its values (positions past Z's end read 0, as Z's own continuation would)
    Z = gz if stride == 1 else upfirdn2d(gz, _one_tap(gz.device), up=stride)
    return conv_dgrad(Z, wk.detach().flip(0).transpose(1, 2).contiguous(), Ci, Hi, Wi, 1, k - 1 - pad)


def _conv_weight_grad(gz, x, taps, stride, pad):
    """The gradient of wk [taps,Ci,Co] of one convolution layer from g_z and the layer's input (or, in the R1 pass, the cotangent of
    the input's gradient, which takes the input's place): p3d_conv_wgrad_f32 over the output's pixels."""
    dw, _ = conv_wgrad(gz, (1, 0, 0), x.contiguous(), None, (stride, 1 if taps == 9 else 0, pad), taps, tuple(gz.shape[-2:]))  # [taps,Co,Ci]
    return dw.transpose(1, 2).contiguous()


class _Conv2dActFn(torch.autograd.Function):
    """Backward of one discriminator convolution layer: bias_act from the output before the residual, the data
    gradient on p3d_conv_dgrad_f32 (flipped, transposed weights; a stride-2 layer's cotangent zero-interleaved first: the adjoint
    of a stride-2 correlation is a stride-1 correlation over it), the weight gradient split over the output's pixels.  With r1 set, a
    backward that autograd records goes through _R1ConvFn: the same launches, differentiable once more."""

    @staticmethod
    def forward(ctx, x, wk, bias, res, meta, r1=False):
        act, gain, clamp, stride, pad = meta
        if res is not None:
            y, pre = _conv2d_act_impl(x, wk, bias, act, gain, clamp, stride, pad, res, want_pre=True)
        else:
            y = pre = _conv2d_act_impl(x, wk, bias, act, gain, clamp, stride, pad, None)
        ctx.meta, ctx.r1 = meta, r1
        ctx.save_for_backward(x, wk, pre, *([bias] if r1 and bias is not None else []))
        return y

    @staticmethod
    def backward(ctx, gy):
        if ctx.r1 and torch.is_grad_enabled():
            return _Conv2dActFn._recorded(ctx, gy)
        return _Conv2dActFn._plain(ctx, gy)

    @staticmethod
    def _recorded(ctx, gy):
        x, wk, pre = ctx.saved_tensors[:3]
        bias = ctx.saved_tensors[3] if len(ctx.saved_tensors) > 3 else None
        _, _, _, stride, pad = ctx.meta
        pre, gy = pre.detach(), gy.contiguous()
        need = ctx.needs_input_grad
        gx = _R1ConvFn.apply(gy, wk, bias, pre, ctx.meta, tuple(x.shape)) if need[0] else None
        gwk = g_bias = None
        if (need[1] or need[2]) and not _NO_WEIGHT_GRADIENTS[0]:
            # the parameters' own first-order gradients, asked for in a recorded pass: today's values, as constants of the graph
            with torch.no_grad():
                gz, gb = _bias_act_backward_meta(pre, gy.detach(), ctx.meta)
                gwk = _conv_weight_grad(gz, x.detach(), wk.shape[0], stride, pad) if need[1] else None
                g_bias = gb.sum(0) if need[2] else None
        return gx, gwk, g_bias, (gy if need[3] else None), None, None

    @staticmethod
    @_first_order
    def _plain(ctx, gy):
        x, wk, pre = ctx.saved_tensors[:3]
        _, _, _, stride, pad = ctx.meta
        gy = gy.contiguous()
        gz, gb = _bias_act_backward_meta(pre, gy, ctx.meta)
        gx = _conv_input_grad(gz, wk, x.shape, stride, pad) if ctx.needs_input_grad[0] else None
        gwk = _conv_weight_grad(gz, x, wk.shape[0], stride, pad) if ctx.needs_input_grad[1] else None
        g_bias = gb.sum(0) if ctx.needs_input_grad[2] else None
        return gx, gwk, g_bias, (gy if ctx.needs_input_grad[3] else None), None, None


class _UpfirdnFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, meta, r1=False):
        ctx.meta, ctx.hw, ctx.r1 = meta, tuple(x.shape[-2:]), r1
        return upfirdn2d(x, *meta)

    @staticmethod
    def backward(ctx, gy):
        if ctx.r1 and torch.is_grad_enabled():
            # linear: the adjoint, called through fir again, is recorded in turn and its own backward is the operator itself (as _BlurFn)
            f, up, down, padding, flip_filter, gain = ctx.meta
            return _upfirdn2d_adjoint(gy, f, up, down, padding, flip_filter, gain, ctx.hw, op=lambda *a, **k: fir(*a, r1=True, **k)), None, None
        return _UpfirdnFn._plain(ctx, gy)

    @staticmethod
    @_first_order
    def _plain(ctx, gy):
        f, up, down, padding, flip_filter, gain = ctx.meta
        return _upfirdn2d_adjoint(gy, f, up, down, padding, flip_filter, gain, ctx.hw), None, None


def fir(x, f, up=1, down=1, padding=0, flip_filter=False, gain=1, r1=False):
    """upfirdn2d for the discriminator: the plain call under no_grad, differentiable in x (the adjoint is upfirdn2d with up and down
    exchanged and the flipped filter, _upfirdn2d_adjoint) when x requires grad: first order only, or with r1 to any order."""
    if _wants_grad(x):
        return _UpfirdnFn.apply(x, (f, up, down, padding, flip_filter, gain), bool(r1))
    return upfirdn2d(x, f, up, down, padding, flip_filter, gain)


def _mbstd_impl(x, group, F):
    x = _chk(x, "x")
    N, Cc, H, W = x.shape
    G = N if group is None else min(int(group), N)
    if N % G != 0 or Cc % F != 0:
        raise RuntimeError("minibatch_std: the group size must divide the batch and num_channels the channels")
    y = torch.empty((N, Cc + F, H, W), dtype=torch.float32, device=x.device)
    sd = torch.empty((N // G, Cc, H, W), dtype=torch.float32, device=x.device)
    with _on(x.device):
        rc = _lib.lib().p3d_mbstd_f32(_p(x), N, Cc, H * W, G, int(F), 1, _p(y), _p(sd), _stream())
    _lib.check(rc, "p3d_mbstd_f32")
    return y, sd, G


def minibatch_std(x, group_size, num_channels=1, r1=False):
    """MinibatchStdLayer.forward (networks_stylegan2.py:854-869): x [N,C,H,W] -> [N,C+F,H,W].  Plain under no_grad, an autograd function
    when x requires grad — same forward bits; first order, or with r1 second order in a backward that autograd records."""
    if _wants_grad(x):
        return _MbStdFn.apply(x, group_size, int(num_channels), bool(r1))
    return _mbstd_impl(x, group_size, int(num_channels))[0]


def mbstd_backward(x, sd, gy, G, F):
    """p3d_mbstd_backward_f32: the statistic channels' contribution to the gradient of x [N,C,H,W]; gy [N,C+F,H,W] is the cotangent of
    the concatenated tensor (its last F channels are read in place), sd the forward's deviation map."""
    x, sd, gy = _chk(x, "x"), _chk(sd, "sd"), _chk(gy, "gy")
    N, Cc, H, W = x.shape
    gx = torch.empty_like(x)
    with _on(x.device):
        rc = _lib.lib().p3d_mbstd_backward_f32(_p(x), _p(sd), C.c_void_p(gy.data_ptr() + 4 * Cc * H * W), (Cc + F) * H * W, N, Cc, H * W,
                                               int(G), int(F), _p(gx), _stream())
    _lib.check(rc, "p3d_mbstd_backward_f32")
    return gx


class _MbStdFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, group, F, r1=False):
        y, sd, G = _mbstd_impl(x, group, F)
        ctx.save_for_backward(x, sd)
        ctx.G, ctx.F, ctx.r1 = G, F, r1
        return y

    @staticmethod
    def backward(ctx, gy):
        if ctx.r1 and torch.is_grad_enabled():
            x, sd = ctx.saved_tensors  # x is the graph's own tensor: the second-order gradient flows on into the layers below
            gy = gy.contiguous()
            return _R1MbStdFn.apply(gy, x, sd, ctx.G, ctx.F) + gy[:, :x.shape[1]], None, None, None
        return _MbStdFn._plain(ctx, gy)

    @staticmethod
    @_first_order
    def _plain(ctx, gy):
        x, sd = ctx.saved_tensors
        gy = gy.contiguous()
        return mbstd_backward(x, sd, gy, ctx.G, ctx.F).add_(gy[:, :x.shape[1]]), None, None, None


# ======================================================================================================================
# The R1 penalty: the recorded first backward of the discriminator's layers, closed under one more differentiation
# (include/p3d_r1.h)
# ======================================================================================================================
def _conv2d_mask_impl(h, wk, pre, act, gain, clamp, stride, pad):
    """p3d_conv2d_mask_f32: the tangent layer m(pre) * corr(h, wk; stride, pad) in one launch, m the mask-and-gain rule of
    bias_act_backward.  h [N,Ci,Hi,Wi], wk [taps,Ci,Co], pre [N,Co,Ho,Wo]."""
    h, wk, pre = _chk(h, "h"), _chk(wk, "wk"), _chk(pre, "pre")
    idx, alpha, dg = _ACTS[act]
    N, Ci, Hi, Wi = h.shape
    taps, _, Co = wk.shape
    if wk.shape[1] != Ci or tuple(pre.shape[:2]) != (N, Co):
        raise RuntimeError("conv2d_mask: h [N,Ci,H,W], wk [taps,Ci,Co] and pre [N,Co,Ho,Wo]")
    out = torch.empty_like(pre)
    with _on(h.device):
        rc = _lib.lib().p3d_conv2d_mask_f32(_p(h), N, Ci, Hi, Wi, _p(wk), taps, Co, pre.shape[2], pre.shape[3], int(stride), int(pad), _p(pre),
                                            idx, float(alpha), float(gain if gain is not None else dg), float(clamp if clamp is not None else -1),
                                            _p(out), _stream())
    _lib.check(rc, "p3d_conv2d_mask_f32")
    return out


def mbstd_backward2(x, gy, h, G, F):
    """p3d_mbstd_backward2_f32, the backward of mbstd_backward: x, h [N,C,H,W] (h the cotangent of mbstd_backward's result), gy
    [N,C+F,H,W] the concatenated cotangent it was called with -> (the gradient of gy's F statistic channels [N,F,H,W], of x [N,C,H,W])."""
    x, gy, h = _chk(x, "x"), _chk(gy, "gy"), _chk(h, "h")
    N, Cc, H, W = x.shape
    g_extra = torch.empty((N, F, H, W), dtype=torch.float32, device=x.device)
    gx = torch.empty_like(x)
    with _on(x.device):
        rc = _lib.lib().p3d_mbstd_backward2_f32(_p(x), C.c_void_p(gy.data_ptr() + 4 * Cc * H * W), (Cc + F) * H * W, _p(h), N, Cc, H * W,
                                                int(G), int(F), _p(g_extra), _p(gx), _stream())
    _lib.check(rc, "p3d_mbstd_backward2_f32")
    return g_extra, gx


def _r1_sumsq_impl(a, b):
    a = _chk(a, "g_image")
    N = a.shape[0]
    b = _chk(b, "g_raw") if b is not None else None
    if a.ndim < 2 or a.numel() == 0 or (b is not None and (b.shape[0] != N or b.numel() == 0)):
        raise RuntimeError("r1_penalty: g_image [N,...] and g_raw [N,...] or None, not empty")
    out = torch.empty((N,), dtype=torch.float32, device=a.device)
    with _on(a.device):
        rc = _lib.lib().p3d_r1_sumsq_f32(_p(a), a.numel() // N, _p(b), b.numel() // N if b is not None else 0, N, _p(out), _stream())
    _lib.check(rc, "p3d_r1_sumsq_f32")
    return out


class _R1ConvFn(torch.autograd.Function):
    """The input gradient of one convolution layer as a function of (g_y, wk, bias), pre a constant: forward = the three steps of
    _Conv2dActFn's plain backward (the same bits).  Backward, for the cotangent h of g_x: towards g_y the tangent layer (one launch),
    towards wk the weight gradient with h in the input's place, towards the bias zeros (the mask's derivative is zero almost
    everywhere; the reference's bias_act gives the same zeros, and Adam counts a zero gradient where it skips a missing one)."""

    @staticmethod
    def forward(ctx, gy, wk, bias, pre, meta, in_shape):
        _, _, _, stride, pad = meta
        gz, _ = _bias_act_backward_meta(pre, gy, meta)
        ctx.meta, ctx.has_bias = meta, bias is not None
        ctx.save_for_backward(gz, wk, pre)
        return _conv_input_grad(gz, wk, in_shape, stride, pad)

    @staticmethod
    @_second_order
    def backward(ctx, h):
        gz, wk, pre = ctx.saved_tensors
        act, gain, clamp, stride, pad = ctx.meta
        h = h.contiguous()
        g_gy = _conv2d_mask_impl(h, wk, pre, act, gain, clamp, stride, pad) if ctx.needs_input_grad[0] else None
        g_wk = _conv_weight_grad(gz, h, wk.shape[0], stride, pad) if ctx.needs_input_grad[1] else None
        g_b = torch.zeros((wk.shape[2],), dtype=h.dtype, device=h.device) if ctx.has_bias and ctx.needs_input_grad[2] else None
        return g_gy, g_wk, g_b, None, None, None


class _R1MaskFn(torch.autograd.Function):
    """bias_act's backward g -> g_z as a function of (g, bias) with the output y a constant (a fully-connected layer with an
    activation in the recorded pass): diagonal, so its own backward is the same launch on the cotangent; zeros towards the bias."""

    @staticmethod
    def forward(ctx, g, bias, y, meta):
        ctx.meta, ctx.has_bias = meta, bias is not None
        ctx.save_for_backward(y)
        return _bias_act_backward_meta(y, g.contiguous(), meta)[0]

    @staticmethod
    @_second_order
    def backward(ctx, h):
        y, = ctx.saved_tensors
        g_g = _bias_act_backward_meta(y, h.contiguous(), ctx.meta)[0] if ctx.needs_input_grad[0] else None
        g_b = torch.zeros((y.shape[1],), dtype=h.dtype, device=h.device) if ctx.has_bias and ctx.needs_input_grad[1] else None
        return g_g, g_b, None, None


class _R1MbStdFn(torch.autograd.Function):
    """mbstd_backward as a function of (gy, x), the deviation map a constant; its backward is p3d_mbstd_backward2_f32."""

    @staticmethod
    def forward(ctx, gy, x, sd, G, F):
        ctx.G, ctx.F = G, F
        ctx.save_for_backward(gy, x)
        return mbstd_backward(x, sd, gy, G, F)

    @staticmethod
    @_second_order
    def backward(ctx, h):
        gy, x = ctx.saved_tensors
        g_extra, gx = mbstd_backward2(x, gy, h.contiguous(), ctx.G, ctx.F)
        g_gy = torch.cat([torch.zeros_like(x), g_extra], dim=1) if ctx.needs_input_grad[0] else None
        return g_gy, (gx if ctx.needs_input_grad[1] else None), None, None, None


class _R1PenaltyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, g_image, g_raw):
        ctx.save_for_backward(g_image, g_raw)
        return _r1_sumsq_impl(g_image, g_raw)

    @staticmethod
    def backward(ctx, cot):
        g_image, g_raw = ctx.saved_tensors
        scale = lambda g: (2 * cot).reshape(-1, *([1] * (g.ndim - 1))) * g
        return scale(g_image), (scale(g_raw) if g_raw is not None else None)


def r1_penalty(g_image, g_raw=None):
    """The R1 penalty of loss_orthocondA.py:727 / :732 per sample: sum g_image^2 (+ sum g_raw^2) over everything but the batch axis, in
    one launch of p3d_r1_sumsq_f32; its gradient is 2 * cotangent[n] * g."""
    if _wants_grad(g_image, g_raw):
        return _R1PenaltyFn.apply(g_image, g_raw)
    return _r1_sumsq_impl(g_image, g_raw)


# ======================================================================================================================
# The training loss's operators (include/p3d_loss.h)
# ======================================================================================================================
BLUR_TILE = (32, 64)  # csrc/p3d_loss.hip: the blur's tile (rows, columns) up to 69 taps; 16 rows above


def gaussian_filter(sigma, device=None):
    """The 1-D filter of the loss's blur, built as loss_orthocondA.py:186 builds it: 2^-((i / sigma)^2) for i = -R .. R, R = floor(3 sigma),
    normalised to sum 1; None for R = 0."""
    R = np.floor(sigma * 3)
    if R <= 0:
        return None
    f = torch.arange(-R, R + 1, device=device).div(sigma).square().neg().exp2()
    return f / f.sum()


def _blur_impl(x, f):
    x, f = _chk(x, "x"), _chk(f, "f")
    if x.ndim < 2 or f.ndim != 1:
        raise RuntimeError("blur_fir: x [..., H, W] and a 1-D filter")
    H, W = x.shape[-2:]
    y = torch.empty_like(x)
    if x.numel() == 0:
        return y
    with _on(x.device):
        rc = _lib.lib().p3d_blur_f32(_p(x), x.numel() // (H * W), H, W, _p(f), f.numel(), _p(y), _stream())
    _lib.check(rc, "p3d_blur_f32")
    return y


class _BlurFn(torch.autograd.Function):
    """The blur is linear: its backward is the same operator with the flipped filter, called through blur_fir again, so the backward is
    itself recorded when autograd asks for it (create_graph=True) and the operator is differentiable to any order."""

    @staticmethod
    def forward(ctx, x, f):
        ctx.f = f
        return _blur_impl(x, f)

    @staticmethod
    def backward(ctx, gy):
        return blur_fir(gy, ctx.f.flip(0)), None


def blur_fir(x, f):
    """p3d_blur_f32: the separable 'same'-size correlation of x [..., H, W] with the 1-D filter f (odd, at most 127 taps) along both axes,
    zero boundary.  A plain call under no_grad; differentiable in x to any order under autograd — same forward bits."""
    if _wants_grad(x):
        return _BlurFn.apply(x, f.detach())
    return _blur_impl(x, f)


def blur(x, sigma):
    """The Gaussian blur of run_D and of the raw target (loss_orthocondA.py:182-187, :222-226): upfirdn2d.filter2d(x, f / f.sum()) with the
    filter of gaussian_filter(sigma); x itself when floor(3 sigma) == 0."""
    f = gaussian_filter(sigma, x.device)
    return x if f is None else blur_fir(x, f)


def _l1_impl(a, b, scale, want_grad):
    a, b = _chk(a, "a"), _chk(b, "b")
    if a.shape != b.shape or a.numel() == 0:
        raise RuntimeError("l1_mean: a and b must have the same, non-empty shape")
    n = a.numel()
    L = _lib.lib()
    ws = _sg_workspace(a.device, L.p3d_l1_workspace_bytes(n))
    out = torch.empty((1,), dtype=torch.float32, device=a.device)
    ga = torch.empty_like(a) if want_grad else None
    with _on(a.device):
        rc = L.p3d_l1_f32(_p(a), _p(b), n, float(scale), _p(out), _p(ga), _p(ws), ws.numel(), _stream())
    _lib.check(rc, "p3d_l1_f32")
    return out[0] / n, ga


class _L1MeanFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        y, ga = _l1_impl(a, b, 1.0 / a.numel(), True)
        ctx.save_for_backward(ga)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        ga, = ctx.saved_tensors
        ga = ga * g
        return (ga if ctx.needs_input_grad[0] else None), (-ga if ctx.needs_input_grad[1] else None)


def l1_mean(a, b):
    """(a - b).abs().mean() on p3d_l1_f32.  Under autograd the gradient sign(a - b) / n (sign(0) = 0) is written by the forward launch
    and multiplied by the incoming cotangent in backward."""
    if _wants_grad(a, b):
        return _L1MeanFn.apply(a, b)
    return _l1_impl(a, b, 0.0, False)[0]


DEPTH_MODES = {"z": _lib.P3D_DEPTH_Z, "x": _lib.P3D_DEPTH_X, "norm": _lib.P3D_DEPTH_NORM}


def _view_terms_impl(weights, xyz, gt_alpha, gt_xyz, depth_mode, q, want_grad):
    weights, xyz, gt_alpha, gt_xyz = _chk(weights, "weights"), _chk(xyz, "xyz"), _chk(gt_alpha, "gt_alpha"), _chk(gt_xyz, "gt_xyz")
    if depth_mode not in DEPTH_MODES:
        raise RuntimeError(f"view_terms: depth_mode must be one of {sorted(DEPTH_MODES)}")
    N, r, S = weights.shape[0], weights.shape[-1], gt_alpha.shape[-1]
    if tuple(weights.shape) != (N, 1, r, r) or tuple(xyz.shape) != (N, 3, r, r) or tuple(gt_alpha.shape) != (N, 1, S, S) \
            or tuple(gt_xyz.shape) != (N, 3, S, S):
        raise RuntimeError("view_terms: weights [N,1,r,r], xyz [N,3,r,r], gt_alpha [N,1,S,S], gt_xyz [N,3,S,S]")
    if q is not None:
        q = _chk(q, "q")
        if tuple(q.shape) != (N, 1, r, r):
            raise RuntimeError("view_terms: q must be [N,1,r,r]")
    L = _lib.lib()
    ws = _sg_workspace(weights.device, L.p3d_view_terms_workspace_bytes(N, r))
    sums = torch.empty((2,), dtype=torch.float32, device=weights.device)
    gw = torch.empty_like(weights) if want_grad else None
    gx = torch.empty_like(xyz) if want_grad else None
    count = N * r * r
    with _on(weights.device):
        rc = L.p3d_view_terms_f32(_p(weights), _p(xyz), _p(gt_alpha), _p(gt_xyz), _p(q), N, r, S, DEPTH_MODES[depth_mode], 1.0 / count,
                                  1.0 / count, _p(sums), _p(gw), _p(gx), _p(ws), ws.numel(), _stream())
    _lib.check(rc, "p3d_view_terms_f32")
    return sums / count, gw, gx


class _ViewTermsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, weights, xyz, gt_alpha, gt_xyz, depth_mode, q):
        terms, gw, gx = _view_terms_impl(weights, xyz, gt_alpha, gt_xyz, depth_mode, q, True)
        ctx.save_for_backward(gw, gx)
        return terms

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        gw, gx = ctx.saved_tensors
        return (gw * g[0] if ctx.needs_input_grad[0] else None), (gx * g[1] if ctx.needs_input_grad[1] else None), None, None, None, None


def view_terms(weights, xyz, gt_alpha, gt_xyz, depth_mode, q=None):
    """The render-resolution terms of one supervised view (p3d_view_terms_f32): a [2] tensor (alpha term, depth term), each the mean
    over the N r^2 texels as the reference's .mean() takes it.  depth_mode 'z' | 'x' | 'norm'; q: an optional [N,1,r,r] texel weight.
    The ground truth and the masks carry no gradient.  Under autograd the gradients of weights and xyz are written by the forward
    launch and multiplied by the incoming cotangents in backward."""
    if _wants_grad(weights, xyz):
        return _ViewTermsFn.apply(weights, xyz, gt_alpha, gt_xyz, depth_mode, q)
    return _view_terms_impl(weights, xyz, gt_alpha, gt_xyz, depth_mode, q, False)[0]


# ======================================================================================================================
# The optimiser step (include/p3d_optim.h)
# ======================================================================================================================
_OPTIM_STEP_DTYPE = np.dtype([("grad", "<u8"), ("step_size", "<f4"), ("bc2_sqrt", "<f4"), ("ema_w", "<f4"), ("grad_aligned16", "<i4")])
_OPTIM_STAGING = 2  # pinned staging buffers of a table, used in turn


def _optim_is_device(t):
    return t.is_cuda


def _optim_chk(t, name):
    """A tensor the kernel writes in place: it has to be a float32 device tensor and dense as it is (a copy would take the write)."""
    if not isinstance(t, torch.Tensor) or not _optim_is_device(t):
        raise RuntimeError(f"{name} must be a CUDA/ROCm tensor (the HIP path has no CPU fallback)")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name} must be torch.float32, got {t.dtype}")
    if not t.is_contiguous():
        raise RuntimeError(f"{name} must be contiguous: the optimiser step writes it in place")
    return t


class _OptimTable:
    """What an optimiser uploads ONCE: the static tensor table (p, m, v, ema pointers, numels, alignment flags) and the chunk plan,
    both in device memory, and what it needs per step: the device buffer of the per-step entries and pinned staging for it.  The
    staging buffers are used in turn, and each is reused only after the event recorded behind its last copy has completed: the copy
    engine may still be reading it when the host gets here again.  The device copy of the per-step entries is rewritten in stream order:
    the steps of one table belong on one stream."""

    def __init__(self, key, device, rows, numels):
        L = _lib.lib()
        n = len(rows)
        tab = (_lib.OptimTensor * n)()
        for i, (ptrs, numel) in enumerate(zip(rows, numels)):
            arr = (C.c_void_p * 4)(*ptrs)
            tab[i].p, tab[i].m, tab[i].v, tab[i].ema = ptrs
            tab[i].numel, tab[i].aligned16 = numel, L.p3d_optim_aligned16(arr, 4)
        nm = (C.c_int64 * n)(*numels)
        self.n_chunks = L.p3d_optim_plan(nm, n, None, 0)
        if self.n_chunks < 0:
            _lib.check(int(self.n_chunks), "p3d_optim_plan")
        plan = (_lib.OptimChunk * max(self.n_chunks, 1))()
        if self.n_chunks > 0 and L.p3d_optim_plan(nm, n, plan, self.n_chunks) != self.n_chunks:
            raise RuntimeError("p3d_optim_plan: the plan does not have the size it announced")
        up = lambda c: torch.frombuffer(bytearray(bytes(c)), dtype=torch.uint8).to(device)
        self.key, self.device, self.n = key, device, n
        self.tensors, self.chunks = up(tab), up(plan)
        nbytes = n * _OPTIM_STEP_DTYPE.itemsize
        self.steps = torch.empty(nbytes, dtype=torch.uint8, device=device)
        self.staging = [torch.empty(nbytes, dtype=torch.uint8).pin_memory() for _ in range(_OPTIM_STAGING)]
        self.views = [s.numpy().view(_OPTIM_STEP_DTYPE) for s in self.staging]
        self.events = [None] * _OPTIM_STAGING
        self.turn = 0

    def upload(self, grad_ptrs, step_sizes, bc2_sqrts, ema_weights):
        """Fill the next staging buffer and copy it to the device on the current stream; the launch that follows on that stream
        reads the copy."""
        i = self.turn
        self.turn = (i + 1) % _OPTIM_STAGING
        if self.events[i] is not None:
            self.events[i].synchronize()
        v = self.views[i]
        v["grad"], v["step_size"], v["bc2_sqrt"], v["ema_w"] = grad_ptrs, step_sizes, bc2_sqrts, ema_weights
        v["grad_aligned16"] = (v["grad"] & 15) == 0
        self.steps.copy_(self.staging[i], non_blocking=True)
        if self.events[i] is None:
            self.events[i] = torch.cuda.Event()
        self.events[i].record()


assert _OPTIM_STEP_DTYPE.itemsize == C.sizeof(_lib.OptimStep)


def _adam_ema_impl(params, grads, exp_avgs, exp_avg_sqs, emas, step_sizes, bc2_sqrts, ema_weights, beta1, beta2, eps, grad_scale, sanitize,
                   table, key=None):
    """The launch of p3d_optim_step_f32.  Lists of equal length; grads / exp_avgs / exp_avg_sqs None = mode EMA, emas None = mode ADAM;
    an entry of grads may be None (the tensor is skipped), and so may the moments of such a tensor.  key: what _optim_key gives for
    these tensors.  Returns the table to pass next time."""
    n = len(params)
    adam, ema = grads is not None, emas is not None
    device = params[0].device
    if key is None:
        key = _optim_key(params, exp_avgs, exp_avg_sqs, emas)
    if table is None or table.key != key:
        table = _OptimTable(key, device, key[1], key[2])
    if table.n_chunks == 0:
        return table
    zeros = [0.0] * n
    with _on(device):
        table.upload([0 if g is None else g.data_ptr() for g in grads] if adam else [0] * n, step_sizes if adam else zeros,
                     bc2_sqrts if adam else zeros, ema_weights if ema else zeros)
        nan_v, posinf_v, neginf_v = sanitize if sanitize is not None else (0.0, 0.0, 0.0)
        a = _lib.OptimArgs(tensors=table.tensors.data_ptr(), steps=table.steps.data_ptr(), chunks=table.chunks.data_ptr(), n_chunks=table.n_chunks,
                           n_tensors=n, mode=_lib.P3D_OPTIM_EMA if not adam else _lib.P3D_OPTIM_ADAM_EMA if ema else _lib.P3D_OPTIM_ADAM,
                           sanitize=int(sanitize is not None), grad_scale=grad_scale, nan_v=nan_v, posinf_v=posinf_v, neginf_v=neginf_v, eps=eps,
                           beta1=beta1, beta2=beta2)
        rc = _lib.lib().p3d_optim_step_f32(C.byref(a), _stream())
    _lib.check(rc, "p3d_optim_step_f32")
    return table


def _optim_key(params, exp_avgs, exp_avg_sqs, emas):
    """What a table was built from: the device, (p, m, v, ema) pointers per tensor (0: none) and the numels."""
    none = [None] * len(params)
    ptr = lambda t: 0 if t is None else t.data_ptr()
    rows = tuple(zip(map(ptr, params), map(ptr, exp_avgs or none), map(ptr, exp_avg_sqs or none), map(ptr, emas or none)))
    return params[0].device, rows, tuple(p.numel() for p in params)


def adam_ema_step(params, grads=None, exp_avgs=None, exp_avg_sqs=None, step_sizes=None, bc2_sqrts=None, *, beta1=0.0, beta2=0.999, eps=1e-8,
                  grad_scale=1.0, sanitize=None, ema_params=None, ema_weights=None, table=None):
    """One launch of the optimiser step over any number of tensors (p3d_optim_step_f32; the formulas: include/p3d_optim.h).

    params: the float32 device tensors p.  With grads (a list, an entry None = Adam skips that tensor in this step: p, m, v untouched),
    exp_avgs, exp_avg_sqs and per tensor step_sizes = lr / (1 - beta1^step), bc2_sqrts = sqrt(1 - beta2^step): Adam.  With ema_params
    and ema_weights (per tensor, in [0, 1]: the weight of the OLD ema value; 0 copies): ema <- lerp(p, ema, w) on the new p, for
    every tensor.  Without grads: the EMA update alone.  The gradient is scaled by grad_scale FIRST and cleaned with
    sanitize = (nan, posinf, neginf) after that; a gradient that is not contiguous is copied (rare), one that is a view into a flat
    vector is read where it lies.

    The kernel writes through raw pointers, which the version counters do not see: this function bumps `_version` of every tensor
    the launch wrote (torch.autograd.graph.increment_version), so every cache keyed on a parameter's version (memo.py) sees the step.
    Returns the uploaded table; pass it back as `table` and it is reused while the tensors stay where they are (the tensors a table
    was built from were checked then; the gradients, new tensors at every step, are checked at every step)."""
    params = list(params)
    n = len(params)
    adam, ema = grads is not None, ema_params is not None
    if n == 0:
        return table
    if not adam and not ema:
        raise RuntimeError("adam_ema_step: neither grads nor ema_params: nothing to do")
    lists = [list(x) if x is not None else None for x in (grads, exp_avgs, exp_avg_sqs, ema_params)]
    for name, x in zip(("grads", "exp_avgs", "exp_avg_sqs", "ema_params"), lists):
        if x is not None and len(x) != n:
            raise RuntimeError(f"adam_ema_step: {name} has {len(x)} entries for {n} params")
    grads, exp_avgs, exp_avg_sqs, ema_params = lists
    if adam and (exp_avgs is None or exp_avg_sqs is None or step_sizes is None or bc2_sqrts is None):
        raise RuntimeError("adam_ema_step: grads need exp_avgs, exp_avg_sqs, step_sizes and bc2_sqrts")
    for i, p in enumerate(params):
        if not isinstance(p, torch.Tensor):
            raise RuntimeError(f"params[{i}] must be a CUDA/ROCm tensor (the HIP path has no CPU fallback)")
    key = _optim_key(params, exp_avgs if adam else None, exp_avg_sqs if adam else None, ema_params)
    if table is None or table.key != key:  # tensors this table has not seen: the full checks
        device = params[0].device
        for name, ts in (("params", params), ("exp_avgs", exp_avgs if adam else None), ("exp_avg_sqs", exp_avg_sqs if adam else None), ("ema_params", ema_params)):
            for i, t in enumerate(ts or ()):
                if t is None and name.startswith("exp_avg"):
                    continue
                _optim_chk(t, f"{name}[{i}]")
                if t.numel() != params[i].numel() or t.device != device:
                    raise RuntimeError(f"adam_ema_step: {name}[{i}] does not match params[{i}] (numel) or is on another device")
    wrote = []
    if adam:
        f32, device = torch.float32, params[0].device
        for i, g in enumerate(grads):
            if g is None:
                continue
            if not g.is_contiguous():
                grads[i] = g = g.contiguous()
            if g.dtype is not f32 or g.numel() != key[2][i] or g.device != device:
                _optim_chk(g, f"grads[{i}]")
                raise RuntimeError(f"adam_ema_step: grads[{i}] does not match params[{i}] (numel) or is on another device")
            if exp_avgs[i] is None or exp_avg_sqs[i] is None:
                raise RuntimeError(f"adam_ema_step: params[{i}] has a gradient and no moments")
            if not bc2_sqrts[i] > 0:
                raise RuntimeError(f"adam_ema_step: bc2_sqrts[{i}] must be positive")
            wrote += (params[i], exp_avgs[i], exp_avg_sqs[i])
        if len(step_sizes) != n or len(bc2_sqrts) != n:
            raise RuntimeError("adam_ema_step: step_sizes and bc2_sqrts need one entry per tensor")
        if not (0.0 <= beta1 < 1.0 and 0.0 <= beta2 < 1.0 and eps >= 0.0):
            raise RuntimeError("adam_ema_step: betas in [0, 1) and eps >= 0")
        if sanitize is not None:
            sanitize = tuple(float(x) for x in sanitize)
            if len(sanitize) != 3:
                raise RuntimeError("adam_ema_step: sanitize = (nan, posinf, neginf)")
    if ema:
        ema_weights = [float(w) for w in ema_weights]
        if len(ema_weights) != n or not all(0.0 <= w <= 1.0 for w in ema_weights):
            raise RuntimeError("adam_ema_step: ema_weights needs one entry in [0, 1] per tensor")
        wrote += ema_params
    table = _adam_ema_impl(params, grads, exp_avgs, exp_avg_sqs, ema_params, step_sizes, bc2_sqrts, ema_weights, float(beta1), float(beta2), float(eps),
                           float(grad_scale), sanitize, table, key)
    wrote = [t for t in wrote if t.numel() > 0]
    if wrote:
        torch.autograd.graph.increment_version(wrote)
    return table


# ======================================================================================================================
# LPIPS, the AlexNet perceptual distance (include/p3d_lpips.h).  Seven device operators (the _impl functions, which
# the CPU tests replace by torch stand-ins), their checked public forms, and ops.lpips_distance: the whole distance as ONE autograd
# function, first order, differentiable in the first image only.
# ======================================================================================================================
LPIPS_MIN_SIZE = 31  # below it the second pool has no output (H -> (H - 7) // 4 -> // 2 -> // 2)


def _lpips_out_hw(Hi, Wi, k, stride, pad):
    Ho, Wo = (Hi + 2 * pad - k) // stride + 1, (Wi + 2 * pad - k) // stride + 1
    if not (1 <= k <= _lib.P3D_LPIPS_MAX_K and 1 <= stride <= _lib.P3D_LPIPS_MAX_STRIDE and 0 <= pad < k):
        raise ValueError(f"lpips convolution: k {k} (1..11), stride {stride} (1..4), pad {pad} (0..k-1)")
    if Hi + 2 * pad < k or Wi + 2 * pad < k:
        raise ValueError("lpips convolution: the padded input is smaller than the kernel")
    return Ho, Wo


def _lpips_conv_relu_impl(x, wk, bias, k, stride, pad, shift, scale):
    x, wk = _chk(x, "x"), _chk(wk, "wk")  # (the first operator of ops.lpips_distance: its images and weights are checked here)
    N, Ci, Hi, Wi = x.shape
    Co = wk.shape[2]
    Ho, Wo = _lpips_out_hw(Hi, Wi, k, stride, pad)
    out = torch.empty((N, Co, Ho, Wo), dtype=torch.float32, device=x.device)
    with _on(x.device):
        rc = _lib.lib().p3d_lpips_conv_relu_f32(_p(x), N, Ci, Hi, Wi, _p(wk), k, Co, Ho, Wo, stride, pad, _p(bias), _p(shift), _p(scale), _p(out),
                                                _stream())
    _lib.check(rc, "p3d_lpips_conv_relu_f32")
    return out


def _lpips_conv_relu_backward_impl(g_in, g_head, a, wkb, k, Ci, Hi, Wi, stride, pad, scale):
    some = g_in if g_in is not None else g_head
    N, Co, Ho, Wo = some.shape
    gx = torch.empty((N, Ci, Hi, Wi), dtype=torch.float32, device=some.device)
    with _on(some.device):
        rc = _lib.lib().p3d_lpips_conv_relu_backward_f32(_p(g_in), _p(g_head), _p(a), N, Co, Ho, Wo, _p(wkb), k, Ci, Hi, Wi, stride, pad, _p(scale),
                                                         _p(gx), _stream())
    _lib.check(rc, "p3d_lpips_conv_relu_backward_f32")
    return gx


def _lpips_pool_impl(x):
    N, Cc, H, W = x.shape
    y = torch.empty((N, Cc, (H - 3) // 2 + 1, (W - 3) // 2 + 1), dtype=torch.float32, device=x.device)
    with _on(x.device):
        rc = _lib.lib().p3d_lpips_pool_f32(_p(x), N * Cc, H, W, _p(y), _stream())
    _lib.check(rc, "p3d_lpips_pool_f32")
    return y


def _lpips_pool_backward_impl(x, g):
    N, Cc, H, W = x.shape
    gx = torch.empty_like(x)
    with _on(x.device):
        rc = _lib.lib().p3d_lpips_pool_backward_f32(_p(x), _p(g), N * Cc, H, W, _p(gx), _stream())
    _lib.check(rc, "p3d_lpips_pool_backward_f32")
    return gx


def _lpips_head_impl(a0, a1, lin, v, out, accumulate):
    """Writes v [N] (this layer's value) and, when out [N] is given, out = v (accumulate False) or out + v."""
    N, Cc = a0.shape[0], a0.shape[1]
    HW = a0.numel() // (N * Cc)
    L = _lib.lib()
    nbytes = L.p3d_lpips_head_workspace_bytes(N, HW)
    ws = _sg_workspace(a0.device, nbytes)
    with _on(a0.device):
        rc = L.p3d_lpips_head_f32(_p(a0), _p(a1), _p(lin), N, Cc, HW, _p(v), _p(out), int(bool(accumulate)), _p(ws), ws.numel(), _stream())
    _lib.check(rc, "p3d_lpips_head_f32")


def _lpips_head_backward_impl(a0, a1, lin, g, g_add=None, relu_mask=False):
    N, Cc = a0.shape[0], a0.shape[1]
    g_a0 = torch.empty_like(a0)
    with _on(a0.device):
        rc = _lib.lib().p3d_lpips_head_backward_f32(_p(a0), _p(a1), _p(lin), _p(g), N, Cc, a0.numel() // (N * Cc), _p(g_add), int(bool(relu_mask)),
                                                    _p(g_a0), _stream())
    _lib.check(rc, "p3d_lpips_head_backward_f32")
    return g_a0


def _lpips_chk(t, name, shape=None, ndim=None):
    t = _chk(t, name)
    if (ndim is not None and t.ndim != ndim) or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise ValueError(f"{name}: shape {tuple(t.shape)}, expected {tuple(shape) if shape is not None else f'{ndim} dimensions'}")
    return t


def lpips_conv_relu(x, wk, bias, k, stride, pad, shift=None, scale=None):
    """max(corr(in, wk) + bias, 0) in one launch (p3d_lpips_conv_relu_f32): x [N,Ci,H,W]; wk [k*k,Ci,Co] = weight.permute(2, 3, 1, 0);
    bias [Co]; shift, scale [Ci] (both or neither): in = (x - shift) / scale, zero padding applied after it."""
    x = _lpips_chk(x, "x", ndim=4)
    Ci = x.shape[1]
    wk = _lpips_chk(wk, "wk", ndim=3)
    if wk.shape[0] != k * k or wk.shape[1] != Ci:
        raise ValueError(f"wk: shape {tuple(wk.shape)}, expected ({k * k}, {Ci}, Co)")
    bias = _lpips_chk(bias, "bias", (wk.shape[2],))
    if (shift is None) != (scale is None):
        raise ValueError("lpips_conv_relu: shift and scale come together")
    if shift is not None:
        shift, scale = _lpips_chk(shift, "shift", (Ci,)), _lpips_chk(scale, "scale", (Ci,))
    _lpips_out_hw(x.shape[2], x.shape[3], int(k), int(stride), int(pad))
    return _lpips_conv_relu_impl(x, wk, bias, int(k), int(stride), int(pad), shift, scale)


def lpips_conv_relu_backward(g_in, g_head, a, wkb, k, Ci, Hi, Wi, stride, pad, scale=None):
    """The layer's data gradient (p3d_lpips_conv_relu_backward_f32): the cotangents g_in and g_head (either may be None), masked by the
    stored output a > 0 (a None: taken as they are, masked already) -> [N,Ci,Hi,Wi].  wkb: stride 1: the flipped, transposed weights [k*k,Co,Ci] (lpips_backward_weights);
    stride > 1 (the stem): the forward's wk [k*k,Ci,Co], Ci <= 4.  scale [Ci]: the scaling layer's division (the stem only)."""
    if g_in is None and g_head is None:
        raise ValueError("lpips_conv_relu_backward: no cotangent")
    shape = (g_in if g_in is not None else g_head).shape
    a = _lpips_chk(a, "a", shape, ndim=4) if a is not None else None
    g_in = _lpips_chk(g_in, "g_in", shape, ndim=4) if g_in is not None else None
    g_head = _lpips_chk(g_head, "g_head", shape, ndim=4) if g_head is not None else None
    k, Ci, Hi, Wi, stride, pad = int(k), int(Ci), int(Hi), int(Wi), int(stride), int(pad)
    if _lpips_out_hw(Hi, Wi, k, stride, pad) != tuple(shape[2:]):
        raise ValueError("lpips_conv_relu_backward: the cotangent does not have the layer's output size for an input of Hi x Wi")
    Co = shape[1]
    wkb = _lpips_chk(wkb, "wkb", (k * k, Co, Ci) if stride == 1 else (k * k, Ci, Co))
    if stride > 1 and Ci > _lib.P3D_LPIPS_BWD_MAX_CI:
        raise ValueError(f"lpips_conv_relu_backward: a strided layer's backward takes at most {_lib.P3D_LPIPS_BWD_MAX_CI} input channels")
    if scale is not None:
        if stride == 1:
            raise ValueError("lpips_conv_relu_backward: the scaling layer sits in front of the strided stem only")
        scale = _lpips_chk(scale, "scale", (Ci,))
    return _lpips_conv_relu_backward_impl(g_in, g_head, a, wkb, k, Ci, Hi, Wi, stride, pad, scale)


def lpips_backward_weights(wk):
    """wk [k*k,Ci,Co] -> [k*k,Co,Ci] with the taps reversed: the operand of a stride-1 layer's data gradient."""
    return wk.detach().flip(0).transpose(1, 2).contiguous()


def lpips_pool(x):
    """3 x 3 stride-2 maximum, no padding, floor mode: [N,C,H,W] -> [N,C,(H-3)//2+1,(W-3)//2+1]."""
    x = _lpips_chk(x, "x", ndim=4)
    if x.shape[2] < 3 or x.shape[3] < 3:
        raise ValueError("lpips_pool: the input is smaller than the window")
    return _lpips_pool_impl(x)


def lpips_pool_backward(x, g):
    """The pool's backward as a gather: each cotangent goes to the first maximum of its window in row-major scan order."""
    x = _lpips_chk(x, "x", ndim=4)
    if x.shape[2] < 3 or x.shape[3] < 3:
        raise ValueError("lpips_pool_backward: the input is smaller than the window")
    g = _lpips_chk(g, "g", (x.shape[0], x.shape[1], (x.shape[2] - 3) // 2 + 1, (x.shape[3] - 3) // 2 + 1))
    return _lpips_pool_backward_impl(x, g)


def _lpips_head_args(a0, a1, lin):
    a0 = _lpips_chk(a0, "a0")
    if a0.ndim < 2:
        raise ValueError("a0: [N,C,...]")
    return a0, _lpips_chk(a1, "a1", a0.shape), _lpips_chk(lin.reshape(-1), "lin", (a0.shape[1],))


def lpips_head(a0, a1, lin):
    """One layer's value v [N] = mean over pixels of sum_c lin[c] (a0 / (|a0| + 1e-10) - a1 / (|a1| + 1e-10))^2 (p3d_lpips_head_f32)."""
    a0, a1, lin = _lpips_head_args(a0, a1, lin)
    v = torch.empty((a0.shape[0],), dtype=torch.float32, device=a0.device)
    _lpips_head_impl(a0, a1, lin, v, None, False)
    return v


def lpips_head_backward(a0, a1, lin, g, g_add=None, relu_mask=False):
    """The head's cotangent of a0 for the cotangent g [N] of its value (p3d_lpips_head_backward_f32); finite where a pixel of a0 is 0.
    g_add (a0's shape): added to it in the same pass; relu_mask: the sum kept only where a0 > 0 — together the finished cotangent of
    the layer's pre-activation, which lpips_conv_relu_backward then takes with a=None."""
    a0, a1, lin = _lpips_head_args(a0, a1, lin)
    g_add = _lpips_chk(g_add, "g_add", a0.shape) if g_add is not None else None
    return _lpips_head_backward_impl(a0, a1, lin, _lpips_chk(g.reshape(-1), "g", (a0.shape[0],)), g_add, relu_mask)


LPIPS_DOUBLE_BACKWARD_MESSAGE = ("the LPIPS distance's HIP backward is first order only: a gradient of its gradient (create_graph=True) "
                                 "is not implemented")


class _LpipsFn(torch.autograd.Function):
    """The whole distance (include/p3d_lpips.h): forward 5 convolutions, 2 pools and 5 heads over the pair as one batch of 2N; backward,
    from the last layer to the first: the pool's gather where a pool follows, the head's backward — which adds the incoming cotangent
    and applies the mask a_l > 0 in the same pass —, the layer's data gradient of that one tensor.  Only in0 receives a gradient; the weights are constants."""

    @staticmethod
    def forward(ctx, in0, in1, net):
        out, saved = _lpips_forward(in0, in1, net)
        ctx.net, ctx.hw = net, tuple(in0.shape[2:])
        ctx.save_for_backward(*saved)
        return out

    @staticmethod
    def backward(ctx, g):
        if torch.is_grad_enabled():
            raise RuntimeError(LPIPS_DOUBLE_BACKWARD_MESSAGE)
        return _lpips_backward_once(ctx, g)


@torch.autograd.function.once_differentiable
def _lpips_backward_once(ctx, g):
    net, acts = ctx.net, ctx.saved_tensors
    N = acts[0].shape[0] // 2
    g = g.reshape(-1).contiguous()
    g_in = None  # the cotangent of a_l that arrives from the layers after it
    for l in range(len(acts) - 1, -1, -1):
        wk, bias, wkb, lin, k, stride, pad, pool_after = net["layers"][l]
        a = acts[l]
        if pool_after and g_in is not None:
            g_in = _lpips_pool_backward_impl(a[:N], g_in)
        gz = _lpips_head_backward_impl(a[:N], a[N:], lin, g, g_in, True)  # a_l > 0 ? g_in + g_head : 0
        if l > 0:
            prev = acts[l - 1]
            Hi, Wi = ((prev.shape[2] - 3) // 2 + 1, (prev.shape[3] - 3) // 2 + 1) if net["layers"][l - 1][7] else tuple(prev.shape[2:])
            Ci = prev.shape[1]
        else:
            (Hi, Wi), Ci = ctx.hw, net["shift"].shape[0]
        g_in = _lpips_conv_relu_backward_impl(gz, None, None, wkb, k, Ci, Hi, Wi, stride, pad, net["scale"] if l == 0 else None)
    return g_in, None, None


def _lpips_forward(in0, in1, net):
    N = in0.shape[0]
    x = torch.cat([in0, in1])  # one launch per layer for the pair: both images share the weights
    acts = []
    for l, (wk, bias, wkb, lin, k, stride, pad, pool_after) in enumerate(net["layers"]):
        x = _lpips_conv_relu_impl(x, wk, bias, k, stride, pad, net["shift"] if l == 0 else None, net["scale"] if l == 0 else None)
        acts.append(x)
        if pool_after:
            x = _lpips_pool_impl(x)
    v = torch.empty((len(acts), N), dtype=torch.float32, device=in0.device)
    out = torch.empty((N,), dtype=torch.float32, device=in0.device)
    for l, a in enumerate(acts):
        _lpips_head_impl(a[:N], a[N:], net["layers"][l][3], v[l], out, l > 0)
    return out.view(N, 1, 1, 1), acts


def lpips_distance(in0, in1, net):
    """The LPIPS distance [N,1,1,1] of in0 and in1 [N,3,H,W] (H, W >= 31) on the operands `net` (LPIPS.operands()): shift, scale [3]
    and per layer (wk, bias, wkb, lin, k, stride, pad, pool_after).  The same launches, hence the same bits, with and without a
    recorded backward; the backward is first order and reaches in0 only (a target that requires grad raises)."""
    for name, t in (("in0", in0), ("in1", in1)):
        if not isinstance(t, torch.Tensor) or t.ndim != 4 or t.shape[1] != net["shift"].shape[0]:
            raise ValueError(f"{name}: expected [N,{net['shift'].shape[0]},H,W]")
    if in0.shape != in1.shape:
        raise ValueError(f"in0 {tuple(in0.shape)} and in1 {tuple(in1.shape)} differ in shape")
    if min(in0.shape[2:]) < LPIPS_MIN_SIZE:
        raise ValueError(f"LPIPS needs H, W >= {LPIPS_MIN_SIZE} (the second pool has no output below): got {tuple(in0.shape[2:])}")
    if torch.is_grad_enabled() and in1.requires_grad:
        raise NotImplementedError("LPIPS: the gradient with respect to the target (in1) is not implemented: detach it")
    in0c, in1c = _lpips_image(in0, "in0"), _lpips_image(in1, "in1")
    if _wants_grad(in0):
        return _LpipsFn.apply(in0c, in1c.detach(), net)
    return _lpips_forward(in0c, in1c, net)[0]


def _lpips_image(t, name):
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name} must be torch.float32, got {t.dtype}")
    return t.contiguous()


# ======================================================================================================================
# The conditioning encoder (include/p3d_encoder.h): a ResNet's layers with folded batch norm, the image front end and
# the walk of a whole network's table in one C call.  Inference only.  Four device operators (the _impl functions, which the CPU tests
# replace by torch stand-ins) and their checked public forms.
# ======================================================================================================================
def _enc_out_hw(H, W, k, stride):
    if k not in (1, 3, 7) or stride not in (1, 2):
        raise ValueError(f"encoder convolution: k {k} (1, 3 or 7), stride {stride} (1 or 2)")
    pad = (k - 1) // 2
    return (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


def enc_resize_hw(H, W, size):
    """torchvision's Resize(int): the shorter side becomes `size`, the longer one int(size * long / short)."""
    H, W, size = int(H), int(W), int(size)
    if size < 1 or H < 1 or W < 1:
        raise ValueError("encoder: sizes are positive")
    return (int(size * H / W), size) if W <= H else (size, int(size * W / H))


def enc_conv_plan(N, Ci, Co, Ho, Wo, k, stride, force_plan=0):
    """The host-side plan of one convolution (p3d_enc_conv_plan, no GPU needed): dict(code, tile, split, cps, workgroups, workspace_bytes)."""
    L = _lib.lib()
    out = (C.c_int * 4)()
    code = L.p3d_enc_conv_plan(N, Ci, Co, Ho, Wo, k, stride, int(force_plan), out)
    if code < 0:
        _lib.check(code, "p3d_enc_conv_plan")
    return dict(code=code, tile=out[0], split=out[1], cps=out[2], workgroups=out[3],
                workspace_bytes=L.p3d_enc_conv_workspace_bytes(N, Ci, Co, Ho, Wo, k, stride, int(force_plan)))


def _enc_conv_impl(x, wk, bias, k, stride, res, relu, force_plan):
    x, wk, bias = _chk(x, "x"), _chk(wk, "wk"), _chk(bias, "bias")
    res = _chk(res, "res") if res is not None else None
    N, Ci, H, W = x.shape
    Co = wk.shape[2]
    Ho, Wo = _enc_out_hw(H, W, k, stride)
    L = _lib.lib()
    out = torch.empty((N, Co, Ho, Wo), dtype=torch.float32, device=x.device)
    ws = _sg_workspace(x.device, L.p3d_enc_conv_workspace_bytes(N, Ci, Co, Ho, Wo, k, stride, force_plan))
    with _on(x.device):
        rc = L.p3d_enc_conv_f32(_p(x), N, Ci, H, W, _p(wk), k, stride, Co, _p(bias), _p(res), _lib.P3D_ENC_RELU if relu else 0, _p(out), force_plan,
                                _p(ws), ws.numel(), _stream())
    _lib.check(rc, "p3d_enc_conv_f32")
    return out


def _enc_maxpool_impl(x):
    x = _chk(x, "x")
    N, Cc, H, W = x.shape
    y = torch.empty((N, Cc, (H - 1) // 2 + 1, (W - 1) // 2 + 1), dtype=torch.float32, device=x.device)
    with _on(x.device):
        rc = _lib.lib().p3d_enc_maxpool_f32(_p(x), N * Cc, H, W, _p(y), _stream())
    _lib.check(rc, "p3d_enc_maxpool_f32")
    return y


def _enc_prepare_impl(img, mean, std, h, w):
    img, mean, std = _chk(img, "img"), _chk(mean, "mean"), _chk(std, "std")
    N, Cc, H, W = img.shape
    out = torch.empty((2 * N, 3, h, w), dtype=torch.float32, device=img.device)
    with _on(img.device):
        rc = _lib.lib().p3d_enc_prepare_f32(_p(img), N, Cc, H, W, _p(mean), _p(std), h, w, _p(out), _stream())
    _lib.check(rc, "p3d_enc_prepare_f32")
    return out


def enc_conv(x, wk, bias, k, stride=1, res=None, relu=False, force_plan=0):
    """[relu](corr(x, wk) + bias [+ res]) (p3d_enc_conv_f32): x [N,Ci,H,W]; wk [k*k,Ci,Co] = weight.permute(2, 3, 1, 0); bias [Co]; res
    None or [N,Co,Ho,Wo]; k 1, 3 or 7, stride 1 or 2, pad (k - 1) / 2.  force_plan: 0 chooses, else (tile << 8) | split (enc_conv_plan)."""
    x = _lpips_chk(x, "x", ndim=4)
    k, stride = int(k), int(stride)
    Ho, Wo = _enc_out_hw(x.shape[2], x.shape[3], k, stride)
    wk = _lpips_chk(wk, "wk", (k * k, x.shape[1], wk.shape[2] if isinstance(wk, torch.Tensor) and wk.ndim == 3 else -1))
    bias = _lpips_chk(bias, "bias", (wk.shape[2],))
    if res is not None:
        res = _lpips_chk(res, "res", (x.shape[0], wk.shape[2], Ho, Wo))
    return _enc_conv_impl(x, wk, bias, k, stride, res, bool(relu), int(force_plan))


def enc_maxpool(x):
    """3 x 3 stride-2 maximum with padding 1 (the padding never wins): [N,C,H,W] -> [N,C,(H-1)//2+1,(W-1)//2+1]."""
    return _enc_maxpool_impl(_lpips_chk(x, "x", ndim=4))


def enc_prepare(img, mean, std, size):
    """The encoder's front end in one launch (p3d_enc_prepare_f32): img [N,C>=3,H,W] in [0, 1] -> [2N,3,h,w]: the first three channels
    resized bilinearly (align_corners=False, no antialiasing) to enc_resize_hw(H, W, size) and normalised by mean / std [3]; rows N..2N-1
    hold the same of the horizontally mirrored image."""
    img = _lpips_chk(img, "img", ndim=4)
    if img.shape[1] < 3:
        raise ValueError(f"img: shape {tuple(img.shape)}, expected at least three channels")
    mean, std = _lpips_chk(mean, "mean", (3,)), _lpips_chk(std, "std", (3,))
    h, w = enc_resize_hw(img.shape[2], img.shape[3], size)
    return _enc_prepare_impl(img, mean, std, h, w)


class EncoderProgram:
    """A whole network as p3d_encoder_forward_f32 takes it: the table of layer records, one weight blob, the activation arena.
    records: dicts with kind ('conv' | 'maxpool' | 'prepare'), shape (N, Ci, H, W), out_shape (N', Co, Ho, Wo), src / dst / res (buffer
    indices, res None), k, stride, relu, plan, and w / b (conv: wk, bias; prepare: mean, std).  buf_len: floats per buffer."""
    KINDS = {"conv": _lib.P3D_ENC_KIND_CONV, "maxpool": _lib.P3D_ENC_KIND_MAXPOOL, "prepare": _lib.P3D_ENC_KIND_PREPARE}

    def __init__(self, records, buf_len, device):
        self.records, self.device = list(records), torch.device(device)
        self.table = (_lib.EncLayer * len(self.records))()
        parts, off = [], 0
        for i, r in enumerate(self.records):
            t = self.table[i]
            t.kind = self.KINDS[r["kind"]]
            t.N, t.Ci, t.H, t.W = r["shape"]
            _, t.Co, t.Ho, t.Wo = r["out_shape"]
            t.k, t.stride = (r["k"], r["stride"]) if r["kind"] == "conv" else (0, 0)
            t.in_, t.out, t.res = r["src"], r["dst"], -1 if r.get("res") is None else r["res"]
            t.flags, t.plan, t.reserved = (_lib.P3D_ENC_RELU if r.get("relu") else 0), int(r.get("plan", 0)), 0
            offs = []
            for name in ("w", "b"):
                if r["kind"] == "maxpool":
                    offs.append(0)
                    continue
                v = r[name].detach().to(torch.float32).reshape(-1)
                offs.append(off)
                parts.append(v)
                off += v.numel()
            t.w_off, t.b_off = offs
        self.weights = torch.cat(parts).to(self.device).contiguous() if parts else torch.zeros(1, device=self.device)
        self.n_bufs = len(buf_len)
        self.buf_len = (C.c_int64 * self.n_bufs)(*[int(n) for n in buf_len])
        offs, at = [], 0
        for n in buf_len:
            offs.append(at)
            at += (int(n) + 63) // 64 * 64  # every buffer starts on a 256-byte boundary
        self.buf_off = (C.c_int64 * self.n_bufs)(*offs)
        self.arena = torch.empty((max(at, 1),), dtype=torch.float32, device=self.device)
        self.launches = None  # (set by the first run: kernels per call)

    def buffer(self, b, shape):
        n = 1
        for s in shape:
            n *= int(s)
        return self.arena[self.buf_off[b]:self.buf_off[b] + n].view(*shape)


def _encoder_forward_impl(prog):
    _chk(prog.arena, "the program's arena"), _chk(prog.weights, "the program's weights")
    L = _lib.lib()
    ws = _sg_workspace(prog.device, L.p3d_encoder_workspace_bytes(prog.table, len(prog.records)))
    with _on(prog.device):
        rc = L.p3d_encoder_forward_f32(prog.table, len(prog.records), _p(prog.weights), prog.weights.numel(), _p(prog.arena), prog.arena.numel(),
                                       prog.buf_off, prog.buf_len, prog.n_bufs, _p(ws), ws.numel(), _stream())
    _lib.check(rc, "p3d_encoder_forward_f32")


def encoder_forward(prog, img, src=0):
    """Run a whole EncoderProgram in ONE call into the library: img is copied into buffer `src` of the arena, every layer is launched
    on the current stream; the results are read with prog.buffer(index, shape) (views of the arena: clone what has to outlive the next call)."""
    if not isinstance(prog, EncoderProgram):
        raise TypeError("encoder_forward: an EncoderProgram")
    if not isinstance(img, torch.Tensor) or img.dtype != torch.float32 or img.device != prog.arena.device:
        raise RuntimeError(f"img must be a torch.float32 tensor on {prog.arena.device}")
    if img.numel() != prog.buf_len[src]:
        raise ValueError(f"img: {img.numel()} values, the program was built for {prog.buf_len[src]}")
    prog.arena[prog.buf_off[src]:prog.buf_off[src] + img.numel()].copy_(img.reshape(-1))
    _encoder_forward_impl(prog)
    return prog


# ---- the geometry metrics (include/p3d_metrics.h) -----------------------------------------------------------------------------------------
def point_mesh_plan(Q, F, slices=0, cull=True):
    """p3d_point_mesh_plan: dict(qblocks, ntiles, slices, tiles_per_slice, query_block, face_tile) of a call with these sizes."""
    out = (C.c_int64 * 6)()
    flags = (0 if cull else _lib.P3D_PM_NO_CULL) | (int(slices) << _lib.P3D_PM_SLICES_SHIFT)
    _lib.check(_lib.lib().p3d_point_mesh_plan(int(Q), int(F), flags, out, 6), "p3d_point_mesh_plan")
    return dict(zip(("qblocks", "ntiles", "slices", "tiles_per_slice", "query_block", "face_tile"), (int(x) for x in out)))


def point_mesh_dist2(points, verts, faces, cull=False, cull_margin=0.0, slices=0, want_face=True, want_closest=True):
    """p3d_point_mesh_dist2_f32: (dist2 [Q], face [Q] int32 or None, closest [Q,3] or None) of points [Q,3] against the mesh verts [V,3],
    faces [F,3] int32 — whose indices the CALLER has checked (panic3d_amd.metrics.point_mesh_squared_distance does).  cull: skip far
    face tiles (bit-identical outputs; wants spatially sorted points and cull_margin = 64 * 2^-24 * D^2); slices: force the number of
    face slices (0: the plan's)."""
    points, verts, faces = _chk(points, "points"), _chk(verts, "verts"), _chk(faces, "faces", torch.int32)
    if points.dim() != 2 or points.shape[1] != 3 or verts.dim() != 2 or verts.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise RuntimeError("point_mesh_dist2: points [Q,3], verts [V,3], faces [F,3]")
    Q, V, F = points.shape[0], verts.shape[0], faces.shape[0]
    L = _lib.lib()
    dev = points.device
    ws = _sg_workspace(dev, L.p3d_point_mesh_workspace_bytes(Q, max(F, 1)))
    d2 = torch.empty((Q,), dtype=torch.float32, device=dev)
    face = torch.empty((Q,), dtype=torch.int32, device=dev) if want_face else None
    closest = torch.empty((Q, 3), dtype=torch.float32, device=dev) if want_closest else None
    flags = (0 if cull else _lib.P3D_PM_NO_CULL) | (int(slices) << _lib.P3D_PM_SLICES_SHIFT)
    with _on(dev):
        rc = L.p3d_point_mesh_dist2_f32(_p(points), Q, _p(verts), V, _p(faces), F, flags, float(cull_margin), _p(d2), _p(face), _p(closest),
                                        _p(ws), ws.numel(), _stream())
    _lib.check(rc, "p3d_point_mesh_dist2_f32")
    return d2, face, closest


# ======================================================================================================================
# The illustration-to-render module (include/p3d_rmline.h): the line mask in one launch, one unpadded 3 x 3 convolution
# per generator layer, and the walk of mask + layers in one C call.  Inference only.  Three device operators (the _impl functions, which
# the CPU tests replace by torch stand-ins) and their checked public forms.
# ======================================================================================================================
RMLINE_ACTS = {"none": _lib.P3D_RMLINE_ACT_NONE, "leaky": _lib.P3D_RMLINE_ACT_LEAKY, "tanh": _lib.P3D_RMLINE_ACT_TANH}
RMLINE_DOG = dict(t=1.0, sigma=0.5, k=1.6, epsilon=0.01, kernel_factor=4, d=2)  # rmline_wrapper.py:24-33
RMLINE_LAUNCHES = [0]  # kernels started by rmline_conv and by the training operators below (tests and the bench read the difference)


def rmline_dog_taps(sigma=0.5, k=1.6, kernel_factor=4, **_):
    """(k0, k1): the taps of the two Gaussians (sketchers_v2.py:72-73).  ValueError above P3D_RMLINE_MAX_TAPS = 33 taps, or for k < 1."""
    sigma, k, kernel_factor = float(sigma), float(k), float(kernel_factor)
    if not (sigma > 0 and k > 0 and kernel_factor > 0 and np.isfinite([sigma, k, kernel_factor]).all()):
        raise ValueError("rmline: sigma, k and kernel_factor are positive and finite")
    if sigma * k * kernel_factor >= _lib.P3D_RMLINE_MAX_TAPS or sigma * kernel_factor >= _lib.P3D_RMLINE_MAX_TAPS:
        raise ValueError(f"rmline: more than {_lib.P3D_RMLINE_MAX_TAPS} taps (sigma {sigma}, k {k}, kernel_factor {kernel_factor})")
    k0, k1 = max(2 * int(sigma * kernel_factor) + 1, 3), max(2 * int(sigma * k * kernel_factor) + 1, 3)
    if max(k0, k1) > _lib.P3D_RMLINE_MAX_TAPS:
        raise ValueError(f"rmline: {max(k0, k1)} taps, at most {_lib.P3D_RMLINE_MAX_TAPS} (sigma {sigma}, k {k}, kernel_factor {kernel_factor})")
    if k1 < k0:
        raise ValueError(f"rmline: k {k} makes the second blur narrower than the first ({k1} < {k0} taps)")
    return k0, k1


def rmline_dog_params(dog=None):
    """The detector's parameters as a checked dict: RMLINE_DOG (the wrapper's values) updated by `dog`."""
    p = dict(RMLINE_DOG)
    extra = set(dog or {}) - set(p)
    if extra:
        raise ValueError(f"rmline: unknown detector parameters {sorted(extra)}")
    p.update(dog or {})
    p["d"] = int(p["d"])
    if not 1 <= p["d"] <= _lib.P3D_RMLINE_MAX_DILATE:
        raise ValueError(f"rmline: d {p['d']}, 1..{_lib.P3D_RMLINE_MAX_DILATE}")
    if not np.isfinite([float(p["t"]), float(p["epsilon"])]).all():
        raise ValueError("rmline: t and epsilon are finite")
    rmline_dog_taps(**p)
    return p


def _rmline_dog_struct(p):
    return _lib.RmlineDog(float(p["t"]), float(p["sigma"]), float(p["k"]), float(p["epsilon"]), float(p["kernel_factor"]), int(p["d"]), 0)


def _rmline_mask_impl(img, hull, dog, want_response):
    img = _chk(img, "img")
    hull = _chk(hull, "hull") if hull is not None else None
    N, Cc, H, W = img.shape
    mask = torch.empty((N, 1, H, W), dtype=torch.float32, device=img.device)
    image = torch.empty((N, 3, H, W), dtype=torch.float32, device=img.device) if Cc == 4 else None
    resp = torch.empty((N, 1, H, W), dtype=torch.float32, device=img.device) if want_response else None
    st = _rmline_dog_struct(dog)
    with _on(img.device):
        rc = _lib.lib().p3d_rmline_mask_f32(_p(img), N, Cc, H, W, _p(hull), C.byref(st), _p(mask), _p(image), _p(resp), _stream())
    _lib.check(rc, "p3d_rmline_mask_f32")
    return mask, image, resp


def _rmline_hull_chk(hull, img):
    if hull is None:
        return None
    return _lpips_chk(hull, "hull", (img.shape[0], 1, img.shape[2], img.shape[3]))


def rmline_mask(img, hull=None, dog=None, want_response=False):
    """The line mask in ONE launch (p3d_rmline_mask_f32): img [N,C,H,W], C 1, 3 or 4 (RGBA is composited on white) -> (mask [N,1,H,W] of
    0 / 1, image, response).  image: the composite [N,3,H,W] for C = 4, img itself for C = 3, None for C = 1.  response: the clipped DoG
    response when want_response, else None.  hull [N,1,H,W] (non-zero = inside) is cleared from the mask.  dog: overrides of RMLINE_DOG."""
    img = _lpips_chk(img, "img", ndim=4)
    if img.shape[1] not in (1, 3, 4):
        raise ValueError(f"img: shape {tuple(img.shape)}, expected 1, 3 or 4 channels")
    hull = _rmline_hull_chk(hull, img)
    mask, image, resp = _rmline_mask_impl(img, hull, rmline_dog_params(dog), bool(want_response))
    return mask, (image if img.shape[1] == 4 else (img if img.shape[1] == 3 else None)), resp


def rmline_conv_plan(Ci, Co, force_plan=0):
    """The host-side plan of one layer (p3d_rmline_conv_plan, no GPU needed): dict(plan, rows, cot, lds_bytes).  ValueError for sizes or a
    forced plan the layer refuses."""
    out = (C.c_int * 3)()
    rc = _lib.lib().p3d_rmline_conv_plan(int(Ci), int(Co), int(force_plan), out)
    if rc < 0:
        raise ValueError(f"rmline_conv_plan: Ci {Ci}, Co {Co} (1..{_lib.P3D_RMLINE_MAX_C}), plan {force_plan} (0 chooses, 1 the 8-row tile, 2 the 4-row tile; "
                         "the 8-row tile must fit the LDS)")
    return dict(plan=rc, rows=out[0], cot=out[1], lds_bytes=out[2])


def _rmline_conv_impl(x, image, mask, hull, wk, bias, act, slope, pad, flags, plan):
    wk, bias = _chk(wk, "wk"), _chk(bias, "bias")
    x, image, mask, hull = (_chk(t, n) if t is not None else None for t, n in ((x, "x"), (image, "image"), (mask, "mask"), (hull, "hull")))
    _, Ci, Co = wk.shape
    if x is not None and x.data_ptr() % 16:  # (a view into a larger tensor: the kernel reads channel-last inputs in 16-byte vectors)
        x = x.clone()
    if flags & _lib.P3D_RMLINE_IN_STACK:
        N, Hin, Win = image.shape[0], image.shape[2] + 2 * pad, image.shape[3] + 2 * pad
    else:
        N, Hin, Win = x.shape[0], x.shape[1], x.shape[2]
    shape = (N, Co, Hin - 2, Win - 2) if flags & _lib.P3D_RMLINE_OUT_PLANAR else (N, Hin - 2, Win - 2, Co)
    out = torch.empty(shape, dtype=torch.float32, device=wk.device)
    with _on(wk.device):
        rc = _lib.lib().p3d_rmline_conv_f32(_p(x), _p(image), _p(mask), _p(hull), N, Hin, Win, pad, Ci, _p(wk), _p(bias), Co, act, slope, flags, plan,
                                            _p(out), _stream())
    _lib.check(rc, "p3d_rmline_conv_f32")
    RMLINE_LAUNCHES[0] += 1
    return out


def rmline_conv(x, wk, bias, act="none", slope=0.01, stack=None, pad=0, planar=False, lerp=None, plan=0, per_tap=False):
    """One unpadded 3 x 3 convolution with bias and activation (p3d_rmline_conv_f32).  x [N,Hin,Win,Ci] channel-last; wk [9,Ci,Co] =
    weight.permute(2, 3, 1, 0); bias [Co]; act 'none', 'leaky' (slope) or 'tanh' -> [N,Hin-2,Win-2,Co] channel-last, or [N,Co,Hin-2,Win-2]
    with planar=True.
    stack=(image [N,3,H,W], mask [N,1,H,W] or None, hull [N,1,H,W] or None) in place of x (x None): the reference's stackin built in the
    load, image * (1 - mask) and hull replicate-padded by `pad`.
    lerp=(image [N,3,Ho,Wo], mask [N,1,Ho,Wo]) with planar=True and Co = 3: the store gives torch.lerp(image, act(z), mask).
    per_tap=True (P3D_RMLINE_SUM_PER_TAP): z's sum as one chain per tap, the nine added in order — shorter chains for training, other bits."""
    if act not in RMLINE_ACTS:
        raise ValueError(f"act: one of {sorted(RMLINE_ACTS)}, got {act!r}")
    wk = _lpips_chk(wk, "wk", ndim=3)
    Ci, Co = wk.shape[1], wk.shape[2]
    if wk.shape[0] != 9 or not (1 <= Ci <= _lib.P3D_RMLINE_MAX_C and 1 <= Co <= _lib.P3D_RMLINE_MAX_C):
        raise ValueError(f"wk: shape {tuple(wk.shape)}, expected (9, Ci, Co) with Ci, Co <= {_lib.P3D_RMLINE_MAX_C}")
    bias = _lpips_chk(bias, "bias", (Co,))
    pad, flags = int(pad), 0
    image = mask = hull = None
    if stack is not None:
        if x is not None:
            raise ValueError("rmline_conv: x or stack, not both")
        image, mask, hull = stack
        image = _lpips_chk(image, "image", ndim=4)
        if image.shape[1] != 3:
            raise ValueError(f"image: shape {tuple(image.shape)}, expected three channels")
        mask = _lpips_chk(mask, "mask", (image.shape[0], 1) + tuple(image.shape[2:])) if mask is not None else None
        hull = _rmline_hull_chk(hull, image)
        if Ci != 3 + (hull is not None):
            raise ValueError(f"wk: {Ci} input channels, the stack has {3 + (hull is not None)}")
        if pad < 0:
            raise ValueError("pad: not negative")
        N, Hin, Win = image.shape[0], image.shape[2] + 2 * pad, image.shape[3] + 2 * pad
        flags |= _lib.P3D_RMLINE_IN_STACK
    else:
        x = _lpips_chk(x, "x", ndim=4)
        if x.shape[3] != Ci:
            raise ValueError(f"x: shape {tuple(x.shape)}, expected channel-last with {Ci} channels")
        if pad != 0:
            raise ValueError("pad: only with stack")
        N, Hin, Win = x.shape[0], x.shape[1], x.shape[2]
    if Hin < 3 or Win < 3:
        raise ValueError(f"rmline_conv: a {Hin} x {Win} input is smaller than the filter")
    if planar:
        flags |= _lib.P3D_RMLINE_OUT_PLANAR
    if lerp is not None:
        if not planar or Co != 3:
            raise ValueError("lerp: needs planar=True and three output channels")
        l_image, l_mask = lerp
        l_image = _lpips_chk(l_image, "lerp image", (N, 3, Hin - 2, Win - 2))
        l_mask = _lpips_chk(l_mask, "lerp mask", (N, 1, Hin - 2, Win - 2))
        if stack is not None:
            if l_image.data_ptr() != image.data_ptr() or (mask is not None and l_mask.data_ptr() != mask.data_ptr()):
                raise ValueError("lerp: with stack, the same image and mask")
            if mask is None:
                flags |= _lib.P3D_RMLINE_IN_NO_MASK
        image, mask = l_image, l_mask
        flags |= _lib.P3D_RMLINE_OUT_LERP
    if per_tap:
        flags |= _lib.P3D_RMLINE_SUM_PER_TAP
    rmline_conv_plan(Ci, Co, plan)
    return _rmline_conv_impl(x, image, mask, hull, wk, bias, RMLINE_ACTS[act], float(slope), pad, flags, int(plan))


class RmlineProgram:
    """The generator as p3d_rmline_forward_f32 takes it: the table of layer records and one weight blob.  layers: dicts with wk [9,Ci,Co],
    bias [Co], act ('none' | 'leaky' | 'tanh'), slope, plan."""

    def __init__(self, layers, device):
        self.layers, self.device = list(layers), torch.device(device)
        if not self.layers:
            raise ValueError("RmlineProgram: at least one layer")
        self.table = (_lib.RmlineLayer * len(self.layers))()
        parts, off = [], 0
        for i, (t, l) in enumerate(zip(self.table, self.layers)):
            _, t.Ci, t.Co = l["wk"].shape
            if i and t.Ci != self.table[i - 1].Co:
                raise ValueError(f"RmlineProgram: layer {i} takes {t.Ci} channels, layer {i - 1} gives {self.table[i - 1].Co}")
            t.act, t.plan, t.slope, t.reserved = RMLINE_ACTS[l.get("act", "none")], int(l.get("plan", 0)), float(l.get("slope", 0.01)), 0
            rmline_conv_plan(t.Ci, t.Co, t.plan)
            t.w_off, t.b_off = off, off + l["wk"].numel()
            parts += [l["wk"].detach().to(torch.float32).reshape(-1), l["bias"].detach().to(torch.float32).reshape(-1)]
            off += l["wk"].numel() + l["bias"].numel()
        self.weights = torch.cat(parts).to(self.device).contiguous()
        self.width = max(t.Co for t in self.table)
        self._acts = (None, None)
        self.launches = None  # (set by every run: kernels the call started)

    def acts(self, n):
        """Two channel-last activation buffers of at least n floats, kept between calls."""
        if self._acts[0] is None or self._acts[0].numel() < n:
            self._acts = tuple(torch.empty((max(n, 1),), dtype=torch.float32, device=self.device) for _ in range(2))
        return self._acts


def _rmline_forward_impl(prog, img, hull, dog, mask, pad, flags):
    img = _chk(img, "img")
    hull, mask = (_chk(t, n) if t is not None else None for t, n in ((hull, "hull"), (mask, "mask")))
    _chk(prog.weights, "the program's weights")
    N, Cc, H, W = img.shape
    n = len(prog.layers)
    dev = img.device
    image = torch.empty((N, 3, H, W), dtype=torch.float32, device=dev) if Cc == 4 else None
    if dog is not None:
        mask = torch.empty((N, 1, H, W), dtype=torch.float32, device=dev)
    out = torch.empty((N, prog.table[n - 1].Co, H + 2 * pad - 2 * n, W + 2 * pad - 2 * n), dtype=torch.float32, device=dev)
    need = N * (H + 2 * pad - 2) * (W + 2 * pad - 2) * prog.width if n > 1 else 0
    act0, act1 = prog.acts(need) if n > 1 else (None, None)
    st = _rmline_dog_struct(dog) if dog is not None else None
    count = C.c_int(0)
    with _on(dev):
        rc = _lib.lib().p3d_rmline_forward_f32(_p(img), N, Cc, H, W, _p(hull), C.byref(st) if st is not None else None, prog.table, n, _p(prog.weights),
                                               prog.weights.numel(), pad, flags, _p(image), _p(mask), _p(act0), _p(act1),
                                               act0.numel() if act0 is not None else 0, _p(out), C.byref(count), _stream())
    _lib.check(rc, "p3d_rmline_forward_f32")
    prog.launches = count.value
    return out, mask, (image if Cc == 4 else img)


def rmline_forward(prog, img, hull=None, dog=None, mask=None, pad=None, mask_input=True, lerp=False):
    """The whole module in ONE call into the library (p3d_rmline_forward_f32) -> (out, mask, image).
    dog given (a dict of overrides of RMLINE_DOG; {} for the wrapper's values): img [N,3|4,H,W] goes through the mask kernel first
    (len(layers) + 1 launches); `mask` must be None.  dog None: img [N,3,H,W] and the caller's mask [N,1,H,W] (len(layers) launches).
    The first layer builds stackin from image, mask (if mask_input) and hull (if the first layer takes four channels), replicate-padded by
    `pad` (default: the depth, so that the output has the input's size); lerp=True stores torch.lerp(image, out, mask), the wrapper's result.
    prog.launches receives the number of kernels the call started."""
    if not isinstance(prog, RmlineProgram):
        raise TypeError("rmline_forward: an RmlineProgram")
    img = _lpips_chk(img, "img", ndim=4)
    n = len(prog.layers)
    pad = n if pad is None else int(pad)
    if dog is not None:
        if mask is not None:
            raise ValueError("rmline_forward: dog or mask, not both")
        if img.shape[1] not in (3, 4):
            raise ValueError(f"img: shape {tuple(img.shape)}, expected 3 or 4 channels")
        dog = rmline_dog_params(dog)
    else:
        if img.shape[1] != 3:
            raise ValueError(f"img: shape {tuple(img.shape)}, expected 3 channels (an RGBA image needs the detector's composite: pass dog)")
        if mask is None and (mask_input or lerp):
            raise ValueError("rmline_forward: mask_input and lerp need a mask (or dog)")
        if mask is not None:
            mask = _lpips_chk(mask, "mask", (img.shape[0], 1) + tuple(img.shape[2:]))
    hull = _rmline_hull_chk(hull, img)
    if prog.table[0].Ci not in (3, 4) or (prog.table[0].Ci == 4 and hull is None):
        raise ValueError(f"rmline_forward: the first layer takes {prog.table[0].Ci} channels: 3, or 4 with a hull")
    if pad < 0 or img.shape[2] + 2 * pad - 2 * n < 1 or img.shape[3] + 2 * pad - 2 * n < 1:
        raise ValueError(f"rmline_forward: a {img.shape[2]} x {img.shape[3]} image padded by {pad} is too small for {n} unpadded layers")
    if lerp and (pad != n or prog.table[n - 1].Co != 3):
        raise ValueError("rmline_forward: lerp needs pad == depth and three output channels")
    flags = (_lib.P3D_RMLINE_FWD_MASK_INPUT if mask_input else 0) | (_lib.P3D_RMLINE_FWD_LERP if lerp else 0)
    return _rmline_forward_impl(prog, img, hull, dog, mask, pad, flags)


# ======================================================================================================================
# CLIP's image tower, its front end, the cosine and PSNR's reductions (include/p3d_clip.h).  Inference only.  The device
# operators are the _impl functions (which the CPU tests replace by torch stand-ins); the public forms check their arguments first.
# ======================================================================================================================
def clip_resize_plan(H, W, S):
    """p3d_clip_resize_plan (host only): dict(h, w, offy, offx, ksy, ksx, row_lo, row_hi) of clip's Resize(S) + CenterCrop(S) of an H x W image."""
    out = (C.c_int * 8)()
    rc = _lib.lib().p3d_clip_resize_plan(int(H), int(W), int(S), out)
    if rc:
        _lib.check(rc, "p3d_clip_resize_plan")
    return dict(zip(("h", "w", "offy", "offx", "ksy", "ksx", "row_lo", "row_hi"), out))


def clip_resize_table(n_in, n_out, first, count):
    """p3d_clip_resize_table (host only): PIL's fixed-point bicubic coefficients of outputs first .. first + count - 1 of one axis
    n_in -> n_out as an int32 array [count, 2 + ksize]: per output xmin, n, k[0 .. ksize)."""
    L = _lib.lib()
    scale = max(n_in / n_out, 1.0)
    ksize = int(np.ceil(2.0 * scale)) * 2 + 1
    tab = np.zeros((int(count), 2 + ksize), dtype=np.int32)
    rc = L.p3d_clip_resize_table(int(n_in), int(n_out), int(first), int(count), ksize, tab.ctypes.data_as(C.POINTER(C.c_int32)))
    if rc:
        _lib.check(rc, "p3d_clip_resize_table")
    return tab


_CLIP_TABLES, _CLIP_TABLES_MAX = {}, 8


def clip_prepare_tables(H, W, S, device):
    """(plan, tabx, taby): the resize plan and the device copies of the two coefficient tables of the S kept columns / rows, kept per
    (H, W, S, device) for the eight most recently built."""
    key = (int(H), int(W), int(S), str(device))
    if key not in _CLIP_TABLES or not memo.enabled():
        pl = clip_resize_plan(H, W, S)
        tabx = torch.from_numpy(clip_resize_table(W, pl["w"], pl["offx"], S)).to(device)
        taby = torch.from_numpy(clip_resize_table(H, pl["h"], pl["offy"], S)).to(device)
        _CLIP_TABLES.pop(key, None)
        while len(_CLIP_TABLES) >= _CLIP_TABLES_MAX:  # the oldest entry goes (an evaluation uses one source size)
            del _CLIP_TABLES[next(iter(_CLIP_TABLES))]
        _CLIP_TABLES[key] = (pl, tabx, taby)
    return _CLIP_TABLES[key]


def _clip_prepare_impl(img, S):
    img = _chk(img, "img")
    N, Cc, H, W = img.shape
    _, tabx, taby = clip_prepare_tables(H, W, S, img.device)
    L = _lib.lib()
    out = torch.empty((N, 3, S, S), dtype=torch.float32, device=img.device)
    ws = _sg_workspace(img.device, L.p3d_clip_prepare_workspace_bytes(N, H, W, S))
    with _on(img.device):
        rc = L.p3d_clip_prepare_f32(_p(img), N, Cc, H, W, S, _p(tabx), _p(taby), _p(out), _p(ws), ws.numel(), _stream())
    _lib.check(rc, "p3d_clip_prepare_f32")
    return out


def clip_prepare(img, S=224):
    """clip's _transform(S) on the device (p3d_clip_prepare_f32): img [N,C>=3,H,W] -> [N,3,S,S]: quantised to 8 bits, PIL's bicubic resize
    of the shorter side to S bit for bit, centre crop, normalisation."""
    img = _lpips_chk(img, "img", ndim=4)
    if img.shape[1] < 3:
        raise ValueError(f"img: shape {tuple(img.shape)}, expected at least three channels")
    return _clip_prepare_impl(img, int(S))


def clip_gemm_plan(M, K, Nout, force_plan=0):
    """The host-side plan of one GEMM (p3d_clip_gemm_plan, no GPU needed): dict(code, tile, split, cps, workgroups, workspace_bytes)."""
    L = _lib.lib()
    out = (C.c_int * 4)()
    code = L.p3d_clip_gemm_plan(int(M), int(K), int(Nout), int(force_plan), out)
    if code < 0:
        _lib.check(code, "p3d_clip_gemm_plan")
    return dict(code=code, tile=out[0], split=out[1], cps=out[2], workgroups=out[3],
                workspace_bytes=L.p3d_clip_gemm_workspace_bytes(int(M), int(K), int(Nout), int(force_plan)))


def _clip_gemm_impl(a, w, bias, res, gelu, patch, force_plan, out=None):
    a, w = _chk(a, "a"), _chk(w, "w")
    bias = _chk(bias, "bias") if bias is not None else None
    res = _chk(res, "res") if res is not None else None
    K, Nout = w.shape
    if patch:
        N, S = a.shape[0], a.shape[2]
        M, flags = N * (S // patch) ** 2, _lib.P3D_CLIP_PATCH
    else:
        N, S, M, flags = 0, 0, a.shape[0], 0
    if gelu:
        flags |= _lib.P3D_CLIP_GELU
    L = _lib.lib()
    if out is None:
        out = torch.empty((M, Nout), dtype=torch.float32, device=a.device)
    ws = _sg_workspace(a.device, L.p3d_clip_gemm_workspace_bytes(M, K, Nout, force_plan))
    with _on(a.device):
        rc = L.p3d_clip_gemm_f32(_p(a), M, K, _p(w), Nout, _p(bias), _p(res), flags, N, S, patch, _p(out), force_plan, _p(ws), ws.numel(), _stream())
    _lib.check(rc, "p3d_clip_gemm_f32")
    return out


def clip_gemm(a, w, bias=None, res=None, gelu=False, patch=0, force_plan=0, inplace=False):
    """epi(a @ w) (p3d_clip_gemm_f32): a [M,K], or with patch > 0 an image [N,3,S,S] read as flattened patches (K = 3 patch^2); w [K,Nout];
    bias [Nout]; gelu: QuickGELU; res [M,Nout] is added last (inplace=True writes the result over res).  force_plan: 0 chooses, else
    (tile << 8) | split (clip_gemm_plan)."""
    patch = int(patch)
    if patch:
        a = _lpips_chk(a, "a", ndim=4)
        if patch < 1 or a.shape[1] != 3 or a.shape[2] != a.shape[3] or a.shape[2] % patch:
            raise ValueError(f"a: shape {tuple(a.shape)}, expected [N,3,S,S] with S a multiple of the patch {patch}")
        M, K = a.shape[0] * (a.shape[2] // patch) ** 2, 3 * patch * patch
    else:
        a = _lpips_chk(a, "a", ndim=2)
        M, K = a.shape
    w = _lpips_chk(w, "w", (K, w.shape[1] if isinstance(w, torch.Tensor) and w.ndim == 2 else -1))
    if bias is not None:
        bias = _lpips_chk(bias, "bias", (w.shape[1],))
    if res is not None:
        res = _lpips_chk(res, "res", (M, w.shape[1]))
    return _clip_gemm_impl(a, w, bias, res, bool(gelu), patch, int(force_plan), out=res if inplace and res is not None else None)


def _clip_layernorm_impl(x, rows, D, ld, gamma, beta, eps):
    x, gamma, beta = _chk(x, "x"), _chk(gamma, "gamma"), _chk(beta, "beta")
    y = torch.empty((rows, D), dtype=torch.float32, device=x.device)
    with _on(x.device):
        rc = _lib.lib().p3d_clip_layernorm_f32(_p(x), rows, D, ld, _p(gamma), _p(beta), eps, _p(y), _stream())
    _lib.check(rc, "p3d_clip_layernorm_f32")
    return y


def clip_layernorm(x, gamma, beta, eps=1e-5, rows=None, ld=None):
    """LayerNorm of the rows of x [M,D] (p3d_clip_layernorm_f32).  rows / ld: normalise `rows` rows that start every `ld` floats of x's
    storage instead (ld = T * D with rows = N: the class token of each image)."""
    x = _lpips_chk(x, "x", ndim=2)
    D = x.shape[1]
    gamma, beta = _lpips_chk(gamma, "gamma", (D,)), _lpips_chk(beta, "beta", (D,))
    rows, ld = (x.shape[0] if rows is None else int(rows)), (D if ld is None else int(ld))
    if rows < 1 or ld < D or (rows - 1) * ld + D > x.numel():
        raise ValueError(f"clip_layernorm: {rows} rows every {ld} floats do not fit x {tuple(x.shape)}")
    return _clip_layernorm_impl(x, rows, D, ld, gamma, beta, float(eps))


def _clip_embed_impl(patches, cls, pos, N, gamma, beta, eps):
    patches, cls, pos, gamma, beta = (_chk(t, n) for t, n in ((patches, "patches"), (cls, "cls"), (pos, "pos"), (gamma, "gamma"), (beta, "beta")))
    T, D = pos.shape
    y = torch.empty((N * T, D), dtype=torch.float32, device=pos.device)
    with _on(pos.device):
        rc = _lib.lib().p3d_clip_embed_f32(_p(patches), _p(cls), _p(pos), N, T, D, _p(gamma), _p(beta), eps, _p(y), _stream())
    _lib.check(rc, "p3d_clip_embed_f32")
    return y


def clip_embed(patches, cls, pos, gamma, beta, eps=1e-5):
    """The embedding step (p3d_clip_embed_f32): patches [N (T-1), D] (the patch GEMM's rows), cls [D], pos [T,D] -> ln_pre of
    [cls | patches] + pos, [N T, D]."""
    pos = _lpips_chk(pos, "pos", ndim=2)
    T, D = pos.shape
    patches = _lpips_chk(patches, "patches", ndim=2)
    if T < 2 or patches.shape[1] != D or patches.shape[0] % (T - 1):
        raise ValueError(f"patches: shape {tuple(patches.shape)}, expected [N * {T - 1}, {D}]")
    cls, gamma, beta = _lpips_chk(cls, "cls", (D,)), _lpips_chk(gamma, "gamma", (D,)), _lpips_chk(beta, "beta", (D,))
    return _clip_embed_impl(patches, cls, pos, patches.shape[0] // (T - 1), gamma, beta, float(eps))


def clip_attention_plan(N, T, heads):
    """p3d_clip_attention_plan: dict(workgroups, qblocks, rows, lds_bytes)."""
    out = (C.c_int * 4)()
    rc = _lib.lib().p3d_clip_attention_plan(int(N), int(T), int(heads), out)
    if rc:
        _lib.check(rc, "p3d_clip_attention_plan")
    return dict(zip(("workgroups", "qblocks", "rows", "lds_bytes"), out))


def _clip_attention_impl(qkv, N, T, heads):
    qkv = _chk(qkv, "qkv")
    D = qkv.shape[1] // 3
    out = torch.empty((N * T, D), dtype=torch.float32, device=qkv.device)
    with _on(qkv.device):
        rc = _lib.lib().p3d_clip_attention_f32(_p(qkv), N, T, heads, D, _p(out), _stream())
    _lib.check(rc, "p3d_clip_attention_f32")
    return out


def clip_attention(qkv, N, T, heads):
    """Softmax attention (p3d_clip_attention_f32): qkv [N T, 3 D], columns q | k | v, head h the columns 64 h .. 64 h + 63 of each ->
    [N T, D].  D = 64 heads and T <= 64."""
    N, T, heads = int(N), int(T), int(heads)
    qkv = _lpips_chk(qkv, "qkv", ndim=2)
    if N < 1 or T < 1 or heads < 1 or qkv.shape[0] != N * T or qkv.shape[1] % 3:
        raise ValueError(f"qkv: shape {tuple(qkv.shape)}, expected [{N} * {T}, 3 D]")
    if qkv.shape[1] != 3 * 64 * heads or T > _lib.P3D_CLIP_MAX_T:
        raise ValueError(f"clip_attention: D = {qkv.shape[1] // 3} must be 64 * heads ({heads}) and T = {T} at most {_lib.P3D_CLIP_MAX_T}")
    return _clip_attention_impl(qkv, N, T, heads)


def _clip_cosine_impl(a, b):
    a, b = _chk(a, "a"), _chk(b, "b")
    sim = torch.empty((a.shape[0],), dtype=torch.float32, device=a.device)
    with _on(a.device):
        rc = _lib.lib().p3d_clip_cosine_f32(_p(a), _p(b), a.shape[0], a.shape[1], _p(sim), _stream())
    _lib.check(rc, "p3d_clip_cosine_f32")
    return sim


def clip_cosine(a, b):
    """measure.py:42 per pair (p3d_clip_cosine_f32): a, b [pairs, D] -> [pairs], row i of a against row i of b."""
    a = _lpips_chk(a, "a", ndim=2)
    b = _lpips_chk(b, "b", tuple(a.shape))
    if a.numel() == 0:
        raise ValueError("clip_cosine: no pairs")
    return _clip_cosine_impl(a, b)


def _psnr_sums_impl(pred, target):
    pred, target = _chk(pred, "pred"), _chk(target, "target")
    L = _lib.lib()
    out = torch.empty((3,), dtype=torch.float32, device=pred.device)
    ws = _sg_workspace(pred.device, L.p3d_psnr_workspace_bytes(pred.numel()))
    with _on(pred.device):
        rc = L.p3d_psnr_f32(_p(pred), _p(target), pred.numel(), _p(out), _p(ws), ws.numel(), _stream())
    _lib.check(rc, "p3d_psnr_f32")
    return out


def psnr_sums(pred, target):
    """PSNR's three reductions in one pass (p3d_psnr_f32): a device tensor [sum (pred - target)^2, min target, max target]."""
    pred = _chk(pred, "pred")
    target = _lpips_chk(target, "target", tuple(pred.shape))
    if pred.numel() == 0:
        raise ValueError("psnr_sums: empty input")
    return _psnr_sums_impl(pred, target)


class ClipProgram:
    """A whole image tower as p3d_clip_forward_f32 takes it: the table of step records over ONE weight blob (the caller's: records carry
    offsets into it) and an activation arena.  records: dicts with kind ('prepare' | 'gemm' | 'layernorm' | 'embed' | 'attention'), src / dst
    / res (buffer indices, res None), the sizes of the kind, and the offsets w, b (b None: no bias), w2, b2.  buf_len: floats per buffer."""
    KINDS = {"prepare": _lib.P3D_CLIP_KIND_PREPARE, "gemm": _lib.P3D_CLIP_KIND_GEMM, "layernorm": _lib.P3D_CLIP_KIND_LAYERNORM,
             "embed": _lib.P3D_CLIP_KIND_EMBED, "attention": _lib.P3D_CLIP_KIND_ATTENTION}

    def __init__(self, records, buf_len, weights):
        self.records, self.weights, self.device = list(records), weights, weights.device
        self.table = (_lib.ClipStep * len(self.records))()
        for t, r in zip(self.table, self.records):
            t.kind = self.KINDS[r["kind"]]
            for name in ("M", "K", "Nout", "N", "T", "heads", "S", "patch", "H", "W", "ld", "plan"):
                setattr(t, name, int(r.get(name, 0)))
            t.in_, t.out, t.res = r["src"], r["dst"], -1 if r.get("res") is None else r["res"]
            t.flags = (_lib.P3D_CLIP_GELU if r.get("gelu") else 0) | (_lib.P3D_CLIP_PATCH if r.get("patch") else 0)
            t.eps = float(r.get("eps", 0.0))
            t.w_off, t.w2_off, t.b2_off = int(r.get("w", 0)), int(r.get("w2", 0)), int(r.get("b2", 0))
            t.b_off = (-1 if r["kind"] == "gemm" else 0) if r.get("b") is None else int(r["b"])
        self.n_bufs = len(buf_len)
        self.buf_len = (C.c_int64 * self.n_bufs)(*[int(n) for n in buf_len])
        offs, at = [], 0
        for n in buf_len:
            offs.append(at)
            at += (int(n) + 63) // 64 * 64  # every buffer starts on a 256-byte boundary
        self.buf_off = (C.c_int64 * self.n_bufs)(*offs)
        self.arena = torch.empty((max(at, 1),), dtype=torch.float32, device=self.device)
        self.launches = sum(2 if r["kind"] == "prepare" else 1 for r in self.records)  # (+ one per split-K reduction: see clip.py)

    def buffer(self, b, shape):
        n = 1
        for s in shape:
            n *= int(s)
        return self.arena[self.buf_off[b]:self.buf_off[b] + n].view(*shape)


def _clip_forward_impl(prog):
    _chk(prog.arena, "the program's arena"), _chk(prog.weights, "the program's weights")
    L = _lib.lib()
    ws = _sg_workspace(prog.device, L.p3d_clip_workspace_bytes(prog.table, len(prog.records)))
    with _on(prog.device):
        rc = L.p3d_clip_forward_f32(prog.table, len(prog.records), _p(prog.weights), prog.weights.numel(), _p(prog.arena), prog.arena.numel(),
                                    prog.buf_off, prog.buf_len, prog.n_bufs, _p(ws), ws.numel(), _stream())
    _lib.check(rc, "p3d_clip_forward_f32")


def clip_forward(prog, x, src=0):
    """Run a whole ClipProgram in ONE call into the library: x is copied into buffer `src` of the arena, every step is launched on the
    current stream; the results are read with prog.buffer(index, shape) (views of the arena: clone what has to outlive the next call)."""
    if not isinstance(prog, ClipProgram):
        raise TypeError("clip_forward: a ClipProgram")
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.device != prog.arena.device:
        raise RuntimeError(f"x must be a torch.float32 tensor on {prog.arena.device}")
    if x.numel() != prog.buf_len[src]:
        raise ValueError(f"x: {x.numel()} values, the program was built for {prog.buf_len[src]}")
    prog.arena[prog.buf_off[src]:prog.buf_off[src] + x.numel()].copy_(x.reshape(-1))
    _clip_forward_impl(prog)
    return prog


# ------------------------------------------------------------------------------------------------------------------------------------------
# The illustration-to-render module's TRAINING operators (include/p3d_rmline_grad.h): batch statistics, the device-side
# fold of a train-mode batch norm, the data gradient, the weight / bias gradient, the batch norm's backward coefficients and the head;
# and the two autograd Functions that rmline_train.RMLineModel composes them with.  binary32, fixed sum orders, no atomics, no host sync.
_RMLINE_WS = {}


def _rmline_ws(device, floats):
    """One float32 workspace per (device, current stream), grown on demand: the launches that share one are ordered on that stream, and
    operators issued on another stream get a workspace of their own."""
    with _on(device):
        key = (device, _raw_stream(_cur_device()))
    ws = _RMLINE_WS.get(key)
    if ws is None or ws.numel() < floats:
        ws = _RMLINE_WS[key] = torch.empty(max(int(floats), 1 << 16), dtype=torch.float32, device=device)
    return ws


def _rmline_c(n, name):
    if not 1 <= n <= _lib.P3D_RMLINE_MAX_C:
        raise ValueError(f"{name}: {n} channels, 1..{_lib.P3D_RMLINE_MAX_C}")
    return int(n)


def _rmline_aligned(t):
    return t.clone() if t.data_ptr() % 16 else t  # (a view into a larger tensor: channel-last tensors move in 16-byte vectors)


def rmline_bn_stats(x, running_mean=None, running_var=None, counter=None, momentum=0.1):
    """(mean [C], biased var [C]) of a channel-last activation x [..., C] over all other axes by a centred algorithm
    (p3d_rmline_bn_stats_f32, two launches).  With running_mean, running_var (float32 [C]) and counter (int64 scalar tensor), all three
    or none: running <- (1 - momentum) running + momentum batch in place, the variance unbiased, and counter += 1 — torch's
    BatchNorm2d in train mode.  One value per channel: ValueError, as torch raises, before any launch."""
    x = _chk(x, "x")
    if x.ndim < 2:
        raise ValueError(f"x: shape {tuple(x.shape)}, expected [..., C]")
    Cc = _rmline_c(x.shape[-1], "x")
    K = x.numel() // Cc
    if K <= 1:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(x.shape)}")
    given = [t is not None for t in (running_mean, running_var, counter)]
    if any(given) and not all(given):
        raise ValueError("rmline_bn_stats: running_mean, running_var and counter come together")
    if all(given):
        running_mean, running_var = _lpips_chk(running_mean, "running_mean", (Cc,)), _lpips_chk(running_var, "running_var", (Cc,))
        counter = _chk(counter, "counter", torch.int64)
        if counter.numel() != 1:
            raise ValueError("counter: one int64")
    if not 0.0 <= float(momentum) <= 1.0:
        raise ValueError("momentum: 0..1")
    x = _rmline_aligned(x)
    mean, var = torch.empty(Cc, dtype=torch.float32, device=x.device), torch.empty(Cc, dtype=torch.float32, device=x.device)
    ws = _rmline_ws(x.device, _lib.P3D_RMLINE_BN_MAX_GROUPS * 4 * 64)
    with _on(x.device):
        rc = _lib.lib().p3d_rmline_bn_stats_f32(_p(x), K, Cc, float(momentum), _p(mean), _p(var), _p(running_mean), _p(running_var), _p(counter),
                                                _p(ws), ws.numel(), _stream())
    _lib.check(rc, "p3d_rmline_bn_stats_f32")
    RMLINE_LAUNCHES[0] += 2
    return mean, var


def rmline_bn_fold(w, bias, bn=None):
    """A layer's operands (wk [9,Ci,Co], bias [Co]) from torch's w [Co,Ci,3,3] and bias, ONE launch (p3d_rmline_bn_fold_f32).
    bn = (gamma, beta, mean, var, eps) of the batch norm IN FRONT of the convolution folds it in: wk = w s, bias + sum of w (beta - mean s),
    s = gamma / sqrt(var + eps), in binary32 on the device; None: a re-layout only."""
    w = _lpips_chk(w, "w", ndim=4)
    Co, Ci = _rmline_c(w.shape[0], "w"), _rmline_c(w.shape[1], "w")
    if tuple(w.shape[2:]) != (3, 3):
        raise ValueError(f"w: shape {tuple(w.shape)}, expected (Co, Ci, 3, 3)")
    bias = _lpips_chk(bias, "bias", (Co,))
    gamma = beta = mean = var = None
    eps = 0.0
    if bn is not None:
        gamma, beta, mean, var, eps = bn
        gamma, beta, mean, var = (_lpips_chk(t, n, (Ci,)) for t, n in ((gamma, "gamma"), (beta, "beta"), (mean, "mean"), (var, "var")))
        if not eps >= 0.0:
            raise ValueError("eps: not negative")
    wk, bf = torch.empty((9, Ci, Co), dtype=torch.float32, device=w.device), torch.empty(Co, dtype=torch.float32, device=w.device)
    with _on(w.device):
        rc = _lib.lib().p3d_rmline_bn_fold_f32(_p(w), _p(bias), _p(gamma), _p(beta), _p(mean), _p(var), float(eps), Ci, Co, _p(wk), _p(bf), _stream())
    _lib.check(rc, "p3d_rmline_bn_fold_f32")
    RMLINE_LAUNCHES[0] += 1
    return wk, bf


def rmline_conv_dgrad(g, wk, a=None, c0=None, c1=None, slope=0.01, planar=False):
    """The data gradient of one unpadded 3 x 3 layer, ONE launch (p3d_rmline_conv_dgrad_f32): g [N,Hg,Wg,Co] channel-last and the layer's
    own wk [9,Ci,Co] -> dx [N,Hg+2,Wg+2,Ci] (planar=True: [N,Ci,Hg+2,Wg+2]), the full correlation.  With a [N,Hg+2,Wg+2,Ci] (the
    post-activation map of the layer below) the store gives (dx + c0 + c1 a) (a > 0 ? 1 : slope): that layer's pre-activation gradient,
    c0 / c1 [Ci] from rmline_bn_coef (both or neither).  slope <= 0 with a: ValueError."""
    g = _lpips_chk(g, "g", ndim=4)
    wk = _lpips_chk(wk, "wk", ndim=3)
    Ci, Co = _rmline_c(wk.shape[1], "wk"), _rmline_c(wk.shape[2], "wk")
    if wk.shape[0] != 9 or g.shape[3] != Co:
        raise ValueError(f"rmline_conv_dgrad: g {tuple(g.shape)} and wk {tuple(wk.shape)} do not fit (g channel-last with Co channels, wk (9, Ci, Co))")
    N, Hg, Wg = g.shape[:3]
    if (c0 is None) != (c1 is None) or (c0 is not None and a is None):
        raise ValueError("rmline_conv_dgrad: c0 and c1 come together, and with a")
    if a is not None:
        a = _rmline_aligned(_lpips_chk(a, "a", (N, Hg + 2, Wg + 2, Ci)))
        if not (slope > 0.0 and math.isfinite(slope)):
            raise ValueError("slope: positive (the sign of a must be its pre-activation's)")
        if c0 is not None:
            c0, c1 = _lpips_chk(c0, "c0", (Ci,)), _lpips_chk(c1, "c1", (Ci,))
    g = _rmline_aligned(g)
    out = torch.empty((N, Ci, Hg + 2, Wg + 2) if planar else (N, Hg + 2, Wg + 2, Ci), dtype=torch.float32, device=g.device)
    with _on(g.device):
        rc = _lib.lib().p3d_rmline_conv_dgrad_f32(_p(g), N, Hg, Wg, Co, _p(wk), Ci, _p(a), _p(c0), _p(c1), float(slope),
                                                  _lib.P3D_RMLINE_OUT_PLANAR if planar else 0, _p(out), _stream())
    _lib.check(rc, "p3d_rmline_conv_dgrad_f32")
    RMLINE_LAUNCHES[0] += 1
    return out


def rmline_wgrad_plan(N, Ci, Co, force_slices=0):
    """The host-side plan of a weight gradient (p3d_rmline_wgrad_plan, no GPU needed): dict(slices, sets, lds_bytes, ws_floats).
    ValueError for sizes the kernel refuses or force_slices outside 1..min(N, 512)."""
    out = (C.c_int64 * 4)()
    rc = _lib.lib().p3d_rmline_wgrad_plan(int(N), int(Ci), int(Co), int(force_slices), out)
    if rc < 0:
        raise ValueError(f"rmline_wgrad_plan: N {N}, Ci {Ci}, Co {Co} (1..{_lib.P3D_RMLINE_MAX_C}), force_slices {force_slices} "
                         f"(0 chooses; at most min(N, {_lib.P3D_RMLINE_WG_MAX_SLICES}))")
    return dict(slices=int(out[0]), sets=int(out[1]), lds_bytes=int(out[2]), ws_floats=int(out[3]))


def rmline_conv_wgrad(x, dz, stack=None, pad=0, force_slices=0, oihw=False):
    """(dw, dbias) of one unpadded 3 x 3 layer, TWO launches (p3d_rmline_conv_wgrad_f32): x [N,Hin,Win,Ci] channel-last (or, with x None,
    stack=(image, mask or None, hull or None) and pad as rmline_conv builds the first layer's input in the load) and dz [N,Hin-2,Win-2,Co]
    -> dw [9,Ci,Co] (oihw=True: [Co,Ci,3,3], torch's layout) and dbias [Co].  force_slices: the number of patch slices (0: the plan's)."""
    dz = _lpips_chk(dz, "dz", ndim=4)
    Co = _rmline_c(dz.shape[3], "dz")
    pad, flags = int(pad), _lib.P3D_RMLINE_OUT_OIHW if oihw else 0
    image = mask = hull = None
    if stack is not None:
        if x is not None:
            raise ValueError("rmline_conv_wgrad: x or stack, not both")
        image, mask, hull = stack
        image = _lpips_chk(image, "image", ndim=4)
        if image.shape[1] != 3 or pad < 0:
            raise ValueError(f"image: shape {tuple(image.shape)}, expected three channels; pad not negative")
        mask = _lpips_chk(mask, "mask", (image.shape[0], 1) + tuple(image.shape[2:])) if mask is not None else None
        hull = _rmline_hull_chk(hull, image)
        Ci = 3 + (hull is not None)
        N, Hin, Win = image.shape[0], image.shape[2] + 2 * pad, image.shape[3] + 2 * pad
        flags |= _lib.P3D_RMLINE_IN_STACK
    else:
        x = _rmline_aligned(_lpips_chk(x, "x", ndim=4))
        Ci = _rmline_c(x.shape[3], "x")
        if pad != 0:
            raise ValueError("pad: only with stack")
        N, Hin, Win = x.shape[:3]
    if Hin < 3 or Win < 3 or tuple(dz.shape) != (N, Hin - 2, Win - 2, Co):
        raise ValueError(f"rmline_conv_wgrad: dz {tuple(dz.shape)} for an input of {N} x {Hin} x {Win}")
    plan = rmline_wgrad_plan(N, Ci, Co, force_slices)
    dz = _rmline_aligned(dz)
    dw = torch.empty((Co, Ci, 3, 3) if oihw else (9, Ci, Co), dtype=torch.float32, device=dz.device)
    db = torch.empty(Co, dtype=torch.float32, device=dz.device)
    ws = _rmline_ws(dz.device, plan["ws_floats"])
    with _on(dz.device):
        rc = _lib.lib().p3d_rmline_conv_wgrad_f32(_p(x), _p(image), _p(mask), _p(hull), N, Hin, Win, pad, Ci, _p(dz), Co, flags, int(force_slices),
                                                  _p(dw), _p(db), _p(ws), ws.numel(), _stream())
    _lib.check(rc, "p3d_rmline_conv_wgrad_f32")
    RMLINE_LAUNCHES[0] += 2
    return dw, db


def rmline_bn_coef(dwk_f, db_f, w, gamma, beta, mean, var, eps, K, want_dw=True, want_affine=True):
    """The backward of the batch norm folded into a layer, ONE launch (p3d_rmline_bn_coef_f32) -> (dgamma, dbeta, dw, c0, c1): from the
    FOLDED operands' gradients dwk_f [9,Ci,Co], db_f [Co], the raw w [Co,Ci,3,3] and the batch norm's gamma, beta, mean, var [Ci], eps and count
    K.  dw [Co,Ci,3,3] is the raw weight's gradient; c0, c1 [Ci] are what rmline_conv_dgrad's store adds.  dgamma / dbeta (want_affine)
    and dw (want_dw) are None when not wanted."""
    dwk_f = _lpips_chk(dwk_f, "dwk_f", ndim=3)
    Ci, Co = _rmline_c(dwk_f.shape[1], "dwk_f"), _rmline_c(dwk_f.shape[2], "dwk_f")
    if dwk_f.shape[0] != 9:
        raise ValueError(f"dwk_f: shape {tuple(dwk_f.shape)}, expected (9, Ci, Co)")
    db_f, w = _lpips_chk(db_f, "db_f", (Co,)), _lpips_chk(w, "w", (Co, Ci, 3, 3))
    gamma, beta, mean, var = (_lpips_chk(t, n, (Ci,)) for t, n in ((gamma, "gamma"), (beta, "beta"), (mean, "mean"), (var, "var")))
    if int(K) <= 1 or not eps >= 0.0:
        raise ValueError("rmline_bn_coef: K > 1 and eps >= 0")
    dev = w.device
    dgamma, dbeta = (torch.empty(Ci, dtype=torch.float32, device=dev), torch.empty(Ci, dtype=torch.float32, device=dev)) if want_affine else (None, None)
    dw = torch.empty((Co, Ci, 3, 3), dtype=torch.float32, device=dev) if want_dw else None
    c0, c1 = torch.empty(Ci, dtype=torch.float32, device=dev), torch.empty(Ci, dtype=torch.float32, device=dev)
    with _on(dev):
        rc = _lib.lib().p3d_rmline_bn_coef_f32(_p(dwk_f), _p(db_f), _p(w), _p(gamma), _p(beta), _p(mean), _p(var), float(eps), int(K), Ci, Co, _p(dgamma), _p(dbeta),
                                               _p(dw), _p(c0), _p(c1), _stream())
    _lib.check(rc, "p3d_rmline_bn_coef_f32")
    RMLINE_LAUNCHES[0] += 1
    return dgamma, dbeta, dw, c0, c1


def rmline_head(t, image, mask, hull=None, crop=0):
    """The head of the loss, ONE launch (p3d_rmline_head_f32): t, image [N,3,H,W], mask [N,1,H,W] -> (img = torch.lerp(image, t, mask),
    loss_l1 [N] = mean |img - image|, crop_img, crop_hull).  crop > 0: the centre window of img ([N,3,H-2crop,W-2crop]) and of hull
    [N,1,H,W] (None: no crop_hull) — the discriminator's input; crop = 0: both None."""
    t = _lpips_chk(t, "t", ndim=4)
    N, Cc, H, W = t.shape
    if Cc != 3:
        raise ValueError(f"t: shape {tuple(t.shape)}, expected three channels")
    image, mask = _lpips_chk(image, "image", (N, 3, H, W)), _lpips_chk(mask, "mask", (N, 1, H, W))
    hull = _rmline_hull_chk(hull, image)
    crop = int(crop)
    if crop < 0 or H - 2 * crop < 1 or W - 2 * crop < 1:
        raise ValueError(f"crop: {crop} of a {H} x {W} map")
    dev = t.device
    img, l1 = torch.empty_like(t), torch.empty(N, dtype=torch.float32, device=dev)
    ci = torch.empty((N, 3, H - 2 * crop, W - 2 * crop), dtype=torch.float32, device=dev) if crop else None
    ch = torch.empty((N, 1, H - 2 * crop, W - 2 * crop), dtype=torch.float32, device=dev) if crop and hull is not None else None
    with _on(dev):
        rc = _lib.lib().p3d_rmline_head_f32(_p(t), _p(image), _p(mask), _p(hull), N, H, W, crop, _p(img), _p(l1), _p(ci), _p(ch), _stream())
    _lib.check(rc, "p3d_rmline_head_f32")
    RMLINE_LAUNCHES[0] += 1
    return img, l1, ci, ch


def rmline_head_grad(t, img, image, mask, g_l1, d, crop=0, shape=None):
    """The head's backward, ONE launch (p3d_rmline_head_grad_f32) -> [N,H,W,3] channel-last:
    f m (g_l1[n] sign(img - image) / (3 H W) + d inside the centre window), f = 1 - t^2 (t None: 1), m = mask (None: 1).
    g_l1 [N] or None (no L1 term); d [N,3,H-2crop,W-2crop] in ANY strides, or None.  shape = (N, H, W) when neither t nor img says it."""
    ref = t if t is not None else (img if img is not None else None)
    if ref is not None:
        N, H, W = ref.shape[0], ref.shape[2], ref.shape[3]
    else:
        N, H, W = shape
    crop = int(crop)
    t = _lpips_chk(t, "t", (N, 3, H, W)) if t is not None else None
    mask = _lpips_chk(mask, "mask", (N, 1, H, W)) if mask is not None else None
    if g_l1 is not None:
        g_l1, img, image = _lpips_chk(g_l1, "g_l1", (N,)), _lpips_chk(img, "img", (N, 3, H, W)), _lpips_chk(image, "image", (N, 3, H, W))
    ds = None
    if d is not None:
        if not d.is_cuda or d.dtype != torch.float32 or tuple(d.shape) != (N, 3, H - 2 * crop, W - 2 * crop):
            raise ValueError(f"d: a float32 device tensor of shape {(N, 3, H - 2 * crop, W - 2 * crop)}")
        ds = (C.c_int64 * 4)(*d.stride())
    out = torch.empty((N, H, W, 3), dtype=torch.float32, device=(t if t is not None else (d if d is not None else img)).device)
    with _on(out.device):
        rc = _lib.lib().p3d_rmline_head_grad_f32(_p(t), _p(img if g_l1 is not None else None), _p(image if g_l1 is not None else None), _p(mask),
                                                 _p(g_l1), _p(d), ds, N, H, W, crop, _p(out), _stream())
    _lib.check(rc, "p3d_rmline_head_grad_f32")
    RMLINE_LAUNCHES[0] += 1
    return out


class RmlineStackFunction(torch.autograd.Function):
    """One pass through a stack of unpadded 3 x 3 convolutions in TRAIN mode — the generator or the discriminator of rmlineganA.py:65-100:
    LeakyReLU and a batch norm with THIS call's statistics after every convolution but the last.

    apply(spec, image, mask, hull, *params): the first layer reads the stack of image * (1 - mask) and hull built in the load; params =
    (w_0, b_0, gamma_0, beta_0, w_1, b_1, ..., w_last, b_last); spec = dict(pad, slope, last_act 'tanh' | 'none', planar, bns: the
    BatchNorm2d modules, whose running statistics and counters are updated in place).  Returns the last layer's output, planar
    [N,Co,H,W] (spec['planar']) or channel-last.  Each batch norm is folded into the NEXT convolution on the device (rmline_bn_fold),
    so the forward is rmline_conv's kernel (with per-tap chains); the post-activation map of every layer is kept.

    backward: per layer from the last, wgrad (of the folded operands) -> coefficients (rmline_bn_coef: the batch norm's parameter
    gradients, the raw weight's, and c0 / c1) -> dgrad, whose store turns the input gradient into the pre-activation gradient of the
    layer below.  A layer's wgrad also runs when its own parameters want no gradient but a batch norm stands in front of it: that batch
    norm's backward needs the sums.  Only `image` and the parameters get gradients."""

    @staticmethod
    def forward(ctx, spec, image, mask, hull, *params):
        bns, L = spec["bns"], (len(params) + 2) // 4
        if len(params) != 4 * L - 2 or len(bns) != L - 1:
            raise ValueError("RmlineStackFunction: params are (w, b, gamma, beta) per layer, without the last layer's batch norm")
        acts, stats, folded, x = [], [], [], None
        for l in range(L):
            w, b = params[4 * l], params[4 * l + 1]
            bn = None
            if l > 0:
                m = bns[l - 1]
                bn = (params[4 * l - 2].detach(), params[4 * l - 1].detach(), stats[l - 1][0], stats[l - 1][1], float(m.eps))
            wk, bf = rmline_bn_fold(w.detach(), b.detach(), bn)
            last = l == L - 1
            x = rmline_conv(x, wk, bf, act=spec["last_act"] if last else "leaky", slope=spec["slope"], stack=(image, mask, hull) if l == 0 else None,
                            pad=spec["pad"] if l == 0 else 0, planar=last and spec["planar"], per_tap=True)
            folded.append(wk)
            if not last:
                m = bns[l]
                if m.momentum is None:
                    raise NotImplementedError("BatchNorm2d(momentum=None): the cumulative average is not built")
                track = m.track_running_stats and m.running_mean is not None
                stats.append(rmline_bn_stats(x, m.running_mean if track else None, m.running_var if track else None,
                                             m.num_batches_tracked if track else None, float(m.momentum)))
                acts.append(x)
        # every tensor through save_for_backward, the output included: an attribute of the ctx would tie the output to its own grad_fn
        # in a reference cycle and keep a pass's activations alive until the cyclic collector runs
        ctx.spec, ctx.L = spec, L
        ctx.save_for_backward(image, mask, hull, x, *params, *folded, *acts, *[m for m, _ in stats], *[v for _, v in stats])
        return x

    @staticmethod
    def backward(ctx, dout):
        spec, L = ctx.spec, ctx.L
        saved = list(ctx.saved_tensors)
        image, mask, hull, out = saved[:4]
        at = [4]

        def take(n):
            at[0] += n
            return saved[at[0] - n:at[0]]
        params, folded, acts = [p.detach() for p in take(4 * L - 2)], take(L), take(L - 1)
        stats = list(zip(take(L - 1), take(L - 1)))
        need = ctx.needs_input_grad  # (spec, image, mask, hull, *params)
        if spec["last_act"] == "tanh":  # (1 - t^2) d, planar -> channel-last, in one launch
            dz = rmline_head_grad(out, None, None, None, None, dout, 0)
        else:
            dz = dout.contiguous() if not spec["planar"] else dout.permute(0, 2, 3, 1).contiguous()
        grads, dimage = [None] * len(params), None
        lowest = min([l for l in range(L) if any(need[4 + 4 * l + j] for j in range(4) if 4 * l + j < len(params))] or [L])
        for l in reversed(range(L)):
            if l < lowest and not need[1]:
                break
            w = params[4 * l]
            want_w = need[4 + 4 * l] or need[4 + 4 * l + 1]
            if want_w or l > 0:
                dw, db = rmline_conv_wgrad(acts[l - 1] if l > 0 else None, dz, stack=(image, mask, hull) if l == 0 else None,
                                           pad=spec["pad"] if l == 0 else 0, oihw=l == 0)
            if l > 0:
                want_affine = need[4 + 4 * l - 2] or need[4 + 4 * l - 1]
                K = acts[l - 1].numel() // acts[l - 1].shape[-1]
                dgamma, dbeta, dw, c0, c1 = rmline_bn_coef(dw, db, w, params[4 * l - 2], params[4 * l - 1], stats[l - 1][0], stats[l - 1][1], float(spec["bns"][l - 1].eps), K,
                                                           want_dw=want_w, want_affine=want_affine)
                if want_affine:
                    grads[4 * l - 2], grads[4 * l - 1] = dgamma, dbeta
                dz = rmline_conv_dgrad(dz, folded[l], a=acts[l - 1], c0=c0, c1=c1, slope=spec["slope"])
            elif need[1]:
                dimage = rmline_conv_dgrad(dz, folded[0], planar=True)[:, :3]
            if want_w:
                grads[4 * l], grads[4 * l + 1] = dw, db
        return (None, dimage, None, None) + tuple(g if need[4 + i] else None for i, g in enumerate(grads))


class RmlineHeadFunction(torch.autograd.Function):
    """The head of rmlineganA.loss (rmlineganA.py:178-187): apply(t, image, mask, hull, crop) -> (img, loss_l1 [N], crop_img, crop_hull)
    as rmline_head gives them.  Gradients reach t only, from loss_l1 and crop_img (img itself is marked non-differentiable: the
    reference's loss uses it through these two alone); t's gradient is handed over in channel-last memory."""

    @staticmethod
    def forward(ctx, t, image, mask, hull, crop):
        img, l1, ci, ch = rmline_head(t.detach(), image, mask, hull, crop)
        ctx.save_for_backward(img, image, mask)
        ctx.crop = int(crop)
        ctx.set_materialize_grads(False)
        outs = (img, l1, ci, ch)
        ctx.mark_non_differentiable(*[o for o in (img, ch) if o is not None])
        return outs

    @staticmethod
    def backward(ctx, _dimg, g_l1, d_crop, _dhull):
        img, image, mask = ctx.saved_tensors
        if g_l1 is None and d_crop is None:
            return None, None, None, None, None
        out = rmline_head_grad(None, img, image, mask, g_l1.contiguous() if g_l1 is not None else None, d_crop, ctx.crop,
                               shape=(img.shape[0], img.shape[2], img.shape[3]))
        return out.permute(0, 3, 1, 2), None, None, None, None


# ---- the augmentation pipe's operator (include/p3d_augment.h) ---------------------------------------------------------
AUGMENT_PLANS = {None: _lib.P3D_AUG_PLAN_AUTO, "auto": _lib.P3D_AUG_PLAN_AUTO, "tile": _lib.P3D_AUG_PLAN_TILE, "staged": _lib.P3D_AUG_PLAN_STAGED}


def augment_filter_tables():
    """(hz [12] float32, sym6 [12] float64): the derived table of include/p3d_augment_table.h, as the library holds it.  hz is the
    operator's resampling filter: the order-6 least-asymmetric low-pass normalised to sum 1."""
    hz, s6 = (C.c_float * 12)(), (C.c_double * 12)()
    _lib.check(_lib.lib().p3d_augment_filter(hz, s6), "p3d_augment_filter")
    return np.array(hz, dtype=np.float32), np.array(s6, dtype=np.float64)


class AugmentGeometry:
    """What one call of the operator needs besides the image: the margins, the sampling matrices and their inverses on the host
    (the plan reads them) and on the device (the kernels read them), and the colour matrices [N, 12] on the device (or None)."""

    def __init__(self, margins, geo_host, geo_dev, col, plan):
        self.margins, self.geo_host, self.geo_dev, self.col, self.plan = margins, geo_host, geo_dev, col, plan
        self.tile = None  # whether the forward runs the tile kernel (then it needs no workspace); set by the first forward


def augment_colour_rows(C, num_channels):
    """C [N, 4, 4] -> the [N, 12] rows the operator reads: C[:, :3, :] for RGB triples; for one channel the reference's mean over the
    three rows (augment.py:369-370), as (scale, 0, 0, offset, 0 ...)."""
    C = _chk(C, "C")
    if C.ndim != 3 or C.shape[1:] != (4, 4):
        raise RuntimeError("augment: C must be [N, 4, 4]")
    if num_channels == 1:
        c1 = C[:, :3, :].mean(dim=1, keepdim=True)
        out = torch.zeros((C.shape[0], 12), dtype=torch.float32, device=C.device)
        out[:, 0:1] = c1[:, :, :3].sum(dim=2)
        out[:, 3:4] = c1[:, :, 3]
        return out
    if num_channels not in (3, 6):
        raise ValueError("Image must be RGB (3 channels) or L (1 channel)")
    return C[:, :3, :].reshape(-1, 12).contiguous()


def augment_geometry(G_inv, margins, C, shape, device, plan=None):
    """G_inv [N, 3, 3] (a HOST tensor or array, or None), the margins (mx0, my0, mx1, my1), C [N, 4, 4] on the device (or None) and
    the image's shape -> AugmentGeometry.  The sampling matrix is composed on the host in float64 (p3d_augment_geometry)."""
    N, Cc, H, W = shape
    plan = plan or os.environ.get("P3D_AUGMENT_PLAN") or "auto"
    if plan not in AUGMENT_PLANS:
        raise RuntimeError(f"augment: plan (or P3D_AUGMENT_PLAN) must be one of {sorted(k for k in AUGMENT_PLANS if k)}, got {plan!r}")
    plan = AUGMENT_PLANS[plan]
    geo_host = geo_dev = None
    margins = tuple(int(v) for v in margins) if margins is not None else (0, 0, 0, 0)
    if G_inv is not None:
        if isinstance(G_inv, torch.Tensor):
            if G_inv.is_cuda:
                raise RuntimeError("augment: G_inv is read on the host; pass a host copy (bring it back in the same copy as the margins)")
            G_inv = G_inv.numpy()
        g = np.ascontiguousarray(G_inv, dtype=np.float32)
        if g.shape != (N, 3, 3) or len(margins) != 4:
            raise RuntimeError("augment: G_inv must be [N, 3, 3] and margins (mx0, my0, mx1, my1)")
        geo_host = np.empty((N, 12), dtype=np.float32)
        _lib.check(_lib.lib().p3d_augment_geometry(g.ctypes.data, N, H, W, *margins, geo_host.ctypes.data), "p3d_augment_geometry")
        geo_dev = torch.from_numpy(geo_host).to(device, non_blocking=True)
    col = augment_colour_rows(C, Cc) if C is not None else None
    if col is not None and col.shape[0] != N:
        raise RuntimeError("augment: C must have the batch of the image")
    return AugmentGeometry(margins, geo_host, geo_dev, col, plan)


def _augment_impl(x, geom, adjoint):
    x = _chk(x, "images")
    if x.ndim != 4:
        raise RuntimeError("augment: images must be [N, C, H, W]")
    if geom.geo_host is None and geom.col is None:
        return x.clone()  # the identity; never the input itself (an autograd.Function must not return its input)
    N, Cc, H, W = x.shape
    L = _lib.lib()
    y = torch.empty_like(x)
    gh = geom.geo_host.ctypes.data if geom.geo_host is not None else None
    nbytes = L.p3d_augment_workspace_bytes(N, Cc, H, W, *geom.margins) if gh is not None else 0
    if gh is not None and not adjoint:
        if geom.tile is None:  # the plan walks every tile's box: once per geometry, not once per call
            out = (C.c_int * 4)()
            _lib.check(L.p3d_augment_plan(gh, N, H, W, *geom.margins, geom.plan, out, 4), "p3d_augment_plan")
            geom.tile = out[0] == _lib.P3D_AUG_PLAN_TILE
        if geom.tile:
            nbytes = 0
    ws = _sg_workspace(x.device, nbytes) if nbytes else None
    with _on(x.device):
        if adjoint:
            rc = L.p3d_augment_apply_adjoint_f32(_p(x), gh, _p(geom.geo_dev), _p(geom.col), N, Cc, H, W, *geom.margins, _p(y), _p(ws), nbytes, _stream())
        else:
            rc = L.p3d_augment_apply_f32(_p(x), gh, _p(geom.geo_dev), _p(geom.col), N, Cc, H, W, *geom.margins, geom.plan, _p(y), _p(ws), nbytes,
                                         _stream())
    _lib.check(rc, "p3d_augment_apply_adjoint_f32" if adjoint else "p3d_augment_apply_f32")
    return y


class _AugmentFn(torch.autograd.Function):
    """The operator is affine in the image and its adjoint linear: each is the other's backward, called through the public functions
    again, so a backward is itself recorded under create_graph=True and the pair is differentiable to any order with no further kernel."""

    @staticmethod
    def forward(ctx, x, geom, adjoint):
        ctx.geom, ctx.adjoint = geom, adjoint
        return _augment_impl(x, geom, adjoint)

    @staticmethod
    def backward(ctx, g):
        if ctx.adjoint:  # the adjoint's backward is the operator without its colour offset
            return _augment_linear(g, ctx.geom), None, None
        return augment_apply_adjoint(g, ctx.geom), None, None


def _augment_linear(x, geom):
    if geom.col is None:
        return augment_apply(x, geom)
    col = geom.col.clone()
    col[:, 3::4] = 0
    return augment_apply(x, AugmentGeometry(geom.margins, geom.geo_host, geom.geo_dev, col, geom.plan))


def _augment_geom(images, G_inv, margins, C, plan):
    if isinstance(G_inv, AugmentGeometry):
        return G_inv
    return augment_geometry(G_inv, margins, C, tuple(images.shape), images.device, plan)


def augment_apply(images, G_inv, margins=None, C=None, plan=None):
    """p3d_augment_apply_f32 on images [N, C, H, W]: reflect-pad by the margins, 2x up, bilinear sampling through G_inv [N, 3, 3] (host),
    2x down, and the colour matrix C [N, 4, 4] (device); either matrix may be None.  G_inv may also be a ready AugmentGeometry
    (augment_geometry), which several calls can share.  plan: None / "tile" / "staged" (or the environment's P3D_AUGMENT_PLAN).
    Differentiable in the images to any order; the same bits with and without autograd."""
    geom = _augment_geom(images, G_inv, margins, C, plan)
    if _wants_grad(images):
        return _AugmentFn.apply(images, geom, False)
    return _augment_impl(images, geom, False)


def augment_apply_adjoint(g, G_inv, margins=None, C=None, plan=None):
    """p3d_augment_apply_adjoint_f32: the transpose of augment_apply's linear part, applied to g [N, C, H, W]."""
    geom = _augment_geom(g, G_inv, margins, C, plan)
    if _wants_grad(g):
        return _AugmentFn.apply(g, geom, True)
    return _augment_impl(g, geom, True)


# ---- the augmentation pipe's tail (include/p3d_augment_tail.h) ---------------------------------------------------------
class AugmentTail:
    """What one call of the tail needs besides the image, on the device: taps [N, K] (or None), z [N, C, H, W] and sigma [N] (both or
    neither), rect [N, 4] int32 = (x0, x1, y0, y1) (or None)."""

    def __init__(self, taps=None, z=None, sigma=None, rect=None):
        self.taps = _chk(taps, "taps") if taps is not None else None
        self.z = _chk(z, "z") if z is not None else None
        self.sigma = _chk(sigma, "sigma").reshape(-1) if sigma is not None else None
        self.rect = _chk(rect, "rect", torch.int32) if rect is not None else None
        if (self.z is None) != (self.sigma is None):
            raise RuntimeError("augment_tail: the noise needs both z and sigma")
        if self.taps is not None and (self.taps.ndim != 2 or self.taps.shape[1] % 2 == 0 or self.taps.shape[1] > _lib.P3D_TAIL_MAX_TAPS):
            raise RuntimeError(f"augment_tail: taps must be [N, K] with K odd and at most {_lib.P3D_TAIL_MAX_TAPS}")


def augment_tail_plan(K):
    """(the forward's tile height, its LDS bytes, the adjoint's tile height, its LDS bytes) for K taps; the tile is P3D_TAIL_TILE_W wide."""
    out = (C.c_int * 4)()
    _lib.check(_lib.lib().p3d_augment_tail_plan(int(K), out, 4), "p3d_augment_tail_plan")
    return tuple(out)


def _augment_tail_impl(x, tail, adjoint):
    x = _chk(x, "images")
    if x.ndim != 4:
        raise RuntimeError("augment_tail: images must be [N, C, H, W]")
    N, Cc, H, W = x.shape
    for t, name, shape in ((tail.taps, "taps", None), (tail.z, "z", tuple(x.shape)), (tail.sigma, "sigma", (N,)), (tail.rect, "rect", (N, 4))):
        if t is None:
            continue
        if t.device != x.device or t.shape[0] != N or (shape is not None and tuple(t.shape) != shape):
            raise RuntimeError(f"augment_tail: {name} must be on the images' device with their batch" + (f", shaped {shape}" if shape else ""))
    K = tail.taps.shape[1] if tail.taps is not None else 0
    if K // 2 >= min(H, W) and K:
        raise RuntimeError(f"augment_tail: {K} taps reflect {K // 2} pixels, beyond an image of {H} x {W} (P3D_E_RANGE)")
    y = torch.empty_like(x)
    L = _lib.lib()
    with _on(x.device):
        if adjoint:
            rc = L.p3d_augment_tail_adjoint_f32(_p(x), _p(tail.taps), K, _p(tail.rect), N, Cc, H, W, _p(y), _stream())
        else:
            rc = L.p3d_augment_tail_f32(_p(x), _p(tail.taps), K, _p(tail.z), _p(tail.sigma), _p(tail.rect), N, Cc, H, W, _p(y), _stream())
    _lib.check(rc, "p3d_augment_tail_adjoint_f32" if adjoint else "p3d_augment_tail_f32")
    return y


class _AugmentTailFn(torch.autograd.Function):
    """The tail is affine in the image (its offset the noise) and its adjoint linear: each is the other's backward, called through the
    public functions again, so the pair is differentiable to any order with no further kernel (the pattern of _AugmentFn)."""

    @staticmethod
    def forward(ctx, x, tail, adjoint):
        ctx.tail, ctx.adjoint = tail, adjoint
        return _augment_tail_impl(x, tail, adjoint)

    @staticmethod
    def backward(ctx, g):
        t = ctx.tail
        if ctx.adjoint:  # the adjoint's backward is the tail without its noise
            return augment_tail(g, AugmentTail(t.taps, None, None, t.rect)), None, None
        return augment_tail_adjoint(g, t), None, None


def _augment_tail_args(taps, z, sigma, rect):
    return taps if isinstance(taps, AugmentTail) else AugmentTail(taps, z, sigma, rect)


def augment_tail(images, taps=None, z=None, sigma=None, rect=None):
    """p3d_augment_tail_f32 on images [N, C, H, W]: the per-sample separable filter taps [N, K] on the reflected image (rows, then
    columns), + sigma [N] * z [N, C, H, W], then zero inside rect [N, 4] int32 = (x0, x1, y0, y1); every stage optional, all on the
    device.  taps may also be a ready AugmentTail.  Differentiable in the images to any order, with no gradient to taps, sigma or z;
    the same bits with and without autograd."""
    tail = _augment_tail_args(taps, z, sigma, rect)
    if _wants_grad(images):
        return _AugmentTailFn.apply(images, tail, False)
    return _augment_tail_impl(images, tail, False)


def augment_tail_adjoint(g, taps=None, z=None, sigma=None, rect=None):
    """p3d_augment_tail_adjoint_f32: the transpose of augment_tail's linear part (the noise does not enter), applied to g [N, C, H, W]."""
    tail = _augment_tail_args(taps, z, sigma, rect)
    if _wants_grad(g):
        return _AugmentTailFn.apply(g, tail, True)
    return _augment_tail_impl(g, tail, True)
