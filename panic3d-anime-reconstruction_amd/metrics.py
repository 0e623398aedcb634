"""The geometry rows of the evaluation table — `_scripts/eval/measure.py:54-99` and `:186-201` — on the device: the distance from
sample points to a mesh (csrc/p3d_metrics.hip in place of `igl.point_mesh_squared_distance`), points drawn on a mesh by area (in
place of `igl.random_points_on_mesh`), the region-of-interest filter, Chamfer distance and F1.

A mesh is a dict with 'verts' [V,3] float32 and 'faces' [F,3] int32, device tensors or numpy arrays (which are uploaded); what
`volume.marching_cubes` / `volume.mesh` return fits as it is.  Nothing comes back to the host until the caller reads a value, apart
from one small read per distance call (the index check) and one per sampling call (the total area).
"""
import numpy as np
import torch

from . import ops

# Culling (skip face tiles that are provably too far; bit-identical results): on by default, five times faster at the evaluation's size
# (DESIGN.md §4.16 has the two timings).
DEFAULT_CULL = True
CULL_MARGIN_FACTOR = 64.0 * 2.0 ** -24  # times the squared diagonal of the joint bounding box of mesh and queries


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError("panic3d_amd.metrics: numpy input needs a GPU to be uploaded to (the HIP path has no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def _as_tensor(x, dtype, device=None):
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x)).to(device if device is not None else _device())
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"expected a tensor or a numpy array, got {type(x).__name__}")
    return x if dtype is None or x.dtype == dtype else x.to(dtype)


def _faces(faces, device=None):
    faces = _as_tensor(faces, None, device)
    if faces.dtype != torch.int32:
        raise ValueError(f"faces must be int32, got {faces.dtype}")
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"faces must be [F,3], got {tuple(faces.shape)}")
    return faces


def _mesh(mesh):
    verts = _as_tensor(mesh["verts"], torch.float32)
    return verts, _faces(mesh["faces"], verts.device)


def morton_codes(points, lo, hi):
    """30-bit Morton code (10 bits per axis, x in the lowest bit) of points [Q,3] in the box [lo, hi]."""
    cell = ((points - lo) / (hi - lo).clamp_min(1e-30) * 1023.0).long().clamp_(0, 1023)

    def spread(x):
        x = (x | (x << 16)) & 0x030000FF
        x = (x | (x << 8)) & 0x0300F00F
        x = (x | (x << 4)) & 0x030C30C3
        return (x | (x << 2)) & 0x09249249
    return spread(cell[:, 0]) | (spread(cell[:, 1]) << 1) | (spread(cell[:, 2]) << 2)


def point_mesh_squared_distance(points, verts, faces, cull=None, slices=0, sort=None):
    """`igl.point_mesh_squared_distance(points, verts, faces)` (measure.py:82): (sqrD [Q], I [Q] int32, C [Q,3]) — the squared distance
    to the mesh, the closest face (the lowest index among equals) and the closest point, device tensors, by the arithmetic of
    include/p3d_metrics.h.  Raises ValueError for faces that are not int32 [F,3] with 0 <= index < V: a bad index never reaches the
    kernel.  cull (default metrics.DEFAULT_CULL): sort the queries by Morton code and skip face tiles that are too far — the outputs are
    bit-identical either way.  slices / sort: force the face-slice count / the Morton sort (tests and tools/bench_metrics.py)."""
    verts = _as_tensor(verts, torch.float32)
    points = _as_tensor(points, torch.float32, verts.device)
    faces = _faces(faces, verts.device)
    if points.dim() != 2 or points.shape[1] != 3 or verts.dim() != 2 or verts.shape[1] != 3:
        raise ValueError("points must be [Q,3] and verts [V,3]")
    V, F, Q = verts.shape[0], faces.shape[0], points.shape[0]
    if V < 1 or F < 1:
        raise ValueError("the mesh has no vertices or no faces")
    cull = DEFAULT_CULL if cull is None else bool(cull)
    sort = cull if sort is None else bool(sort)
    bad = ((faces < 0) | (faces >= V)).any()
    margin = 0.0
    if (cull or sort) and Q > 0:
        lo = torch.minimum(verts.amin(0), points.amin(0))
        hi = torch.maximum(verts.amax(0), points.amax(0))
        bad, diag2 = torch.stack([bad.double(), ((hi - lo).double() ** 2).sum()]).tolist()  # ONE read for the check and the margin
        margin = CULL_MARGIN_FACTOR * diag2
    else:
        bad = bool(bad)
    if bad:
        raise ValueError(f"faces holds an index outside [0, {V})")
    if not (margin < float("inf")):
        raise ValueError("points and verts must be finite")
    if sort and Q > 0:
        perm = torch.sort(morton_codes(points, lo, hi))[1]
        d2, face, closest = ops.point_mesh_dist2(points[perm].contiguous(), verts, faces, cull=cull, cull_margin=margin, slices=slices)
        out = (torch.empty_like(d2), torch.empty_like(face), torch.empty_like(closest))
        for o, r in zip(out, (d2, face, closest)):
            o[perm] = r
        return out
    return ops.point_mesh_dist2(points, verts, faces, cull=cull, cull_margin=margin, slices=slices)


def sample_points_on_mesh(verts, faces, n, generator=None):
    """n points on the mesh, uniform by area: (points [n,3] float32, face_index [n] int64, barycentric [n,3] float64).  A face is drawn
    with probability proportional to its area (areas and their cumulative sum in float64, torch.searchsorted on uniform draws), then
    barycentrics (1 - sqrt(u1), sqrt(u1) (1 - u2), sqrt(u1) u2).  The same DISTRIBUTION as `igl.random_points_on_mesh`
    (lustrous_gltf_v0_measurable.py sample_points_near_surface with sigma = 0), not the same points: igl's generator cannot be
    reproduced.  generator: a torch.Generator on the mesh's device.  A mesh whose total area is 0 raises ValueError."""
    verts = _as_tensor(verts, torch.float32)
    faces = _faces(faces, verts.device)
    if faces.shape[0] < 1:
        raise ValueError("sample_points_on_mesh: the mesh has no faces")
    v = verts.double()
    a, b, c = (v[faces[:, k].long()] for k in range(3))
    area = 0.5 * torch.linalg.cross(b - a, c - a).norm(dim=1)
    cum = torch.cumsum(area, 0)
    total = float(cum[-1])
    if not (total > 0.0 and total < float("inf")):
        raise ValueError(f"sample_points_on_mesh: the mesh's total area is {total}")
    u = torch.rand((int(n), 3), dtype=torch.float64, device=verts.device, generator=generator)
    idx = torch.searchsorted(cum, u[:, 0] * cum[-1], right=True).clamp_max(faces.shape[0] - 1)  # right: a zero-area face is never drawn
    s = u[:, 1].sqrt()
    bary = torch.stack([1 - s, s * (1 - u[:, 2]), s * u[:, 2]], 1)
    pts = bary[:, 0:1] * a[idx] + bary[:, 1:2] * b[idx] + bary[:, 2:3] * c[idx]
    return pts.float(), idx, bary


def roi_bounds(roi, bw, size=512):
    """The world-space rectangle (x_lo, x_hi, y_lo, y_hi) of a region of interest given as ((row, column), (height, width)) in pixels
    of a size^2 front view of a box of width bw centred on the origin.  Image columns run along +x from -bw/2, image rows along -y
    from +bw/2 — measure.py:54-61's convention and its order of operations, so a vertex on a boundary falls on the same side."""
    (row, col), (height, width) = roi
    x_lo = -bw / 2 + ((col / size) * bw)
    y_hi = bw / 2 - ((row / size) * bw)
    return x_lo, x_lo + bw * (width / size), y_hi - bw * (height / size), y_hi


def filter_mesh(verts, faces, roi, bw, size=512):
    """The part of a mesh inside a region of interest (measure.py:54-76): the vertices strictly inside roi_bounds(roi, bw, size) in x and
    y, the faces whose three vertices all survive, re-indexed to the surviving vertices (a vertex's new index is the number of survivors
    before it).  dict(verts, faces), on the mesh's device."""
    verts = _as_tensor(verts, None)
    faces = _faces(faces, verts.device)
    x_lo, x_hi, y_lo, y_hi = roi_bounds(roi, bw, size)
    x, y = verts[:, 0], verts[:, 1]
    keep = (x > x_lo) & (x < x_hi) & (y > y_lo) & (y < y_hi)
    new_index = (torch.cumsum(keep, 0) - 1).to(torch.int32)
    whole = keep[faces.long()].all(dim=1)
    return {"verts": verts[keep], "faces": new_index[faces[whole].long()]}


def point_mesh_f1(p2s, s2p, thresh):
    """measure.py:87-99: precision = the share of p2s <= thresh, recall = the share of s2p <= thresh, f1 = their harmonic mean, 0 when
    both are 0.  0-d float64 device tensors."""
    pre = (p2s <= thresh).double().mean()
    rec = (s2p <= thresh).double().mean()
    s = pre + rec
    f1 = 2 * pre * rec / torch.where(s > 0, s, torch.ones_like(s))
    return {"precision": pre, "recall": rec, "threshold": thresh, "f1": f1}


def psnr(pred, target, data_range=None):
    """`torchmetrics.PeakSignalNoiseRatio()(pred, target)` (measure.py:45) as a float: ONE value for the whole batch,
    10 log10(range^2 / mse) with mse = sum (pred - target)^2 / count.  data_range=None (the reference's default-constructed metric):
    range = max(target) - min(target) — torchmetrics was not available where this was written, so that default is UNCHECKED against the
    package.  The three reductions come from one pass on the device in binary32 (ops.psnr_sums: one small read); the division and the
    logarithm are taken here in float64.  Identical images give inf.  A constant target with data_range=None has range 0: the formula is
    evaluated as torch would evaluate it, -inf (nan when the images are identical as well)."""
    if not isinstance(pred, torch.Tensor) or not isinstance(target, torch.Tensor) or pred.shape != target.shape:
        raise ValueError("psnr: two tensors of one shape")
    if torch.is_grad_enabled() and (pred.requires_grad or target.requires_grad):
        raise NotImplementedError("psnr is inference only: detach the images or call it under torch.no_grad()")
    if data_range is not None and not float(data_range) > 0.0:
        raise ValueError(f"psnr: data_range must be positive, got {data_range}")
    if pred.numel() == 0 or pred.dtype != torch.float32 or target.dtype != torch.float32:
        raise ValueError("psnr: non-empty float32 tensors")
    ss, lo, hi = (np.float64(v) for v in ops._psnr_sums_impl(pred.detach().contiguous(), target.detach().contiguous()).tolist())
    rng = np.float64(data_range) if data_range is not None else hi - lo
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(10.0 * np.log10(rng * rng / (ss / np.float64(pred.numel()))))


def image_metrics(pred, gt, lpips_model, clip_model):
    """The 2-D block of measure.py:34-50 for one batch of views: {'lpips', 'psnr', 'clip'} as floats.  pred, gt [N,3,H,W] float32 in
    [0, 1]; lpips_model a panic3d_amd.LPIPSLoss (called as the reference calls it, on the images as they are), clip_model a
    panic3d_amd.CLIPSimilarity.  lpips and clip are means over the batch (the reference passes one view at a time)."""
    with torch.no_grad():
        return {"lpips": float(lpips_model(pred, gt).double().mean()), "psnr": psnr(pred, gt), "clip": float(clip_model(pred, gt).double().mean())}


def geometry_metrics(mesh_pred, mesh_gt, n_sample=10000, thresholds=(0.005, 0.01, 0.05, 0.1, 0.5), generator=None, points_pred=None,
                     points_gt=None):
    """measure.py:186-201 for one subject: p2s = the mean distance from points on the predicted mesh to the ground-truth mesh, s2p the
    other way round, cd = their mean, f1_XXX = point_mesh_f1 at each threshold (XXX = 1000 * threshold rounded, three digits) — 0-d float64
    device tensors — and the points used.  points_pred / points_gt skip the sampling.  (The reference's line 201 ASSIGNS the F1 instead
    of appending it, so its table shows the last subject's value; here every subject gets its own, the caller averages.)"""
    vp, fp = _mesh(mesh_pred)
    vg, fg = _mesh(mesh_gt)
    if points_pred is None:
        points_pred = sample_points_on_mesh(vp, fp, n_sample, generator)[0]
    if points_gt is None:
        points_gt = sample_points_on_mesh(vg, fg, n_sample, generator)[0]
    points_pred = _as_tensor(points_pred, torch.float32, vp.device)
    points_gt = _as_tensor(points_gt, torch.float32, vp.device)
    p2s = point_mesh_squared_distance(points_pred, vg, fg)[0].double().sqrt()
    s2p = point_mesh_squared_distance(points_gt, vp, fp)[0].double().sqrt()
    out = {"p2s": p2s.mean(), "s2p": s2p.mean()}
    out["cd"] = (out["p2s"] + out["s2p"]) / 2
    for th in thresholds:
        out["f1_%03d" % round(th * 1000)] = point_mesh_f1(p2s, s2p, th)["f1"]
    out["points_pred"], out["points_gt"] = points_pred, points_gt
    return out
