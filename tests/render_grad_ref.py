"""The float64 references of the renderer / point-decode backward (include/p3d_render_grad.h), in one place.

restate64         ImportanceRenderer.forward after the depths are drawn (ray_marcher.py, renderer.py, triplane.py) as torch ops at
                  GIVEN merged, sorted depths, differentiated by autograd;
decode_restate64  the same for run_model (renderer.py:266-280) on points.

Both take their mask decisions as DATA (the forward's own sigma with its +-1000 sentinels, or a boolean array): a cull decision must
not flip between binary32 and binary64.  Both can run in another dtype (the conditioning check of
tests/test_render_grad_ref_cpu.py) and with one seeded defect `mut` (that file's mutations).  Both can return a "touched" map: the
plane texels that receive a tap of at least one sample whose gradient is not structurally zero, from float64 tap geometry at the
binary32 points.  None of this is written from the kernels."""
import numpy as np
import torch
import torch.nn.functional as F

SENTINELS = (-1000.0, 1000.0)  # P3D_SIGMA_MASKED, P3D_SIGMA_SOLID (renderer.py:143,190-198)
TAPS = ((0, 0), (1, 0), (0, 1), (1, 1))  # (dx, dy) of nw, ne, sw, se


def plane_axes(use_triplane):
    """generate_planes (renderer.py:26-50): the (x, y) grid coordinates of the three planes."""
    return [(0, 1), (0, 2), (1, 2) if use_triplane else (2, 0)]


def rel_l2(ours, ref):
    """Relative L2 over the reference's finite entries; NaN if ours is not finite there."""
    ours, ref = np.asarray(ours, np.float64), np.asarray(ref, np.float64)
    fin = np.isfinite(ref)
    return float(np.linalg.norm((ours - ref)[fin]) / max(np.linalg.norm(ref[fin]), 1e-30))


def points32(rays_o, rays_d, depths):
    """The binary32 sample points o + t * d, multiply then add (renderer.py:179): [N,R,S,3]."""
    o, d, t = rays_o.float().cpu(), rays_d.float().cpu(), depths.float().cpu()
    return o.unsqueeze(-2) + t.reshape(*o.shape[:2], -1, 1) * d.unsqueeze(-2)


# ---- tap geometry in float64 ---------------------------------------------------------------------------------------------------
def plane_taps64(gx, gy, H, W):
    """F.grid_sample(bilinear, zeros, align_corners=False) geometry of one plane: (x [4,...], y, weight, valid) per tap.  A point
    outside (-1, W) x (-1, H) has no valid tap."""
    gx, gy = np.asarray(gx, np.float64), np.asarray(gy, np.float64)
    ix, iy = (gx + 1) * (0.5 * W) - 0.5, (gy + 1) * (0.5 * H) - 0.5
    inside = (ix > -1) & (ix < W) & (iy > -1) & (iy < H)
    x0, y0 = np.floor(ix), np.floor(iy)
    wx1, wy1 = ix - x0, iy - y0
    xs, ys, ws, ok = [], [], [], []
    for dx, dy in TAPS:
        x, y = x0 + dx, y0 + dy
        xs.append(x)
        ys.append(y)
        ws.append((wx1 if dx else 1 - wx1) * (wy1 if dy else 1 - wy1))
        ok.append(inside & (x >= 0) & (x < W) & (y >= 0) & (y < H))
    return np.stack(xs), np.stack(ys), np.stack(ws), np.stack(ok)


def tap_classes(pts, H, W, box_warp, use_triplane):
    """Per (sample, plane): 0 = no tap in range, 1 = one to three taps in range (the half-texel border), 2 = all four."""
    q = np.asarray(pts, np.float64).reshape(-1, 3) * (2.0 / box_warp)
    out = []
    for a, b in plane_axes(use_triplane):
        n = plane_taps64(q[:, a], q[:, b], H, W)[3].sum(0)
        out.append(np.where(n == 0, 0, np.where(n == 4, 2, 1)))
    return np.stack(out, 1)


def touched_map(pts, live, Np, H, W, box_warp, use_triplane, band=None):
    """bool [Np,3,H,W]: texels that a live sample (pts [N,M,3] binary32, live [N,M]) may write.  A tap of weight exactly zero
    writes nothing; a coordinate within `band` texels of a texel centre or of the plane's edge (where binary32 and binary64 may
    floor differently) marks both candidates."""
    pts = np.asarray(pts, np.float32)
    N = pts.shape[0]
    band = 4e-6 * (max(H, W) + 2) if band is None else band
    out = np.zeros((Np, 3, H, W), bool)
    img = np.broadcast_to((np.arange(N) if Np > 1 else np.zeros(N, int))[:, None], pts.shape[:2])[live]
    q = pts.astype(np.float64)[live] * (2.0 / box_warp)
    for p, (a, b) in enumerate(plane_axes(use_triplane)):
        ix, iy = (q[:, a] + 1) * (0.5 * W) - 0.5, (q[:, b] + 1) * (0.5 * H) - 0.5
        inside = (ix + band > -1) & (ix - band < W) & (iy + band > -1) & (iy - band < H)
        rng = []
        for i, n in ((ix, W), (iy, H)):
            exact = i == np.floor(i)
            lo = np.where(exact, i, np.floor(i - band))
            hi = np.where(exact, i, np.floor(i + band) + 1)
            rng.append((lo, hi, n))
        for dx in range(3):
            for dy in range(3):
                x, y = rng[0][0] + dx, rng[1][0] + dy
                ok = inside & (x <= rng[0][1]) & (y <= rng[1][1]) & (x >= 0) & (x < W) & (y >= 0) & (y < H)
                out[img[ok], p, y[ok].astype(int), x[ok].astype(int)] = True
    return out


# ---- the decode (triplane.py sample_from_planes + OSGDecoder) ---------------------------------------------------------------------
def _sample_taps(src, gx, gy, shift=None):
    """grid_sample restated tap by tap (src [N,C,H,W], gx / gy [N,M]) -> [N,C,M].  shift = (bool [N,M], tap): those samples READ
    that tap where they should and send its gradient one texel to the right (a mutation)."""
    N, Cc, H, W = src.shape
    flat = src.reshape(N, Cc, H * W)
    ix, iy = (gx + 1) * (0.5 * W) - 0.5, (gy + 1) * (0.5 * H) - 0.5
    inside = (ix > -1) & (ix < W) & (iy > -1) & (iy < H)
    x0, y0 = torch.floor(ix), torch.floor(iy)
    wx1, wy1 = ix - x0, iy - y0
    out = 0
    for k, (dx, dy) in enumerate(TAPS):
        x, y = x0 + dx, y0 + dy
        w = (wx1 if dx else 1 - wx1) * (wy1 if dy else 1 - wy1)
        ok = inside & (x >= 0) & (x < W) & (y >= 0) & (y < H)
        idx = (y.clamp(0, H - 1) * W + x.clamp(0, W - 1)).long()
        v = torch.gather(flat, 2, idx[:, None, :].expand(N, Cc, -1))
        if shift is not None and shift[1] == k:
            to = torch.gather(flat, 2, (idx + shift[0].long()).clamp(max=H * W - 1)[:, None, :].expand(N, Cc, -1))
            v = v.detach() + (to - to.detach())
        out = out + v * (w * ok)[:, None, :]
    return out


def _decode(pl, mlp, pts, box_warp, use_triplane, fsig, mut):
    """pl [Np,3,32,H,W], pts [N,M,3] -> sigma [N,M], rgb [N,M,32] (triplane.py:516-544, renderer.py:52-81)."""
    N, M, _ = pts.shape
    w0, b0, w1, b1 = mlp
    q = pts * (2.0 / box_warp)
    axes = plane_axes(use_triplane)
    if "swap2" in mut:
        axes[2] = axes[2][::-1]
    feats = 0
    for p, (a, b) in enumerate(axes):
        src = pl[:, p]
        if "image0" in mut:
            src = src[:1]
        if src.shape[0] == 1 and N > 1:
            src = src.expand(N, -1, -1, -1)
        if "tap" in mut or mut.get("sampler") == "taps":
            sh = mut.get("tap")
            feats = feats + _sample_taps(src, q[..., a], q[..., b], (sh[0], sh[2]) if sh is not None and sh[1] == p else None)
        else:
            grid = torch.stack([q[..., a], q[..., b]], -1).reshape(N, 1, -1, 2)
            feats = feats + F.grid_sample(src, grid, mode="bilinear", padding_mode="zeros", align_corners=False).reshape(N, 32, -1)
    X = (feats / 3).permute(0, 2, 1)
    h = F.softplus(X @ w0.t() + b0)
    o = h @ w1.t() + b1
    if "drop" in mut:  # those samples' whole contribution to every gradient
        o = torch.where(mut["drop"].reshape(N, M, 1), o.detach(), o)
    sg = torch.sigmoid(o[..., 1:])
    rgb = sg if fsig else sg * (1.0 if "no1002" in mut else 1.002) - 0.001
    return o[..., 0], rgb


def _leaves(planes, mlp, dtype):
    pl = planes.detach().to(dtype).requires_grad_(True)
    return pl, [t.detach().to(dtype).requires_grad_(True) for t in mlp]


def _grads(loss, pl, ps):
    if not loss.requires_grad:  # no cotangent at all
        return torch.zeros_like(pl), [torch.zeros_like(x) for x in ps]
    g = torch.autograd.grad(loss, [pl] + ps, allow_unused=True)
    g = [torch.zeros_like(x) if v is None else v for v, x in zip(g, [pl] + ps)]
    return g[0], g[1:]


def _nonzero_rows(c):
    return None if c is None else (np.asarray(c.detach().cpu(), np.float64).reshape(c.shape[0], c.shape[1], -1) != 0).any(-1)


def restate64(planes, mlp, rays_o, rays_d, depths, sig_dump, opts, ro, cot, per_view, fsig, dtype=torch.float64, mut=None,
              touched=False):
    """ray_marcher.py + renderer.py + triplane.py as float64 torch ops at the given merged depths [N,R,S] (sorted per ray; any
    S >= 2); mask decisions taken from the forward's own sigma dump (a cull decision must not flip between binary32 and binary64:
    entries equal to a sentinel are masked, every other entry is ignored).  planes [N,3,32,H,W] or [1,...] shared by the N views;
    ro: box_warp, use_triplane, white_back; cot = (g_feat, g_depth, g_wsum, g_xyz), any None.  `opts` is not read (kept for the
    callers).  Returns the loss's gradients (planes, [w0, b0, w1, b1]) and, if `touched`, the touched map [Np,3,H,W]."""
    mut = mut or {}
    N, R, _ = rays_o.shape
    depths = depths.detach().reshape(N, R, -1)
    S = depths.shape[-1]
    pl, ps = _leaves(planes, mlp, dtype)
    t = depths.to(dtype).reshape(N, R, S, 1)
    pts = rays_o.detach().to(dtype).unsqueeze(-2) + t * rays_d.detach().to(dtype).unsqueeze(-2)  # [N,R,S,3]
    sigma, rgb = _decode(pl, ps, pts.reshape(N, -1, 3), ro["box_warp"], ro["use_triplane"], fsig, mut)
    sigma, rgb = sigma.reshape(N, R, S, 1), rgb.reshape(N, R, S, 32)
    sd = sig_dump.detach().reshape(N, R, S, 1).to(dtype)
    masked = (sd == SENTINELS[0]) | (sd == SENTINELS[1])
    if "nomask" in mut:
        masked = torch.zeros_like(masked)
    if "maskgrad" in mut:  # the forward's value, the unmasked sample's gradient
        sigma = torch.where(masked, sd + (sigma - sigma.detach()), sigma)
    else:
        sigma = torch.where(masked, sd, sigma)
    colors = torch.cat([rgb, pts], -1)
    deltas = t[:, :, 1:] - t[:, :, :-1]
    cm = (colors[:, :, :-1] + colors[:, :, 1:]) / 2
    dm = F.softplus((sigma[:, :, :-1] + sigma[:, :, 1:]) / 2 - 1)
    tm = (t[:, :, :-1] + t[:, :, 1:]) / 2
    alpha = 1 - torch.exp(-dm * deltas)
    T_ = torch.cumprod(torch.cat([torch.ones_like(alpha[:, :, :1]), 1 - alpha + 1e-10], -2), -2)[:, :, :-1]
    w = alpha * T_
    comp = (w * cm).sum(-2)
    W = w.sum(2)
    if "depthW0" in mut:  # no nan_to_num: the division's backward runs on rays of zero total weight
        D = (w * tm).sum(-2) / W
    else:  # nan_to_num(D / W, inf) (ray_marcher.py:47-48): a constant where W == 0
        D = (w * tm).sum(-2) / torch.where(W > 0, W, torch.ones_like(W))
        D = torch.where(W > 0, D, torch.full_like(D, float("inf")))
    if per_view:
        lo = t.reshape(N, -1).min(1).values.view(N, 1, 1)
        hi = t.reshape(N, -1).max(1).values.view(N, 1, 1)
        D = torch.minimum(torch.maximum(D, lo), hi)
    else:
        D = torch.clamp(D, t.min().item(), t.max().item())
    if ro.get("white_back", False) and "nowhite" not in mut:
        comp = comp + 1 - W
    comp = comp * 2 - 1
    loss = torch.zeros((), dtype=dtype, device=pl.device)
    for c, x in zip(cot, (comp[..., :32], D, W, comp[..., 32:])):
        if c is not None:
            loss = loss + (x * c.detach().to(dtype).reshape(x.shape)).sum()
    gp, gm = _grads(loss, pl, ps)
    if not touched:
        return gp, gm
    # structurally non-zero: the colour path needs a non-zero g_feat on the ray, the density path any non-zero cotangent on the
    # ray and an unmasked sample (positions carry no plane gradient: g_xyz acts through the weights only)
    rows = [_nonzero_rows(c) for c in cot]
    zero = np.zeros((N, R), bool)
    anyc = rows[0] if rows[0] is not None else zero
    anyg = np.any([r for r in rows if r is not None] or [zero], 0)
    live = anyc[:, :, None] | (anyg[:, :, None] & ~masked.cpu().numpy().reshape(N, R, S))
    p32 = points32(rays_o, rays_d, depths).numpy().reshape(N, R * S, 3)
    H, Wd = pl.shape[-2:]
    return gp, gm, touched_map(p32, live.reshape(N, R * S), pl.shape[0], H, Wd, ro["box_warp"], ro["use_triplane"])


def decode_restate64(planes, mlp, coords, g_sigma, g_rgb, masked, ro, fsig, dtype=torch.float64, mut=None):
    """run_model (renderer.py:266-280) on coords [N,M,3] with cotangents g_sigma [N,M(,1)] and g_rgb [N,M,32] (either None);
    masked [N,M] bool: the points whose density a mask overwrote (a constant: no gradient; their colours keep theirs).  planes
    [N,3,32,H,W] or [1,...] shared.  Returns (planes gradient, [w0, b0, w1, b1] gradients, touched map [Np,3,H,W])."""
    mut = mut or {}
    N, M, _ = coords.shape
    pl, ps = _leaves(planes, mlp, dtype)
    pts = coords.detach().to(dtype)
    sigma, rgb = _decode(pl, ps, pts, ro["box_warp"], ro["use_triplane"], fsig, mut)
    mk = torch.as_tensor(np.asarray(masked, bool), device=pl.device).reshape(N, M)
    if "nomask" in mut or "maskgrad" in mut:
        mk = torch.zeros_like(mk)
    sigma = torch.where(mk, sigma.detach(), sigma)
    loss = torch.zeros((), dtype=dtype, device=pl.device)
    if g_sigma is not None:
        loss = loss + (sigma * g_sigma.detach().to(dtype).reshape(N, M)).sum()
    if g_rgb is not None:
        loss = loss + (rgb * g_rgb.detach().to(dtype)).sum()
    gp, gm = _grads(loss, pl, ps)
    zero = np.zeros((N, M), bool)
    anyc = _nonzero_rows(g_rgb) if g_rgb is not None else zero
    anys = _nonzero_rows(g_sigma.reshape(N, M, 1)) if g_sigma is not None else zero
    live = anyc | (anys & ~np.asarray(masked, bool).reshape(N, M))
    H, Wd = pl.shape[-2:]
    tm = touched_map(coords.detach().float().cpu().numpy(), live, pl.shape[0], H, Wd, ro["box_warp"], ro["use_triplane"])
    return gp, gm, tm


# ---- the gate of tests/test_hip_render_grad_edges.py ---------------------------------------------------------------------------
KEYS = ("planes", "w0", "b0", "w1", "b1")


def gate_errors(gp, gm, ref_gp, ref_gm, touched):
    """Relative L2 per tensor (planes [Np,3,32,H,W]), the number of non-zero entries outside the touched map, finiteness."""
    ours = [np.asarray(x.detach().cpu() if torch.is_tensor(x) else x, np.float64) for x in [gp] + list(gm)]
    ref = [np.asarray(x.detach().cpu(), np.float64) for x in [ref_gp] + list(ref_gm)]
    errs = {k: rel_l2(a, b) for k, a, b in zip(KEYS, ours, ref)}
    stray = int(np.count_nonzero(ours[0][~np.broadcast_to(touched[:, :, None], ours[0].shape)]))
    return errs, stray, all(np.isfinite(a).all() for a in ours)


def gate_passes(errs, stray, finite, tol):
    return bool(finite and stray == 0 and all(e <= tol for e in errs.values()))
