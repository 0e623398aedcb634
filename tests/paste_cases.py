"""Cases, float64 restatement and gate shared by the tests of the front-view paste's FORWARD kernel (k_paste_front, csrc/p3d_paste.hip;
tests/test_paste_forward_cpu.py, tests/test_hip_paste_forward.py).  Not collected.

`paste_forward_ref` restates training/triplane.py:553-691 (as panic3d_amd/paste.py words it) in float64 from the formulas, with a
per-pixel allowance for every output that is built from the restatement alone:

  sum part         GATE_C sqrt(K) 2^-24 sum|terms| (synthesis_grad_ref.GATE_C), the project's gate for a binary32 sum of K terms; it is
                   carried through a later step by that step's derivative (through the square roots as tol(q^2) / (2 q), through the
                   map from the up-sampled x / y to the sampling coordinate as S / box_warp).
  coordinate part  two binary32 evaluations of a source coordinate differ legitimately (a fused multiply-add where another takes two
                   steps; ix carries about an ulp of S): 2 ulps of the coordinate's magnitude, 2 * 2^-23 * max(1, |coordinate|), times
                   the largest difference between the tap values the coordinate blends.  A coordinate that lies within that distance of
                   a cell boundary blends, in one of the two evaluations, the taps of the neighbouring cell: those differences count
                   too.  For the illustration the 3 x 3 cells around the sampled one are taken throughout.

A pixel is UNDECIDED for a binary mask when its continuous quantity lies within its allowance of the threshold; the 0/1 masks must be
equal on decided pixels, and `mask` / `image` are compared where all three binary masks are decided.  The thresholds are fixed
constants in CASES, never a statistic of the data (the nearest-sampled discrepancy repeats each source value (S/r)^2 times, and a
median IS one of them)."""
import math

import torch
import torch.nn.functional as F

from synthesis_grad_ref import EPS32, GATE_C
from train_step_cases import _bilerp, up_taps

BW = 0.7
THRESH_WEIGHT, THRESH_OCC = 0.45, 0.5
UNDECIDED_SHARE, SMALL_CASE = 0.005, 400  # at most 0.5 % undecided pixels per mask; none in a case of fewer than 400 pixels

# (r, S, N, shared illustration, normalize_images, xyz scale, thresh_edges, thresh_dxyz, seed).  The seed is 1000 r + S + N, except for
# the one-pixel case: the first seed after that at which the pixel's weight passes and its mask_occ is fractional.  The edge and
# discrepancy thresholds: 0.005 above the case's median of the continuous quantity rounded to two decimals (computed once, written down
# here); at r = 1 and at S = 1 the up-sampled xyz is constant over the Sobel's window and the norm is sqrt(3e-6) = 0.0017, so that
# threshold only has to stay well away from it.
CASES = [
    (16, 64, 1, False, False, 0.25, 0.125, 0.455, 16065),  # integer ratio, N S S a multiple of 256
    (5, 37, 2, False, True, 0.25, 0.075, 0.465, 5039),  # ragged, partial last workgroup
    (37, 96, 3, True, True, 0.25, 0.185, 0.455, 37099),  # non-integer ratio, shared illustration
    (20, 12, 2, True, False, 0.25, 0.185, 0.495, 20014),  # down-sampling, r > S
    (1, 8, 2, False, True, 0.25, 0.05, 0.275, 1010),  # every tap clamps
    (3, 3, 1, False, False, 0.25, 0.385, 0.305, 3004),  # identity size: the border ring is 8 of 9 pixels
    (4, 1, 1, False, False, 0.25, 0.05, 0.695, 4010),  # one output pixel
    (2, 5, 3, False, True, 0.25, 0.175, 0.445, 2008),  # three views with their own rays and illustrations
    (7, 33, 2, False, False, 0.6, 0.265, 0.805, 7035),  # most samples beyond the illustration: the bx / by taps and the clamp
    (32, 128, 2, True, True, 0.25, 0.135, 0.475, 32130),  # the production ratio of 4
]
CLAMPED_CASE = 8
CASE_IDS = [f"r{c[0]}-S{c[1]}-N{c[2]}" for c in CASES]
BINARY = ("mask_weights", "mask_edges", "mask_dxyz")
CONTINUOUS = ("mask_occ", "mask", "paste", "image")


def case_thresholds(case):
    return (THRESH_WEIGHT, case[6], THRESH_OCC, case[7])


def case_inputs(case):
    """Seeded as tests/test_hip_paste_grad._forward draws them (same order from one CPU generator), rays_o scaled by 0.3 so that the
    discrepancy is of the order of box_warp; the illustration is white noise in [0, 1]."""
    r, S, N, shared, _, scale = case[:6]
    g = torch.Generator().manual_seed(case[8])
    xyz = torch.randn(N, 3, r, r, generator=g) * scale
    front = torch.rand(1 if shared else N, 3, S, S, generator=g)
    weights, occ = torch.rand(N, 1, r, r, generator=g), torch.rand(N, 1, r, r, generator=g)
    ro, rd = torch.randn(N, 3, r, r, generator=g) * 0.3, F.normalize(torch.randn(N, 3, r, r, generator=g), dim=1)
    image = torch.randn(N, 3, S, S, generator=g)
    return dict(weights=weights, xyz=xyz, occ=occ, rays_o=ro, rays_d=rd, front=front, image=image)


def nearest_index(S, r, coords="binary32"):
    """F.interpolate(mode='nearest') r -> S: min(int(i * (r / S)), r - 1), the product and the ratio in binary32 or in float64."""
    dt = torch.float32 if coords == "binary32" else torch.float64
    scale = torch.tensor(r, dtype=dt) / torch.tensor(S, dtype=dt)
    return (torch.arange(S, dtype=dt) * scale).to(torch.int64).clamp_max(r - 1)


def _taps(S, r, coords):
    """(i0, i1, l float64, source coordinate float64) of the r -> S bilinear resize (align_corners=False)."""
    if coords == "binary32":
        i0, i1, l = up_taps(S, r)
        return i0, i1, l.double(), i0.double() + l.double()
    i = torch.arange(S, dtype=torch.float64)
    src = ((i + 0.5) * (r / S) - 0.5).clamp_min(0.0)
    i0 = src.to(torch.int64).clamp_max(r - 1)
    return i0, (i0 + 1).clamp_max(r - 1), src - i0.double(), src


def _sum_tol(K, absterms):
    return GATE_C * math.sqrt(K) * EPS32 * absterms


def _coord_tol(src):
    return 2.0 * 2.0 ** -23 * src.abs().clamp_min(1.0)


def _up(m, ty, tx):
    """The up-sampled map [..., S, S] of m [..., r, r] in float64 and its allowance: the sum part of the four-term blend plus, per axis,
    the coordinate's allowance times the largest difference between the taps it blends (those of the neighbouring cell included where
    the coordinate lies within its allowance of that cell)."""
    r = m.shape[-1]
    (y0, y1, ly, sy), (x0, x1, lx, sx) = ty, tx
    val = _bilerp(m, (y0, y1, ly), (x0, x1, lx))
    tol = _sum_tol(4, _bilerp(m.abs(), (y0, y1, ly), (x0, x1, lx)))
    cy, cx = _coord_tol(sy), _coord_tol(sx)
    g = lambda yy, xx: m[..., yy[:, None], xx[None, :]]
    cl = lambda t: t.clamp(0, r - 1)
    # along y: rows (y0, y1) at the columns x0 and x1; the neighbouring cells are rows (y0 - 1, y0) and (y1, y1 + 1)
    dy = lambda a, b: torch.maximum((g(a, x0) - g(b, x0)).abs(), (g(a, x1) - g(b, x1)).abs())
    dY = dy(y0, y1)
    dY = torch.where((ly <= cy)[:, None], torch.maximum(dY, dy(cl(y0 - 1), y0)), dY)
    dY = torch.where((ly >= 1 - cy)[:, None], torch.maximum(dY, dy(y1, cl(y1 + 1))), dY)
    dx = lambda a, b: torch.maximum((g(y0, a) - g(y0, b)).abs(), (g(y1, a) - g(y1, b)).abs())
    dX = dx(x0, x1)
    dX = torch.where((lx <= cx)[None, :], torch.maximum(dX, dx(cl(x0 - 1), x0)), dX)
    dX = torch.where((lx >= 1 - cx)[None, :], torch.maximum(dX, dx(x1, cl(x1 + 1))), dX)
    return val, tol + cy[:, None] * dY + cx[None, :] * dX


def paste_forward_ref(weights, xyz, occ, rays_o, rays_d, front, image, thresholds, box_warp, normalize_images, coords="binary32"):
    """Float64 restatement of paste_front (training/triplane.py:553-691) on binary32 inputs.  coords='binary32': the quantities that
    are functions of the integers S and r alone — the bilinear taps (i0, i1, l) and the nearest index — take their binary32 values;
    everything that depends on data is float64.  coords='float64': those in float64 too (what float64 torch computes).  The thresholds
    are compared as the binary32 numbers the kernel receives.

    Returns a dict: 'weights' / 'edges' / 'occ' / 'dxyz' -> (continuous quantity before its threshold, allowance), each [N,1,S,S];
    'mask_weights' / 'mask_edges' / 'mask_dxyz' -> (0/1 mask, undecided pixels); 'mask_occ' / 'mask' / 'paste' / 'image' ->
    (value, allowance); 'decided' -> the pixels at which all three binary masks are decided; 'clamped' -> the pixels whose sampling
    coordinate was clamped to the illustration's border in x or y."""
    d = lambda t: torch.as_tensor(t).detach().cpu().double()
    weights, xyz, occ, rays_o, rays_d, front, image = (d(t) for t in (weights, xyz, occ, rays_o, rays_d, front, image))
    tw, te, to, td = (float(torch.tensor(t, dtype=torch.float32)) for t in thresholds)
    bw = float(torch.tensor(box_warp, dtype=torch.float32))
    N, _, r, _ = xyz.shape
    S = image.shape[-1]
    t = _taps(S, r, coords)
    res = {}
    # visible weight: interpolate(image_weights) > thresh_weight
    res["weights"] = _up(weights, t, t)
    # front occlusion: interpolate((occ < thresh_occ).float()), fractional
    res["occ"] = _up((occ < to).double(), t, t)
    # crevices: the norm over the three channels of sobel(interpolate(xyz)); 3x3 kernels / 8 on the replicate-padded image
    up, up_tol = _up(xyz, t, t)
    i = torch.arange(S)
    nb = [(i - 1).clamp_min(0), i, (i + 1).clamp_max(S - 1)]
    v = [[up[..., nb[a][:, None], nb[b][None, :]] for b in range(3)] for a in range(3)]
    vt = [[up_tol[..., nb[a][:, None], nb[b][None, :]] for b in range(3)] for a in range(3)]
    gx = ((v[0][2] - v[0][0]) + 2.0 * (v[1][2] - v[1][0]) + (v[2][2] - v[2][0])) * 0.125
    gy = ((v[2][0] - v[0][0]) + 2.0 * (v[2][1] - v[0][1]) + (v[2][2] - v[0][2])) * 0.125
    ax = (v[0][2].abs() + v[0][0].abs() + 2.0 * (v[1][2].abs() + v[1][0].abs()) + v[2][2].abs() + v[2][0].abs()) * 0.125
    ay = (v[2][0].abs() + v[0][0].abs() + 2.0 * (v[2][1].abs() + v[0][1].abs()) + v[2][2].abs() + v[0][2].abs()) * 0.125
    gx_tol = _sum_tol(6, ax) + (vt[0][2] + vt[0][0] + 2.0 * (vt[1][2] + vt[1][0]) + vt[2][2] + vt[2][0]) * 0.125
    gy_tol = _sum_tol(6, ay) + (vt[2][0] + vt[0][0] + 2.0 * (vt[2][1] + vt[0][1]) + vt[2][2] + vt[0][2]) * 0.125
    q2 = (gx * gx + gy * gy + 1e-6).sum(1, keepdim=True)  # >= 3e-6
    q2_tol = _sum_tol(9, q2) + (2.0 * gx.abs() * gx_tol + 2.0 * gy.abs() * gy_tol).sum(1, keepdim=True)
    q = q2.sqrt()
    res["edges"] = (q, q2_tol / (2.0 * q))
    # xyz discrepancy: the distance of the rendered point (xyz * (-1, 1, -1)) from its own ray, nearest-sampled
    p = xyz * torch.tensor([-1.0, 1.0, -1.0], dtype=torch.float64)[None, :, None, None]
    dv = p - rays_o
    dot = (dv * rays_d).sum(1, keepdim=True)
    adot = (dv * rays_d).abs().sum(1, keepdim=True)
    e = dv - dot * rays_d
    e_tol = _sum_tol(5, dv.abs() + adot * rays_d.abs())
    d2 = (e * e).sum(1, keepdim=True)
    d2_tol = _sum_tol(3, d2) + (2.0 * e.abs() * e_tol).sum(1, keepdim=True)
    dist = d2.sqrt()
    dist_tol = d2_tol / (2.0 * dist.clamp_min(1e-300))
    n = nearest_index(S, r, coords)
    res["dxyz"] = tuple(a[..., n[:, None], n[None, :]] for a in (dist, dist_tol))
    # the masks and the pixels at which each is decided
    for name, key, thr, passes in (("mask_weights", "weights", tw, lambda a, b: a > b), ("mask_edges", "edges", te, lambda a, b: a < b),
                                   ("mask_dxyz", "dxyz", td, lambda a, b: a < b)):
        val, tol = res[key]
        res[name] = (passes(val, thr).double(), (val - thr).abs() <= tol)
    res["mask_occ"] = res["occ"]
    decided = ~(res["mask_weights"][1] | res["mask_edges"][1] | res["mask_dxyz"][1])
    res["decided"] = decided
    binary = res["mask_weights"][0] * res["mask_edges"][0] * res["mask_dxyz"][0]
    mask, mask_tol = binary * res["occ"][0], binary * res["occ"][1]
    res["mask"] = (mask, mask_tol)
    # sample_orthofront: vij = 1 - (xyz[[1, 0]] + bw / 2) / bw, grid = vij * 2 - 1 on the TRANSPOSED illustration, bilinear, border
    # padding, align_corners=False: ix = clamp(((gx + 1) S - 1) / 2, 0, S - 1) from the up-sampled y, iy from the up-sampled x
    tocopy = front * 2.0 - 1.0 if normalize_images else front
    if tocopy.shape[0] == 1 and N > 1:
        tocopy = tocopy.expand(N, -1, -1, -1)
    tr = tocopy.transpose(2, 3)  # tr[n, c, row, col] = tocopy[n, c, col, row]
    coord = lambda u: (((1.0 - (u + bw / 2) / bw) * 2.0 - 1.0 + 1.0) * S - 1.0) / 2.0
    ix_u, iy_u = coord(up[:, 1]), coord(up[:, 0])
    ix_tol = up_tol[:, 1] * (S / bw) + _coord_tol(ix_u)
    iy_tol = up_tol[:, 0] * (S / bw) + _coord_tol(iy_u)
    res["clamped"] = (~((ix_u > 0) & (ix_u < S - 1)) | ~((iy_u > 0) & (iy_u < S - 1)))[:, None]
    ix, iy = ix_u.clamp(0, S - 1), iy_u.clamp(0, S - 1)
    x0, y0 = ix.floor(), iy.floor()
    tx, ty = (ix - x0)[:, None], (iy - y0)[:, None]
    x0, y0 = x0.long(), y0.long()
    flat = tr.reshape(N, 3, S * S)

    def at(yy, xx):  # the transposed illustration at (row yy, column xx), the border replicated
        idx = (yy.clamp(0, S - 1) * S + xx.clamp(0, S - 1)).reshape(N, 1, S * S).expand(-1, 3, -1)
        return flat.gather(2, idx).reshape(N, 3, S, S)
    terms = [at(y0, x0) * (1 - tx) * (1 - ty), at(y0, x0 + 1) * tx * (1 - ty), at(y0 + 1, x0) * (1 - tx) * ty, at(y0 + 1, x0 + 1) * tx * ty]
    paste = sum(terms)
    paste_tol = _sum_tol(4, sum(a.abs() for a in terms))
    # 3 x 3 cells = 4 x 4 texels around the sampled cell: the largest difference between neighbours along x and along y
    tex = [[at(y0 + a, x0 + b) for b in range(-1, 3)] for a in range(-1, 3)]
    dX = torch.stack([(tex[a][b + 1] - tex[a][b]).abs() for a in range(4) for b in range(3)]).amax(0)
    dY = torch.stack([(tex[a + 1][b] - tex[a][b]).abs() for a in range(3) for b in range(4)]).amax(0)
    paste_tol = paste_tol + ix_tol[:, None] * dX + iy_tol[:, None] * dY
    res["paste"] = (paste, paste_tol)
    # torch.lerp(image, paste, mask)
    out = image + mask * (paste - image)
    out_tol = _sum_tol(3, image.abs() + mask * (paste.abs() + image.abs())) + mask * paste_tol + (paste - image).abs() * mask_tol
    res["image"] = (out, out_tol)
    return res


def case_reference(case, coords="binary32", _memo={}):
    """The case's inputs and its restatement, computed once per process and shared (never modified)."""
    key = (case, coords)
    if key not in _memo:
        inp = case_inputs(case)
        _memo[key] = (inp, paste_forward_ref(**inp, thresholds=case_thresholds(case), box_warp=BW, normalize_images=case[4], coords=coords))
    return _memo[key]


def undecided(ref):
    """mask name -> number of undecided pixels."""
    return {k: int(ref[k][1].sum()) for k in BINARY}


def undecided_cap(case):
    px = case[2] * case[1] * case[1]
    return 0 if px < SMALL_CASE else int(UNDECIDED_SHARE * px)


def gate(ours, ref):
    """ours: name -> tensor (the seven outputs).  Returns name -> worst ratio against the allowance (continuous outputs; <= 1 passes)
    or the number of decided pixels whose 0/1 value differs (binary masks; 0 passes).  `mask` and `image` are compared where all
    three binary masks are decided; where an allowance is zero the value must be exact."""
    rep = {}
    for k in BINARY:
        o = torch.as_tensor(ours[k]).detach().cpu().double()
        val, und = ref[k]
        rep[k] = int((((o != val) & ~und) | ~((o == 0) | (o == 1))).sum())
    for k in CONTINUOUS:
        o = torch.as_tensor(ours[k]).detach().cpu().double()
        val, tol = ref[k]
        diff = (o - val).abs()
        ratio = torch.where(tol > 0, diff / tol.clamp_min(1e-300), torch.where(diff > 0, math.inf, 0.0))
        ratio = torch.where(torch.isfinite(o), ratio, torch.full_like(ratio, math.inf))
        if k in ("mask", "image"):
            ratio = ratio * ref["decided"]
        rep[k] = float(ratio.max())
    return rep


def gate_failures(rep):
    return [k for k, v in rep.items() if (v > 0 if k in BINARY else v > 1.0)]


# ---- the same composition in torch (binary32 on CPU: a legitimate result; float64: what the restatement must equal) ------------------
FAULTS = ("sobel_zero_pad", "sobel_centre_1", "nearest_rounded", "occ_after", "no_sign", "rays_view0", "front_view0", "swap_xy",
          "not_transposed", "zeros_padding", "align_corners")


def _sobel(x, pad, centre, eps=1e-6):
    xp = F.pad(x, [1, 1, 1, 1], mode=pad)
    tl, tc, tr = xp[..., :-2, :-2], xp[..., :-2, 1:-1], xp[..., :-2, 2:]
    ml, mr = xp[..., 1:-1, :-2], xp[..., 1:-1, 2:]
    bl, bc, br = xp[..., 2:, :-2], xp[..., 2:, 1:-1], xp[..., 2:, 2:]
    gx = ((tr - tl) + centre * (mr - ml) + (br - bl)) * 0.125
    gy = ((bl - tl) + centre * (bc - tc) + (br - tr)) * 0.125
    return torch.sqrt(gx * gx + gy * gy + eps)


def paste_forward_torch(weights, xyz, occ, rays_o, rays_d, front, image, thresholds, box_warp, normalize_images, dtype=torch.float32,
                        fault=None):
    """paste.paste_front_torch's composition (F.interpolate, paste.sobel_magnitude, paste.xyz_discrepancy, paste.sample_orthofront,
    torch.lerp) on given maps, in `dtype` on CPU.  Returns the seven outputs and, under 'q', the four continuous quantities.
    fault: one of FAULTS, the seeded faults the gate must catch."""
    from panic3d_amd import paste
    assert fault is None or fault in FAULTS
    c = lambda t: torch.as_tensor(t).detach().cpu().to(dtype)
    weights, xyz, occ, rays_o, rays_d, front, image = (c(t) for t in (weights, xyz, occ, rays_o, rays_d, front, image))
    tw, te, to, td = (float(torch.tensor(t, dtype=torch.float32)) for t in thresholds)
    bw = float(torch.tensor(box_warp, dtype=torch.float32))
    N, S, r = xyz.shape[0], image.shape[-1], xyz.shape[-1]
    up = lambda m: F.interpolate(m, S, mode="bilinear", align_corners=(fault == "align_corners"))
    q = {"weights": up(weights)}
    up_xyz = up(xyz)
    if fault == "sobel_zero_pad":
        sob = _sobel(up_xyz, "constant", 2.0)
    elif fault == "sobel_centre_1":
        sob = _sobel(up_xyz, "replicate", 1.0)
    else:
        sob = paste.sobel_magnitude(up_xyz)
    q["edges"] = sob.norm(2, dim=1, keepdim=True)
    q["occ"] = up(occ) if fault == "occ_after" else up((occ < to).to(dtype))
    if fault == "rays_view0":
        rays_o, rays_d = rays_o[:1].expand(N, -1, -1, -1), rays_d[:1].expand(N, -1, -1, -1)
    if fault == "no_sign":
        a = xyz - rays_o
        disc = (a - (a * rays_d).sum(dim=1, keepdim=True) * rays_d).norm(2, dim=1, keepdim=True)
    else:
        disc = paste.xyz_discrepancy(xyz, {"ray_origins": rays_o, "ray_directions": rays_d})
    if fault == "nearest_rounded":
        n = torch.round(torch.arange(S, dtype=torch.float32) * (torch.tensor(r, dtype=torch.float32) / S)).long().clamp_max(r - 1)
        q["dxyz"] = disc[..., n[:, None], n[None, :]]
    else:
        q["dxyz"] = F.interpolate(disc, S, mode="nearest")
    wmask, smask, dmask = (q["weights"] > tw).to(dtype), (q["edges"] < te).to(dtype), (q["dxyz"] < td).to(dtype)
    fmask = (q["occ"] < to).to(dtype) if fault == "occ_after" else q["occ"]
    mask = wmask * smask * fmask * dmask
    tocopy = front * 2 - 1 if normalize_images else front
    if fault == "front_view0":
        tocopy = tocopy[:1]
    if tocopy.shape[0] == 1 and N > 1:
        tocopy = tocopy.expand(N, -1, -1, -1)
    if fault in ("swap_xy", "not_transposed", "zeros_padding"):
        vij = 1 - (up_xyz[:, [0, 1] if fault == "swap_xy" else [1, 0]] + bw / 2) / bw
        src = tocopy if fault == "not_transposed" else tocopy.permute(0, 1, 3, 2)
        pst = F.grid_sample(src, vij.permute(0, 2, 3, 1) * 2 - 1, padding_mode="zeros" if fault == "zeros_padding" else "border",
                            mode="bilinear", align_corners=False)
    else:
        pst = paste.sample_orthofront(tocopy, up_xyz, bw)
    return {"image": torch.lerp(image, pst, mask), "paste": pst, "mask": mask, "mask_weights": wmask, "mask_edges": smask,
            "mask_occ": fmask, "mask_dxyz": dmask, "q": q}


# ---- ties: values exactly on a threshold ---------------------------------------------------------------------------------------------
def ties_case():
    """r = S = 4, one view: the taps have l = 0 exactly, so every up-sampled value is the source value bit for bit, and the expected
    masks can be written by hand.  Row y of the weights: equal to thresh_weight (0: the comparison is a strict >), the next binary32
    above (1), the next below (0), 1.0 (1).  Column x of occ: equal to thresh_occ (0: strict <), the next below (1), the next above
    (0), 0.0 (1).  Discrepancy by (y + x) % 3 with rays_d = (0, 0, 1), rays_o = 0: p = (3/16, 4/16, z) is at exactly 5/16 =
    thresh_dxyz from the ray (0: strict <); p scaled by (1 - 2^-22) in x and y passes (1), by (1 + 2^-22) does not (0).  (The
    neighbouring binary32 of 3/16 or 4/16 alone need not move the ROUNDED distance off 5/16: the four roundings on the way — two
    squares, a sum, a root — are worth up to 2 ulps, so the passing pixel stands 4 ulps away.)  thresh_edges is out of reach (1e3): every
    pixel passes.  Returns (inputs, thresholds, expected masks)."""
    f32 = torch.float32
    S = 4
    tw, to, td = torch.tensor(THRESH_WEIGHT, dtype=f32), torch.tensor(THRESH_OCC, dtype=f32), torch.tensor(5.0 / 16.0, dtype=f32)
    inf = torch.tensor(math.inf, dtype=f32)
    wrow = torch.stack([tw, torch.nextafter(tw, inf), torch.nextafter(tw, -inf), torch.tensor(1.0)])
    ocol = torch.stack([to, torch.nextafter(to, -inf), torch.nextafter(to, inf), torch.tensor(0.0)])
    weights = wrow[:, None].expand(S, S).reshape(1, 1, S, S).contiguous()
    occ = ocol[None, :].expand(S, S).reshape(1, 1, S, S).contiguous()
    yy, xx = torch.meshgrid(torch.arange(S), torch.arange(S), indexing="ij")
    kind = (yy + xx) % 3
    eps = 2.0 ** -22
    fac = torch.where(kind == 0, 1.0, torch.where(kind == 1, 1.0 - eps, 1.0 + eps)).to(f32)
    g = torch.Generator().manual_seed(44)
    z = torch.randn(S, S, generator=g)
    # xyz * (-1, 1, -1) = p
    xyz = torch.stack([-(3.0 / 16.0) * fac, (4.0 / 16.0) * fac, -z])[None].contiguous()
    assert torch.equal(xyz[0, 0].double(), -(3.0 / 16.0) * fac.double()) and torch.equal(xyz[0, 1].double(), 0.25 * fac.double())  # exact in binary32
    rd = torch.zeros(1, 3, S, S)
    rd[:, 2] = 1.0
    inputs = dict(weights=weights, xyz=xyz, occ=occ, rays_o=torch.zeros(1, 3, S, S), rays_d=rd,
                  front=torch.rand(1, 3, S, S, generator=g), image=torch.randn(1, 3, S, S, generator=g))
    m = lambda t: t.to(f32).reshape(1, 1, S, S)
    expect = {"mask_weights": m(torch.tensor([0.0, 1.0, 0.0, 1.0])[:, None].expand(S, S)),
              "mask_occ": m(torch.tensor([0.0, 1.0, 0.0, 1.0])[None, :].expand(S, S)),
              "mask_dxyz": m(kind == 1), "mask_edges": torch.ones(1, 1, S, S)}
    expect["mask"] = expect["mask_weights"] * expect["mask_edges"] * expect["mask_occ"] * expect["mask_dxyz"]
    return inputs, (THRESH_WEIGHT, 1e3, THRESH_OCC, 5.0 / 16.0), expect


def check_ties(ours, inputs, expect):
    """The five masks equal to the hand-written ones; where the mask is 0 the image keeps its bits, where it is 1 it takes the paste's
    (torch.lerp's two branches are exact at w = 0 and w = 1)."""
    for k, want in expect.items():
        assert torch.equal(torch.as_tensor(ours[k]).cpu().float(), want), (k, ours[k], want)
    m = expect["mask"].expand(-1, 3, -1, -1)
    assert 0 < int(m.sum()) < m.numel()
    img, pst = torch.as_tensor(ours["image"]).cpu(), torch.as_tensor(ours["paste"]).cpu()
    assert torch.equal(img[m == 0], inputs["image"][m == 0]) and torch.equal(img[m == 1], pst[m == 1])
