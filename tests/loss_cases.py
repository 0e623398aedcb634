"""Cases of the training loss (panic3d_amd/loss.py, include/p3d_loss.h), shared by tests/test_loss_cpu.py, tests/test_hip_loss.py and
tests/golden/make_golden_loss.py:

  * float64 restatements of the three operators, written from the formulas of include/p3d_loss.h (with seedable faults, so that the
    tests can show that their gates notice them);
  * the gates;
  * torch stand-ins of the operators for CPU runs and install_ops(monkeypatch, ops);
  * the stand-in G, D and lpips_model and the seeded phase cases on which the reference's loss and this package's are compared.
"""
import math

import numpy as np
import torch

F = torch.nn.functional
EPS32 = 2.0 ** -24
GATE_C = 8.0
REL_L2 = 1e-5


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double().ravel().cpu(), torch.as_tensor(b).double().ravel().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def gate_ratio(ours, ref, absref, K):
    """max over elements of |ours - ref| / (sqrt(K) 2^-24 absref); an element with absref == 0 must be exact (else inf)."""
    d = (torch.as_tensor(ours).double().cpu() - ref.double()).abs()
    scale = math.sqrt(max(K, 1)) * EPS32 * absref.double()
    r = torch.where(scale > 0, d / scale.clamp_min(1e-300), torch.where(d > 0, math.inf, 0.0))
    return float(r.max()) if r.numel() else 0.0


def gate(name, ours, ref, absref, K, keep=None, verbose=True):
    """The project's gate for one tensor: per value 8 sqrt(K) 2^-24 sum|terms|, and rel-L2 <= 1e-5 (a tensor that is zero everywhere
    must be matched exactly).  keep: a boolean mask of the values compared.  Returns the list of violations."""
    ours = torch.as_tensor(ours).double().cpu().reshape(ref.shape)
    if keep is not None:
        ours, ref, absref = ours[keep], ref[keep], absref[keep]
    r, e = gate_ratio(ours, ref, absref, K), rel_l2(ours, ref) if float(ref.abs().max() if ref.numel() else 0) > 0 else 0.0
    if verbose:
        print(f"gate {name}: worst {r:.3f} (c = {GATE_C:g}, K = {K}), rel-L2 {e:.2e}")
    return ([f"{name}: ratio {r:.3g}"] if not r <= GATE_C else []) + ([f"{name}: rel-L2 {e:.3g}"] if not e <= REL_L2 else [])


# ---- the blur -------------------------------------------------------------------------------------------------------------------------
def _pass_f64(x, f, axis):
    """sum over t of f[t] x[.. + t - R ..] along `axis` (-1: x, -2: y), zero outside."""
    T = f.numel()
    R = (T - 1) // 2
    n = x.shape[axis]
    out = torch.zeros_like(x)
    for t in range(T):
        s = t - R  # out[i] += f[t] x[i + s]
        lo, hi = max(0, -s), min(n, n - s)
        if lo >= hi:
            continue
        dst, src = [slice(None)] * x.ndim, [slice(None)] * x.ndim
        dst[axis], src[axis] = slice(lo, hi), slice(lo + s, hi + s)
        out[tuple(dst)] += f[t] * x[tuple(src)]
    return out


def blur_f64(x, f, fault=None):
    """p3d_blur_f32 in float64: the row pass, then the column pass.  fault 'transposed': the row pass runs along y as well."""
    x, f = x.double(), f.double()
    return _pass_f64(_pass_f64(x, f, -2 if fault == "transposed" else -1), f, -2)


def blur_adjoint_f64(g, f, fault=None):
    """The adjoint: the same operator with the flipped filter.  fault 'unflipped': with the filter as it is."""
    return blur_f64(g, f if fault == "unflipped" else f.flip(0))


def blur_absref(x, f):
    return blur_f64(x.abs(), f.abs())


def blur_torch(x, f):
    """upfirdn2d.py:197-209 on torch's convolution, in the dtype of x: what the reference computes (f given as the correlation's)."""
    T = f.numel()
    R = (T - 1) // 2
    shape = x.shape
    y = x.reshape(-1, 1, *shape[-2:])
    y = F.conv2d(F.pad(y, [R, R, R, R]), f.to(x.dtype).view(1, 1, 1, T))
    y = F.conv2d(y, f.to(x.dtype).view(1, 1, T, 1))
    return y.reshape(shape)


BLUR_TAPS = (1, 3, 61, 127)


def blur_shapes(tile):
    th, tw = tile
    return [(5, 7), (33, 31), (th + 1, tw + 1), (1, 70)]


def blur_filter(taps, seed=0):
    """An ASYMMETRIC filter of `taps` taps with mixed signs, sum of |f| = 1: a flipped or transposed pass is another operator."""
    g = torch.Generator().manual_seed(1000 + taps + seed)
    f = torch.rand(taps, generator=g) - 0.3
    f = f * torch.linspace(0.5, 1.5, taps)
    return (f / f.abs().sum()).float()


def blur_input(NC, H, W, seed=0):
    g = torch.Generator().manual_seed(seed + 7 * NC + 131 * H + W)
    return torch.randn(NC, H, W, generator=g), torch.randn(NC, H, W, generator=g)


# ---- L1 -------------------------------------------------------------------------------------------------------------------------------
def l1_f64(a, b, scale):
    d = a.double() - b.double()
    return dict(sum=d.abs().sum(), absref=(a.double().abs() + b.double().abs()).sum(), g_a=torch.sign(d) * np.float32(scale).astype(np.float64))


L1_K = 64  # a lane's chain (at most a few terms at the tests' sizes), two 8-level trees, the partials' chain


# ---- the view terms -------------------------------------------------------------------------------------------------------------------
def up_taps(r, S):
    """The bilinear taps of the S -> r resize as the kernel evaluates them, in binary32: (i0, i1, lambda)."""
    f32 = np.float32
    scale = f32(S) / f32(r)
    src = (np.arange(r, dtype=np.float32) + f32(0.5)) * scale - f32(0.5)
    src = np.maximum(src, f32(0))
    i0 = np.minimum(src.astype(np.int64), S - 1)
    i1 = np.minimum(i0 + 1, S - 1)
    lam = src - i0.astype(np.float32)
    return torch.from_numpy(i0), torch.from_numpy(i1), torch.from_numpy(lam.astype(np.float64))


def resize_f64(x, r):
    """[.., S, S] -> [.., r, r]: (1-ly) ((1-lx) v00 + lx v01) + ly ((1-lx) v10 + lx v11) in float64 on the binary32 taps."""
    S = x.shape[-1]
    i0, i1, lam = up_taps(r, S)
    x = x.double()
    rows0, rows1 = x[..., i0, :], x[..., i1, :]
    top = (1 - lam) * rows0[..., i0] + lam * rows0[..., i1]
    bot = (1 - lam) * rows1[..., i0] + lam * rows1[..., i1]
    ly = lam.view(-1, 1)
    return (1 - ly) * top + ly * bot


def box5_f64(a, tile=None):
    """The zero-padded 5 x 5 sum.  tile (a fault): the sum taken inside tile x tile blocks only, as a kernel without its halo would."""
    ones = torch.ones(1, 1, 5, 5, dtype=a.dtype)
    if tile is None:
        return F.conv2d(a, ones, padding=2)
    out = torch.zeros_like(a)
    r = a.shape[-1]
    for y0 in range(0, r, tile):
        for x0 in range(0, r, tile):
            out[..., y0:y0 + tile, x0:x0 + tile] = F.conv2d(a[..., y0:y0 + tile, x0:x0 + tile], ones, padding=2)
    return out


VT_K, VT_K_NORM, VT_K_SUM = 10, 16, 40  # roundings: the resize (7) + difference, product, scale; the norm's sqrt and division; the trees
VT_MARGIN = 1e-5
VT_TILE = 16


def view_terms_f64(weights, xyz, gt_alpha, gt_xyz, mode, q, s_alpha, s_depth, fault=None):
    """p3d_view_terms_f32 in float64, with sum|terms| for the gates and `tight`: the texels whose mask decision lies within VT_MARGIN of
    a threshold.  fault 'halo': the box filter without the tile's halo; 'mz': the depth term masked by m where mz belongs."""
    r = weights.shape[-1]
    w, x = weights.double(), xyz.double()
    a, g = resize_f64(gt_alpha, r), resize_f64(gt_xyz, r)
    gabs = resize_f64(gt_xyz.abs(), r)
    box = box5_f64(a, VT_TILE if fault == "halo" else None) / 25
    m = ((box - 0.5).abs() * 2 > 0.5)
    mz = m if fault == "mz" else m & (w > 0.5) & (a > 0.5)
    tight_m = torch.minimum((box - 0.25).abs(), (box - 0.75).abs()) < VT_MARGIN
    tight_z = tight_m | ((a - 0.5).abs() < VT_MARGIN) | ((w - 0.5).abs() < VT_MARGIN)
    if gt_alpha.shape[-1] % r == 0 and math.log2(gt_alpha.shape[-1] // r).is_integer() and float(gt_alpha.frac().abs().max()) == 0:
        # binary alphas resized by a power of two: every tap weight, resized alpha and box sum is exact in binary32, a value on a
        # threshold is on it in both precisions, and no texel is left out
        tight_m, tight_z = torch.zeros_like(tight_m), torch.zeros_like(tight_z)
    qv = torch.ones_like(w) if q is None else q.double()
    s_alpha, s_depth = float(np.float32(s_alpha)), float(np.float32(s_depth))
    dw = w - a
    t_alpha = dw * dw * m * qv
    g_w = s_alpha * 2 * dw * m * qv
    mzq = mz * qv
    e = x - g
    eabs = x.abs() + gabs
    g_x = torch.zeros_like(x)
    g_x_abs = torch.zeros_like(x)
    if mode == "norm":
        d = e.square().sum(1, keepdim=True).sqrt()
        t_depth = d * mzq
        t_depth_abs = eabs.square().sum(1, keepdim=True).sqrt() * mzq
        safe = torch.where(d > 0, d, torch.ones_like(d))
        g_x = torch.where(d > 0, s_depth * e / safe * mzq, torch.zeros_like(e))
        g_x_abs = torch.where(d > 0, abs(s_depth) * 2 * eabs.sum(1, keepdim=True) / safe * mzq, torch.zeros_like(e)).expand_as(e).clone()
    else:
        c = 2 if mode == "z" else 0
        t_depth = e[:, c:c + 1].square() * mzq
        t_depth_abs = eabs[:, c:c + 1].square() * mzq
        g_x[:, c:c + 1] = s_depth * 2 * e[:, c:c + 1] * mzq
        g_x_abs[:, c:c + 1] = abs(s_depth) * 2 * eabs[:, c:c + 1] * mzq
    wabs = w.abs() + a.abs()
    return dict(sums=torch.stack([t_alpha.sum(), t_depth.sum()]), sums_abs=torch.stack([(wabs * wabs * m * qv).sum(), t_depth_abs.sum()]),
                # what the texels left out of the comparison could add to or take from each sum, whichever way their masks fall
                sums_slack=torch.stack([(dw * dw * qv * tight_m).sum(), ((d if mode == "norm" else e[:, c:c + 1].square()) * qv * tight_z).sum()]),
                g_w=g_w, g_w_abs=abs(s_alpha) * 2 * wabs * m * qv, g_x=g_x, g_x_abs=g_x_abs, tight_m=tight_m, tight_z=tight_z, m=m, mz=mz, a=a, g=g)


def view_terms_gate(got, ref, mode, verbose=True):
    """got: dict(sums [2], g_w, g_x) of an implementation; ref: view_terms_f64's.  The tight texels are left out of the gradients'
    comparison and their possible terms are allowed on the sums."""
    bad = []
    d = (torch.as_tensor(got["sums"]).double().cpu() - ref["sums"]).abs()
    allow = GATE_C * math.sqrt(VT_K_SUM) * EPS32 * ref["sums_abs"] + ref["sums_slack"]
    if verbose:
        print(f"sums: |diff| {d.tolist()} allowed {allow.tolist()}")
    bad += [f"sums[{i}]" for i in range(2) if not d[i] <= allow[i]]
    bad += gate("g_w", got["g_w"], ref["g_w"], ref["g_w_abs"], VT_K, keep=~ref["tight_m"], verbose=verbose)
    bad += gate("g_x", got["g_x"], ref["g_x"], ref["g_x_abs"], VT_K_NORM if mode == "norm" else VT_K, keep=~ref["tight_z"].expand_as(ref["g_x"]),
                verbose=verbose)
    return bad


def view_terms_f32(weights, xyz, gt_alpha, gt_xyz, mode, q, s_alpha, s_depth, fault=None):
    """The float64 restatement rounded to binary32: a correct implementation for the gates' own tests."""
    ref = view_terms_f64(weights, xyz, gt_alpha, gt_xyz, mode, q, s_alpha, s_depth, fault=fault)
    return {k: ref[k].float() for k in ("sums", "g_w", "g_x")}


VT_SHAPES = ((32, 8), (20, 6), (9, 9), (33, 8), (40, 19))  # (S, r); the last one spans more than one 16 x 16 tile
VT_MAX_TIGHT = 0.01


def blob_alpha(N, S, seed):
    """Binary alphas made of two overlapping discs per sample: large flat regions, so that the box mask is true over much of the map."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(S, dtype=torch.float32), torch.arange(S, dtype=torch.float32), indexing="ij")
    out = torch.zeros(N, 1, S, S)
    for n in range(N):
        for _ in range(2):
            cy, cx = (torch.rand(2, generator=g) * 0.3 + 0.35) * S
            rad = (torch.rand((), generator=g) * 0.12 + 0.3) * S
            out[n, 0] = torch.maximum(out[n, 0], ((yy - cy) ** 2 + (xx - cx) ** 2 < rad * rad).float())
    return out


def view_terms_case(S, r, with_q, seed=0, N=2):
    g = torch.Generator().manual_seed(50 + 1000 * S + r + seed)
    gt_alpha = blob_alpha(N, S, 60 + S + r + seed)
    gt_xyz = torch.randn(N, 3, S, S, generator=g) * 0.3
    # as a render's would, the weights follow the alpha: the three masks overlap
    weights = 0.5 * F.interpolate(gt_alpha, r, mode="bilinear") + 0.55 * torch.rand(N, 1, r, r, generator=g)
    up = F.interpolate(gt_xyz, r, mode="bilinear")
    xyz = up + torch.randn(N, 3, r, r, generator=g) * 0.05
    xyz[:, :, 0, 0] = up[:, :, 0, 0]  # (almost) zero distance at one texel: the norm mode's guarded division
    q = (torch.rand(N, 1, r, r, generator=g) > 0.3).float() if with_q else None
    return dict(weights=weights, xyz=xyz, gt_alpha=gt_alpha, gt_xyz=gt_xyz, q=q)


# ---- torch stand-ins of the operators (CPU runs of the host wiring) -------------------------------------------------------------------
def blur_impl_torch(x, f):
    return blur_torch(x, f)


def l1_impl_torch(a, b, scale, want_grad):
    d = a - b
    return d.abs().mean(), (torch.sign(d) * scale if want_grad else None)


def view_terms_impl_torch(weights, xyz, gt_alpha, gt_xyz, depth_mode, q, want_grad):
    """The reference's own sequence of torch calls (loss_orthocondA.py:287-308 and its siblings) in binary32, the gradients from
    autograd."""
    r = weights.shape[-1]
    with torch.enable_grad():
        w, x = weights.detach().requires_grad_(True), xyz.detach().requires_grad_(True)
        a = F.interpolate(gt_alpha, r, mode="bilinear")
        m = F.conv2d(a, torch.ones(1, 1, 5, 5, device=a.device, dtype=a.dtype), stride=1, padding=2) / 25
        m = (m - 0.5).abs() * 2 > 0.5
        qv = 1.0 if q is None else q
        t_alpha = (w - a).pow(2).mul(m.float() * qv).mean()
        g = F.interpolate(gt_xyz, r, mode="bilinear")
        mz = (m & (w > 0.5) & (a > 0.5)).detach()
        if depth_mode == "norm":
            t_depth = ((x - g).pow(2).sum(dim=1) + 0.0).sqrt().mul((mz.float() * qv)[:, 0]).mean()
        else:
            c = 2 if depth_mode == "z" else 0
            t_depth = (x[:, c] - g[:, c]).pow(2).mul((mz.float() * qv)[:, 0]).mean()
        gw = gx = None
        if want_grad:
            gw, = torch.autograd.grad(t_alpha, w)
            gx, = torch.autograd.grad(t_depth, x)
            gx = torch.nan_to_num(gx, nan=0.0)  # distance exactly 0: include/p3d_loss.h gives 0 where autograd gives NaN
    return torch.stack([t_alpha.detach(), t_depth.detach()]), gw, gx


def install_ops(monkeypatch, ops):
    for name, fn in dict(_blur_impl=blur_impl_torch, _l1_impl=l1_impl_torch, _view_terms_impl=view_terms_impl_torch).items():
        monkeypatch.setattr(ops, name, fn)


# ---- the stand-in networks and the phase cases ----------------------------------------------------------------------------------------
N, S, RES, Z_DIM, C_DIM, W_DIM, NUM_WS, BOX_WARP = 2, 32, 8, 6, 25, 5, 4, 1.0
VIEWS = ("front", "left", "right", "back")


class StandInG(torch.nn.Module):
    """f() returns seeded leaf parameters (times a factor of the styles when it is given ws, so that run_G's draws show in the result);
    mapping is a fixed map of z and c; sample_mixed a smooth function of the coordinates, the directions and the styles."""

    def __init__(self, rendering_kwargs, seed=1):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        P = torch.nn.Parameter
        self.image = P(torch.randn(N, 3, S, S, generator=g) * 0.5)
        self.image_raw = P(torch.randn(N, 3, RES, RES, generator=g) * 0.5)
        self.image_weights = P(torch.rand(N, 1, RES, RES, generator=g))
        self.image_xyz = P((torch.rand(N, 3, RES, RES, generator=g) - 0.5) * BOX_WARP)
        self.map_z = P(torch.randn(Z_DIM, W_DIM, generator=g) * 0.5)
        self.map_c = P(torch.randn(C_DIM, W_DIM, generator=g) * 0.2)
        self.sig_a = P(torch.randn(3, 4, generator=g))
        self.rendering_kwargs = dict(rendering_kwargs)
        self.cond_mode = "ortho_front.stand_in"
        self.z_dim, self.c_dim, self.w_dim = Z_DIM, C_DIM, W_DIM

    def mapping(self, z, c, cond, truncation_psi=1, truncation_cutoff=None, update_emas=False):
        w = torch.tanh(z @ self.map_z + c @ self.map_c)
        return w.unsqueeze(1).repeat(1, NUM_WS, 1) * torch.linspace(0.5, 1.5, NUM_WS, device=w.device).view(1, -1, 1)

    def f(self, x):
        k = 1 + 0.1 * x["ws"].mean(dim=(1, 2)).view(-1, 1, 1, 1) if "ws" in x else 1
        xyz = self.image_xyz * k
        if "ws" not in x:  # a supervised view: near the view's ground truth, so that the depth terms see moderate residuals
            xyz = xyz * 0.2 + F.interpolate(x["cond"]["image_ortho_front_xyz"], RES, mode="bilinear")
        return {"image": self.image * k, "image_raw": self.image_raw * k, "image_weights": self.image_weights * k, "image_xyz": xyz}

    def sample_mixed(self, coordinates, directions, ws, cond, truncation_psi=1, truncation_cutoff=None, update_emas=False):
        s = torch.sin(coordinates @ self.sig_a).sum(-1, keepdim=True) + 0.1 * directions.sum(-1, keepdim=True)
        return {"sigma": s * (1 + ws.mean(dim=(1, 2)).view(-1, 1, 1))}


class StandInD(torch.nn.Module):
    """A seeded linear functional of image and image_raw."""

    def __init__(self, seed=2):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.w_image = torch.nn.Parameter(torch.randn(3, S, S, generator=g) * 0.02)
        self.w_raw = torch.nn.Parameter(torch.randn(3, RES, RES, generator=g) * 0.05)
        self.bias = torch.nn.Parameter(torch.tensor(0.1))

    def forward(self, img, c, cond, update_emas=False):
        return ((img["image"] * self.w_image).sum(dim=(1, 2, 3)) + (img["image_raw"] * self.w_raw).sum(dim=(1, 2, 3)) + self.bias).unsqueeze(1)


def lpips_stand_in(a, b):
    return (a - b).square().mean(dim=(1, 2, 3))


def loss_inputs(seed=3, device="cpu"):
    g = torch.Generator().manual_seed(seed)
    u = (torch.arange(S, dtype=torch.float32) + 0.5) / S - 0.5
    vv, uu = torch.meshgrid(u, u, indexing="ij")
    front_z = 0.2 * torch.cos(3 * uu) * torch.cos(3 * vv)
    cond = {}
    for i, view in enumerate(VIEWS):
        p = f"image_ortho_{view}"
        cond[p] = torch.rand(N, 3, S, S, generator=g)
        cond[p + "_alpha"] = blob_alpha(N, S, seed + 10 + i)
        cond[p + "_xyz"] = torch.stack([uu * BOX_WARP, vv * BOX_WARP, front_z]).expand(N, 3, S, S) + torch.randn(N, 3, S, S, generator=g) * 0.02
        cond[p + "_camera"] = torch.randn(N, C_DIM, generator=g)
    cond["image"] = torch.rand(N, 3, S, S, generator=g)
    cond["image_alpha"] = blob_alpha(N, S, seed + 20)
    # the view's points: on the front view's lattice (transposed roles, as mask_view_orthofront reads them), a little behind or before
    cond["image_xyz"] = torch.stack([vv * BOX_WARP, uu * BOX_WARP, front_z]).expand(N, 3, S, S) \
        + torch.randn(N, 3, S, S, generator=g) * torch.tensor([0.03, 0.03, 0.01]).view(1, 3, 1, 1)
    cond["image_camera"] = torch.randn(N, C_DIM, generator=g)
    inp = dict(real_img=torch.randn(N, 3, S, S, generator=g), real_c=torch.randn(N, C_DIM, generator=g), real_cond=cond,
               gen_z=torch.randn(N, Z_DIM, generator=g), gen_c=torch.randn(N, C_DIM, generator=g))
    to = lambda v: {k: to(x) for k, x in v.items()} if isinstance(v, dict) else v.to(device)
    return to(inp)


LAMBDAS = {f"lambda_{grp}_{t}": round(0.3 + 0.17 * i + 0.05 * j, 3)
           for i, grp in enumerate(("Gcond", "Gcond_sides", "Gcond_back", "Gcond_rand", "recon")) for j, t in enumerate(("lpips", "l1", "alpha_l2", "depth_l2"))}
LOSS_KW = dict(LAMBDAS, r1_gamma=10, blur_init_sigma=10, blur_fade_kimg=1, neural_rendering_resolution_initial=RES, gpc_reg_prob=0.5,
               gpc_reg_fade_kimg=1, dual_discrimination=True, filter_mode="antialiased")
NIMG = {"s10": 0, "s1.5": 850, "s0": 2000}  # cur_nimg -> blur sigma 10, 1.5 and 0 (blur_fade_kimg 1: sigma = 10 (1 - cur_nimg / 1000))
RK = dict(box_warp=BOX_WARP, density_reg=0.0, reg_type="l1", density_reg_p_dist=0.004)
GAIN = 1.7


def _case(phase, sig, rk=None, **kw):
    return dict(phase=phase, cur_nimg=NIMG[sig], rk=dict(RK, **(rk or {})), kw=dict(LOSS_KW, **kw))


MASKED = dict(lossmask_mode_adv="replace_3", lossmask_mode_recon="dilate_5", style_mixing_prob=0.5)
PHASE_CASES = {
    "Gcond": _case("Gcond", "s10"),
    "Gside-left": _case("Gside-left", "s10"),
    "Gside-right": _case("Gside-right", "s1.5"),
    "Gside-back": _case("Gside-back", "s0"),
    "Grand": _case("Grand", "s10"),
    **{f"Gmain-{s}": _case("Gmain", s, style_mixing_prob=0.5) for s in NIMG},
    **{f"Gmain-masked-{s}": _case("Gmain", s, **MASKED) for s in NIMG},
    "Gmain-recon-only": _case("Gmain", "s10", lossmask_mode_recon="dilate_3"),  # no adversarial mask: the blurred image is reconstructed
    **{f"Dmain-{s}": _case("Dmain", s) for s in NIMG},
    "Dboth-r1-0": _case("Dboth", "s10", r1_gamma=0),
    "Gboth-noreg": _case("Gboth", "s1.5", **MASKED),
    "Gboth-l1": _case("Gboth", "s10", rk=dict(density_reg=0.25, reg_type="l1"), lossmask_mode_recon="dilate_3"),
    "Greg-l1": _case("Greg", "s10", rk=dict(density_reg=0.25, reg_type="l1")),
    "Greg-monotonic-detach": _case("Greg", "s1.5", rk=dict(density_reg=0.5, reg_type="monotonic-detach")),
    "Greg-monotonic-fixed": _case("Greg", "s0", rk=dict(density_reg=0.5, reg_type="monotonic-fixed")),
}


def run_phase(loss_cls, case, capture, device="cpu", seed=11):
    """One accumulate_gradients call of `loss_cls` on the stand-ins: (reports: name -> tensor, gradients: name -> tensor over the
    leaves of G and D that received one).  capture(fn): installs fn(name, value) as the loss module's report hook."""
    G, D = StandInG(case["rk"]).to(device), StandInD().to(device)
    inp = loss_inputs(device=device)
    reports = {}

    def hook(name, value):
        reports[name] = torch.as_tensor(value).detach().clone().float().cpu()
        return value
    capture(hook)
    loss = loss_cls(device=torch.device(device), G=G, D=D, augment_pipe=None, lpips_model=lpips_stand_in, **case["kw"])
    torch.manual_seed(seed)
    loss.accumulate_gradients(phase=case["phase"], gain=GAIN, cur_nimg=case["cur_nimg"], **inp)
    grads = {f"{m}.{n}": p.grad.detach().cpu() for m, mod in (("G", G), ("D", D)) for n, p in mod.named_parameters() if p.grad is not None}
    return reports, grads


def draws_on_cpu(monkeypatch):
    """Take the loss's random draws (torch.rand, torch.randn_like, Tensor.random_) from the CPU's generator and move them to the device
    that was asked for: a seeded run on a GPU then sees the numbers of the reference's seeded CPU run."""
    rand, randn, random_ = torch.rand, torch.randn, torch.Tensor.random_

    def on_cpu_random_(self, *a, **k):
        return self.copy_(random_(torch.empty(self.shape, dtype=self.dtype), *a, **k))
    monkeypatch.setattr(torch, "rand", lambda *a, device=None, **k: rand(*a, **k).to(device))
    monkeypatch.setattr(torch, "randn_like", lambda t, **k: randn(t.shape, dtype=t.dtype).to(t.device))
    monkeypatch.setattr(torch.Tensor, "random_", on_cpu_random_)


def compare_with_fixture(golden, name, reports, grads):
    """The device test's bounds: reported values to 1e-5 relative (of the tensor's largest magnitude), gradients to rel-L2 <= 1e-4."""
    want_r = {k.split("|")[2]: v for k, v in golden.items() if k.startswith(f"{name}|report|")}
    want_g = {k.split("|")[2]: v for k, v in golden.items() if k.startswith(f"{name}|grad|")}
    assert set(reports) == set(want_r) and set(grads) == set(want_g), (name, sorted(reports), sorted(want_r), sorted(grads), sorted(want_g))
    for k, v in want_r.items():
        v = torch.from_numpy(v)
        err = float((reports[k].reshape(v.shape) - v).abs().max()) / max(float(v.abs().max()), 1e-30)
        print(f"{name} {k}: {err:.2e}")
        assert err <= 1e-5, (name, k, err)
    for k, v in want_g.items():
        v = torch.from_numpy(v)
        assert torch.isfinite(grads[k]).all()
        err = rel_l2(grads[k], v) if float(v.abs().max()) > 0 else float(grads[k].abs().max())
        print(f"{name} grad {k}: {err:.2e}")
        assert err <= 1e-4, (name, k, err)


def fixture_key(case_name, kind, name):
    return f"{case_name}|{kind}|{name}"
