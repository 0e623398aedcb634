"""Cases shared by the tests of the mapping network's and the front-view paste's backward (tests/test_mapping_grad_cpu.py,
tests/test_hip_mapping_grad.py, tests/test_hip_paste_grad.py) and by the generator of their fixtures
(tests/golden/make_golden_train_step.py): seeded parameters and inputs that either implementation of TriPlaneGenerator rebuilds bit for
bit, float64 restatements written from the formulas (not from the code under test), and torch stand-ins of the device operators so
that the host wiring runs on CPU."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from p3d_shared_cases import TRI_KW  # noqa: F401  (the generator of tests/golden/syn_triplane_f.npz)

EPS32 = 2.0 ** -24

# ---- mapping network ---------------------------------------------------------------------------------------------------------------
MAPPING_LAYERS = (2, 8)
PSI, CUTOFF, BATCH, RESNET_K = 0.7, 4, 3, 8


def mapping_kw(num_layers):
    return dict(TRI_KW, cond_mode=f"resnetcond_{RESNET_K}", mapping_kwargs={"num_layers": num_layers})


def fill_mapping(G, seed):
    """Seeded mapping parameters for either implementation (same names by construction), in sorted-name order from one CPU generator:
    weights N(0,1) / lr_multiplier (StyleGAN2's init: `bias_gain` is the layer's lr_multiplier), biases 0.2 N(0,1) / lr_multiplier, and
    a non-zero w_avg so that truncation matters."""
    g = torch.Generator().manual_seed(int(seed))
    mp = G.backbone.mapping
    with torch.no_grad():
        for name, p in sorted(mp.named_parameters()):
            layer = getattr(mp, name.split(".")[0])
            v = torch.randn(p.shape, generator=g) / layer.bias_gain
            p.copy_(v if name.endswith("weight") else 0.2 * v)
        mp.w_avg.copy_(torch.randn(mp.w_avg.shape, generator=g) * 0.3)
    return G


def mapping_inputs(num_ws, seed):
    g = torch.Generator().manual_seed(int(seed))
    return {"zs": torch.randn(BATCH, num_ws, 512, generator=g), "c": torch.randn(BATCH, 25, generator=g),
            "feats": torch.randn(BATCH, 16, generator=g), "g_ws": torch.randn(BATCH, num_ws, 512, generator=g)}


def checksum(G, inp):
    return float(sum(p.detach().double().sum() for p in G.backbone.mapping.parameters()) + sum(v.double().sum() for v in inp.values()))


def sub(t):
    """What the fixture keeps of a gradient: all of a small tensor, every 8th row and column of a weight matrix."""
    return t[::8, ::8].contiguous() if t.dim() == 2 and t.numel() > 65536 else t


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def mapping_zplus_f64(params, w_avg, zs, c, feats, psi=1, cutoff=None, c_scale=1.0):
    """TriPlaneGenerator.mapping_zplus + MappingNetwork.forward (triplane.py:123-143, networks_stylegan2.py:250-291) restated in float64
    from the formulas: slot i of the output is slot i of the mapping of the i-th z.  params: name -> float64 tensor (raw parameters);
    the gains follow from the shapes (lr_multiplier 1 for embed, 0.01 for fc<i>)."""
    bs, n, _ = zs.shape
    norm2 = lambda x: x * (x.square().mean(dim=1, keepdim=True) + 1e-8).rsqrt()

    def fc(name, x, lr, act):
        w, b = params[name + ".weight"], params[name + ".bias"]
        y = x @ (w * (lr / math.sqrt(w.shape[1]))).t() + b * lr
        return F.leaky_relu(y, 0.2) * math.sqrt(2) if act else y
    z = zs.reshape(bs * n, -1)
    cc = torch.cat([(c * c_scale)[:, None].expand(-1, n, -1).reshape(bs * n, -1), feats[:, None, :RESNET_K].expand(-1, n, -1).reshape(bs * n, -1)], 1)
    x = torch.cat([norm2(z), norm2(fc("embed", cc, 1.0, False))], 1)
    i = 0
    while f"fc{i}.weight" in params:
        x = fc(f"fc{i}", x, 0.01, True)
        i += 1
    w = x.reshape(bs, n, -1)  # row (b, i) is the mapping of z_i: every slot of its broadcast ws holds it
    if psi != 1:
        t = w_avg + psi * (w - w_avg)
        if cutoff is None:
            w = t
        else:  # in the i-th broadcast ws the slots below the cutoff are truncated: slot i is, iff i < cutoff
            keep = (torch.arange(n) < cutoff)[None, :, None]
            w = torch.where(keep, t, w)
    return w, x


def mapping_against_fixture(P, device, L):
    """The body of the reference test, run on CPU (stand-in operators) and on the GPU: ws to the forward gate (1e-5 absolute), every
    parameter gradient and the gradients of z and resnet_feats to rel-L2 1e-4 against the reference's fp32 autograd and to 1e-5 against
    the float64 restatement, w_avg after two update_emas calls to 1e-6."""
    import p3d_testing as T
    from panic3d_amd.generator import TriPlaneGenerator
    g = T.load_golden("mapping_grad.npz")
    G = fill_mapping(TriPlaneGenerator(**mapping_kw(L)).eval(), 100 + L).to(device)
    mp = G.backbone.mapping
    inp = mapping_inputs(G.backbone.num_ws, 200 + L)
    p = f"L{L}_"
    assert abs(checksum(G, inp) - float(g[p + "checksum"])) < 1e-6 * abs(float(g[p + "checksum"])) + 1e-6, "re-drawn parameters / inputs differ"
    zs, feats = inp["zs"].clone().to(device).requires_grad_(True), inp["feats"].clone().to(device).requires_grad_(True)
    ws = G.mapping_zplus(zs, inp["c"].to(device), {"resnet_feats": feats}, truncation_psi=PSI, truncation_cutoff=CUTOFF)
    assert ws.grad_fn is not None
    assert float((ws.detach().cpu() - torch.from_numpy(g[p + "ws"])).abs().max()) < 1e-5
    (ws * inp["g_ws"].to(device)).sum().backward()
    # float64 restatement, full tensors
    p64 = {n: q.detach().cpu().double().requires_grad_(True) for n, q in mp.named_parameters()}
    z64, f64 = inp["zs"].double().requires_grad_(True), inp["feats"].double().requires_grad_(True)
    w64, _ = mapping_zplus_f64(p64, mp.w_avg.detach().cpu().double(), z64, inp["c"].double(), f64, PSI, CUTOFF)
    assert float((ws.detach().cpu().double() - w64.detach()).abs().max()) < 1e-5
    (w64 * inp["g_ws"].double()).sum().backward()
    bad = []
    for name, ours, ref32, ref64 in [("zs", zs.grad, g[p + "g_zs"], z64.grad), ("feats", feats.grad, g[p + "g_feats"], f64.grad)] + \
            [(n, q.grad, g[p + "g_" + n.replace(".", "__")], p64[n].grad) for n, q in mp.named_parameters()]:
        assert ours is not None and torch.isfinite(ours).all() and torch.count_nonzero(ours) > 0, name
        e32 = rel_l2(sub(ours.cpu()) if name not in ("zs", "feats") else ours, ref32)
        e64 = rel_l2(ours, ref64)
        print(f"L{L} {name}: vs reference fp32 {e32:.2e}, vs float64 {e64:.2e}")
        if not (e32 <= 1e-4 and e64 <= 1e-5):
            bad.append((name, e32, e64))
        if name not in ("zs", "feats"):
            n_ref = float(g[p + "n_" + name.replace(".", "__")])
            assert abs(float(ours.double().norm()) - n_ref) <= 1e-4 * n_ref, name
    assert not bad, bad
    # update_emas: two calls move w_avg twice, as the reference's do; the second call's ws and gradients
    G.zero_grad(set_to_none=True)
    for i in range(2):
        inp2 = mapping_inputs(G.backbone.num_ws, 300 + L + i)
        z2, f2 = inp2["zs"].clone().to(device).requires_grad_(True), inp2["feats"].clone().to(device).requires_grad_(True)
        ws2 = G.mapping_zplus(z2, inp2["c"].to(device), {"resnet_feats": f2}, update_emas=True)
    assert float((mp.w_avg.cpu() - torch.from_numpy(g[p + "emas_w_avg"])).abs().max()) <= 1e-6
    assert float((ws2.detach().cpu() - torch.from_numpy(g[p + "emas_ws"])).abs().max()) < 1e-5
    (ws2 * inp2["g_ws"].to(device)).sum().backward()
    assert rel_l2(z2.grad, g[p + "emas_g_zs"]) <= 1e-4 and rel_l2(sub(mp.fc0.weight.grad.cpu()), g[p + "emas_g_fc0_weight"]) <= 1e-4


def mapping_bits_and_memo(P, device):
    """The grad-mode ws is the no-grad ws bit for bit; a no-grad call after a grad call still uses the memoised detached weights; an
    optimiser step (a parameter version bump) is seen by the next call of either kind."""
    from panic3d_amd.generator import TriPlaneGenerator
    G = fill_mapping(TriPlaneGenerator(**mapping_kw(2)).eval(), 7).to(device)
    mp = G.backbone.mapping
    inp = {k: v.to(device) for k, v in mapping_inputs(G.backbone.num_ws, 8).items()}
    call = lambda: G.mapping_zplus(inp["zs"], inp["c"], {"resnet_feats": inp["feats"]}, truncation_psi=PSI, truncation_cutoff=CUTOFF)
    with torch.no_grad():
        cold = call().clone()
    memo = [mp.fc0._scaled_wb, mp.embed._scaled_wb]
    hot = call()
    assert hot.grad_fn is not None and torch.equal(hot.detach(), cold)
    with torch.no_grad():
        again = call()
    assert again.grad_fn is None and torch.equal(again, cold)
    assert mp.fc0._scaled_wb is memo[0] and mp.embed._scaled_wb is memo[1] and not memo[0][0].requires_grad
    (hot * inp["g_ws"]).sum().backward()
    opt = torch.optim.SGD(mp.parameters(), lr=10.0)
    opt.step()
    with torch.no_grad():
        stepped = call()
    assert not torch.equal(stepped, cold) and mp.fc0._scaled_wb is not memo[0]
    assert torch.equal(call().detach(), stepped)
    # one z expanded to every slot (what f() does): mapped once, and the gradient is the sum over the slots of the full z-plus call
    z = inp["zs"][:, 0].clone().requires_grad_(True)
    zs = z[:, None, :].expand(-1, G.backbone.num_ws, -1)
    assert zs.stride(1) == 0
    short = G.mapping_zplus(zs, inp["c"], {"resnet_feats": inp["feats"]}, truncation_psi=PSI, truncation_cutoff=CUTOFF)
    gs, = torch.autograd.grad((short * inp["g_ws"]).sum(), z)
    z2 = inp["zs"][:, 0].clone().requires_grad_(True)
    full = G.mapping_zplus(z2[:, None, :].expand(-1, G.backbone.num_ws, -1).contiguous(), inp["c"], {"resnet_feats": inp["feats"]},
                           truncation_psi=PSI, truncation_cutoff=CUTOFF)
    gf, = torch.autograd.grad((full * inp["g_ws"]).sum(), z2)
    assert float((short - full).detach().abs().max()) < 1e-5 and rel_l2(gs, gf) < 1e-5


# ---- torch stand-ins of the device operators (CPU tests) ---------------------------------------------------------------------------
def bias_act_backward_torch(y, g_y, act, alpha, gain, clamp, dscale=None, want_noise=False):
    """ops.bias_act_backward from the header's formula (include/p3d_synthesis_grad.h): the mask comes from the output."""
    assert dscale is None and not want_noise
    on = torch.ones_like(y) if clamp is None or clamp < 0 else (y.abs() < clamp).to(y.dtype)
    slope = torch.where(y <= 0, torch.full_like(y, alpha), torch.ones_like(y)) if int(act) == 1 else torch.ones_like(y)
    gz = g_y * gain * on * slope
    return gz, gz.reshape(y.shape[0], y.shape[1], -1).sum(-1), None


def install_mapping_ops(monkeypatch, ops):
    import p3d_torch_ops
    monkeypatch.setattr(ops, "bias_act", p3d_torch_ops.bias_act)
    monkeypatch.setattr(ops, "bias_act_backward", bias_act_backward_torch)


# ---- front-view paste ----------------------------------------------------------------------------------------------------------------
PASTE_PARAMS = {"mode": "default", "thresh_weight": 0.5, "thresh_edges": 0.2, "thresh_occ": 0.5, "offset_occ": 0.01, "thresh_dxyz": 0.05,
                "grad_sample": True}  # the thresholds of test_paste_front_vs_reference


def smooth_illustration(N, S, seed):
    """A gently curved illustration, per view and channel a + b u + c v + d u v + e u^2 + f v^2 over u, v in [0, 1] with |d|, |e|, |f| <=
    0.15 |b|, |c|: values in [0, 1], a gradient that differs per channel and direction and varies by ~30 % across the image.  Why
    not white noise here: bilinear sampling is C0, its derivative jumps at every texel boundary by the difference of neighbouring
    slopes.  Two binary32 evaluations of ix (torch's and the kernel's) differ by a fraction of an ulp of S, so a few pixels in 10^5
    land in different cells; with white noise each such pixel's term changes by O(1) and one of them alone moves the rel-L2 of g_xyz
    by ~1/sqrt(#masked pixels) ~ 7e-3 — the reference's own rounding, not the backward's arithmetic.  Here the jump is ~2 e / (S b)
    ~ 1e-3 of a term, below the 1e-5 gate after the same division.  White noise at fixed coordinates is what the kernel-level test uses."""
    g = torch.Generator().manual_seed(int(seed))
    k = torch.rand(N, 3, 6, generator=g)
    b, c = (0.25 + 0.25 * k[..., 1]) * torch.where(k[..., 0] > 0.5, 1.0, -1.0), (0.25 + 0.25 * k[..., 2]) * torch.where(k[..., 3] > 0.5, 1.0, -1.0)
    d, e, f = 0.15 * b * (2 * k[..., 3] - 1), 0.15 * b * (2 * k[..., 4] - 1), 0.15 * c * (2 * k[..., 5] - 1)
    u = ((torch.arange(S, dtype=torch.float32) + 0.5) / S)
    U, V = u[None, None, None, :], u[None, None, :, None]
    q = lambda t: t[..., None, None]
    img = q(b) * U + q(c) * V + q(d) * U * V + q(e) * U * U + q(f) * V * V
    lo, hi = img.amin(dim=(2, 3), keepdim=True), img.amax(dim=(2, 3), keepdim=True)
    return (img - lo) / (hi - lo) * 0.8 + 0.1


def paste_x(device):
    """An orthographic front view and a perspective view of two subjects, each with its own 512^2 illustration."""
    front = smooth_illustration(2, 512, 11)
    t = lambda v: torch.tensor(v).to(device)
    return dict(elevations=t([0.0, 5.0]), azimuths=t([0.0, 20.0]), fovs=t([-1.0, 30.0]), seeds=[3, 4], cond={"image_ortho_front": front.to(device)},
                triplane_crop=0.1, cull_clouds=0.5, neural_rendering_resolution=16)


def prepaste_from_sub4(sub4):
    """The pre-paste image of the train_step fixture: the 4x bilinear up-sampling (CPU, deterministic) of the stored subsample."""
    return F.interpolate(torch.as_tensor(sub4).cpu(), scale_factor=4, mode="bilinear", align_corners=False)


def paste_loss(image, weights, xyz):
    target = torch.rand(image.shape, generator=torch.Generator().manual_seed(12)).to(image.device)
    return (image - target).abs().mean() + weights.square().mean() + xyz[:, 2].square().mean()


def up_taps(S, r):
    """F.interpolate(bilinear, align_corners=False) r -> S as the kernels evaluate it in binary32 (csrc/p3d_paste_common.hpp up_index):
    (i0, i1 int64 [S], l float32 [S])."""
    i = torch.arange(S, dtype=torch.float32)
    scale = torch.tensor(r, dtype=torch.float32) / torch.tensor(S, dtype=torch.float32)
    src = ((i + 0.5) * scale - 0.5).clamp_min(0.0)
    i0 = src.to(torch.int64).clamp_max(r - 1)
    i1 = (i0 + 1).clamp_max(r - 1)
    return i0, i1, src - i0.to(torch.float32)


def _bilerp(m, ty, tx):
    """[..., r, r] -> [..., S, S] with given taps, in m's dtype, in the kernels' order of operations."""
    (y0, y1, ly), (x0, x1, lx) = ty, tx
    ly, lx = ly.to(m.dtype)[:, None], lx.to(m.dtype)[None, :]
    a00, a01 = m[..., y0[:, None], x0[None, :]], m[..., y0[:, None], x1[None, :]]
    a10, a11 = m[..., y1[:, None], x0[None, :]], m[..., y1[:, None], x1[None, :]]
    return (1 - ly) * ((1 - lx) * a00 + lx * a01) + ly * ((1 - lx) * a10 + lx * a11)


def paste_backward_ref(g_out, g_paste, mask, xyz, front, box_warp, normalize_images, grad_sample, coords="forward", fault=None):
    """Float64 gradients of torch.lerp(image, sample_orthofront(tocopy, interpolate(xyz, S)), mask) (+ the returned paste's cotangent)
    with respect to image, xyz and the illustration, for a GIVEN mask, written out term by term so that the absolute-value sums of the
    gate come with them: returns {name: (value, abs-value sum, K)}.

    coords="forward": the up-sampling taps and the sampling coordinates take the VALUES the binary32 forward computed (restated here
    operation for operation) and everything else — tap values, weights' products, every sum — is float64.  The gate bounds the
    rounding of the backward's own sums (8 sqrt(K) 2^-24 of the absolute-value sum); the forward's coordinates carry the forward's
    rounding, ~1 ulp of S in ix (6e-5 at S = 512), which moves a tap weight by that much and is not the backward's to answer for.
    coords="float64": coordinates in float64 too — this is what float64 torch autograd of the composition computes
    (test_paste_reference_is_torch_autograd checks that on CPU).
    fault: 'tap' drops the south-east tap's share, 'swap' exchanges the x / y channels, 'border' keeps the gradient where the forward
    clamped — the three faults the gate must catch."""
    dd = lambda t: None if t is None else torch.as_tensor(t).detach().cpu().double()
    g_out, g_paste, mask, front = dd(g_out), dd(g_paste), dd(mask), dd(front)
    xyz32 = torch.as_tensor(xyz).detach().cpu().float()
    N, _, r, _ = xyz32.shape
    S = mask.shape[-1]
    res = {}
    zero = torch.zeros(N, 3, S, S, dtype=torch.float64)
    go = g_out if g_out is not None else zero
    res["g_image"] = (go * (1 - mask), (go * (1 - mask)).abs(), 1)
    if not grad_sample:
        return res
    gp = go * mask + (g_paste if g_paste is not None else zero)
    abs_gp = (go * mask).abs() + (g_paste.abs() if g_paste is not None else zero)
    if coords == "forward":
        taps = up_taps(S, r)
        up = _bilerp(xyz32[:, :2], taps, taps)  # binary32, the kernel's order of operations
        bw = torch.tensor(box_warp, dtype=torch.float32)
        v = 1.0 - (up + bw * 0.5) / bw
        gxy = v * 2.0 - 1.0
        iu = ((gxy + 1.0) * float(S) - 1.0) * 0.5  # [:,0] from up-sampled x -> grid y (iy); [:,1] from up-sampled y -> grid x (ix)
        iu = iu.double()
        taps64 = tuple(t.double() if t.dtype.is_floating_point else t for t in taps)
    else:
        i = torch.arange(S, dtype=torch.float64)
        src = ((i + 0.5) * (r / S) - 0.5).clamp_min(0.0)
        i0 = src.to(torch.int64).clamp_max(r - 1)
        taps64 = (i0, (i0 + 1).clamp_max(r - 1), src - i0.double())
        up = _bilerp(xyz32[:, :2].double(), taps64, taps64)
        iu = (((1.0 - (up + box_warp / 2) / box_warp) * 2 - 1 + 1) * S - 1) / 2
    iy_u, ix_u = iu[:, 0], iu[:, 1]
    inside = lambda u: ((u > 0) & (u < S - 1)).double()
    ix, iy = ix_u.clamp(0, S - 1), iy_u.clamp(0, S - 1)
    x0, y0 = ix.floor(), iy.floor()
    tx, ty = (ix - x0)[:, None], (iy - y0)[:, None]
    x0, y0 = x0.long(), y0.long()
    x1, y1 = x0 + 1, y0 + 1
    tocopy = front * 2 - 1 if normalize_images else front
    if tocopy.shape[0] == 1 and N > 1:
        tocopy = tocopy.expand(N, -1, -1, -1)
    flat = tocopy.reshape(N, 3, S * S)

    def at(yy, xx):  # the transposed illustration at (row yy, column xx) = front[c][xx][yy]; out of range: 0
        ok = ((yy < S) & (xx < S)).double()[:, None]
        idx = (xx.clamp_max(S - 1) * S + yy.clamp_max(S - 1)).reshape(N, 1, S * S).expand(-1, 3, -1)
        return flat.gather(2, idx).reshape(N, 3, S, S) * ok
    nw, ne, sw, se = at(y0, x0), at(y0, x1), at(y1, x0), at(y1, x1)
    if fault == "tap":
        se = torch.zeros_like(se)
    terms_x = [(ne - nw) * (1 - ty), (se - sw) * ty]
    terms_y = [(sw - nw) * (1 - tx), (se - ne) * tx]
    dcoord = -S / box_warp
    bx, by = (inside(ix_u), inside(iy_u)) if fault != "border" else (torch.ones_like(ix_u), torch.ones_like(iy_u))
    g_upy = sum((gp * t).sum(1) for t in terms_x) * dcoord * bx  # up-sampled y (xyz channel 1) drives grid x
    g_upx = sum((gp * t).sum(1) for t in terms_y) * dcoord * by
    a_upy = sum((abs_gp * t.abs()).sum(1) for t in terms_x) * abs(dcoord) * bx
    a_upx = sum((abs_gp * t.abs()).sum(1) for t in terms_y) * abs(dcoord) * by
    if fault == "swap":
        g_upx, g_upy = g_upy, g_upx
    # the adjoint of the r -> S resize: every pixel hands (1-ly)(1-lx), (1-ly) lx, ly (1-lx), ly lx of its gradient to its four taps
    i0, i1, l = taps64
    Wm = torch.zeros(S, r, dtype=torch.float64)
    Wm[torch.arange(S), i0] += 1 - l
    Wm[torch.arange(S), i1] += l
    g_xyz = torch.zeros(N, 3, r, r, dtype=torch.float64)
    a_xyz = torch.zeros_like(g_xyz)
    for c, (gv, av) in enumerate(((g_upx, a_upx), (g_upy, a_upy))):
        g_xyz[:, c] = Wm.t() @ gv @ Wm
        a_xyz[:, c] = Wm.t() @ av @ Wm
    k_xyz = int((math.ceil(2 * S / r) + 1) ** 2 * 6)  # pixels whose taps touch a texel x (3 channels x 2 terms)
    res["g_xyz"] = (g_xyz, a_xyz, k_xyz)
    # the illustration: four-tap scatter of g_paste x weight (x 2 under normalize_images), summed over the views of a shared one
    shared = front.shape[0] == 1 and N > 1
    gf = torch.zeros(N, 3, S * S, dtype=torch.float64)
    af = torch.zeros_like(gf)
    k = 2.0 if normalize_images else 1.0
    cnt = torch.zeros(N, 1, S * S, dtype=torch.float64)
    for yy, xx, w in ((y0, x0, (1 - tx) * (1 - ty)), (y0, x1, tx * (1 - ty)), (y1, x0, (1 - tx) * ty), (y1, x1, tx * ty)):
        ok = ((yy < S) & (xx < S)).double()[:, None]
        idx = (xx.clamp_max(S - 1) * S + yy.clamp_max(S - 1)).reshape(N, 1, S * S)
        gf.scatter_add_(2, idx.expand(-1, 3, -1), (gp * w * ok * k).reshape(N, 3, S * S))
        af.scatter_add_(2, idx.expand(-1, 3, -1), (abs_gp * w * ok * k).reshape(N, 3, S * S))
        cnt.scatter_add_(2, idx, ok.reshape(N, 1, S * S).expand(-1, 1, -1).contiguous())
    gf, af = gf.reshape(N, 3, S, S), af.reshape(N, 3, S, S)
    if shared:
        gf, af, cnt = gf.sum(0, keepdim=True), af.sum(0, keepdim=True), cnt.sum(0, keepdim=True)
    res["g_front"] = (gf, af, max(int(cnt.max()), 1))
    return res


def paste_backward_torch(g_out, g_paste, mask, xyz, front, box_warp, normalize_images, grad_sample, want_image=True, want_xyz=False,
                         want_front=False, fault=None):
    """A binary32 stand-in of ops.paste_front_backward on CPU tensors (the float64 restatement at the forward's coordinates, rounded):
    what the CPU tests run the host wiring and the gate's fault detection on."""
    res = paste_backward_ref(g_out, g_paste, mask, xyz, front, box_warp, normalize_images, grad_sample, fault=fault)
    f = lambda k, want: res[k][0].float() if want and k in res else None
    return f("g_image", want_image), f("g_xyz", want_xyz), f("g_front", want_front)


def gate_ratio(ours, ref, absref, K):
    """max |ours - ref| / (sqrt(K) 2^-24 absref); where absref == 0 the value must be exact."""
    d = (torch.as_tensor(ours).double().cpu() - ref).abs()
    scale = math.sqrt(max(K, 1)) * EPS32 * absref
    r = torch.where(scale > 0, d / scale.clamp_min(1e-300), torch.where(d > 0, math.inf, 0.0))
    return float(r.max())


def check_paste_against_fixture(g, mask, g_prepaste, g_xyz):
    """Mask disagreement with the reference below 1 % (the cap of the forward test); g_prepaste on the agreeing pixels of the stored
    every-4th-pixel subsample and g_xyz on the texels whose up-sampling footprint holds no disagreeing pixel: rel-L2 <= 1e-5, the
    compared sets at least 95 % of the pixels / texels."""
    m_ref = torch.from_numpy(g["mask"])
    mask = mask.detach().cpu()
    differ = (mask - m_ref).abs() > 1e-3
    share = float(differ.float().mean())
    print(f"mask pixels that disagree with the reference: {share:.4%}")
    assert share < 0.01
    assert 0.01 < float(m_ref.mean()) < 0.99
    ok_px = ~differ[..., ::4, ::4].expand(-1, 3, -1, -1)
    ours, ref = g_prepaste.detach().cpu()[..., ::4, ::4], torch.from_numpy(g["g_prepaste_sub4"])
    assert float(ok_px.float().mean()) >= 0.95
    e_img = rel_l2(ours[ok_px], ref[ok_px])
    N, _, r, _ = g["g_xyz"].shape
    S = m_ref.shape[-1]
    i0, i1, _ = up_taps(S, r)
    W = torch.zeros(S, r)
    W[torch.arange(S), i0] = 1
    W[torch.arange(S), i1] = 1
    dirty = (W.t() @ differ[:, 0].float() @ W) > 0  # texels with a disagreeing pixel in their footprint
    ok_tx = ~dirty[:, None].expand(-1, 3, -1, -1)
    assert float(ok_tx.float().mean()) >= 0.95
    e_xyz = rel_l2(g_xyz.detach().cpu()[ok_tx], torch.from_numpy(g["g_xyz"])[ok_tx])
    print(f"g_prepaste rel-L2 {e_img:.2e} on {float(ok_px.float().mean()):.2%} of the pixels; g_xyz rel-L2 {e_xyz:.2e} on {float(ok_tx.float().mean()):.2%} of the texels")
    assert torch.count_nonzero(torch.from_numpy(g["g_xyz"])[:, :2]) > 0
    assert e_img <= 1e-5 and e_xyz <= 1e-5, (e_img, e_xyz)
