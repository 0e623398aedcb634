"""CPU (-m "not gpu"): the float64 references of the synthesis backward (tests/synthesis_grad_ref.py) and the gate that
tests/test_hip_synthesis_grad_edges.py applies with them.

1. The references are right: for the three product configurations (plain 3x3 / pad 1 with flipped weights, up-sampling stride 2 /
   pad 0 after the FIR adjoint, 1x1) on ragged shapes they agree with torch float64 autograd of F.conv2d / F.conv_transpose2d,
   and the bias_act rule agrees with autograd of the _bias_act_ref formulation away from its kinks.
2. The gate is tight enough to matter: a float32 evaluation of each operation at the largest K of the GPU matrix passes it, and
   each seeded corruption of that result (a 16-wide K chunk dropped, the last tile row or column zeroed, a tap shifted by one pixel,
   a slab counted twice, samples swapped in g_d, the lrelu slope flipped at y == 0) fails it."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import p3d_torch_ops as TO
import synthesis_grad_cases as SC
import synthesis_grad_ref as R

D = torch.float64


def _close(a, b, tol=1e-12):
    e = R.rel_l2(a.detach(), b.detach())
    assert e <= tol, e


@pytest.mark.parametrize("kind,N,I,O,H,W", [("plain", 3, 17, 13, 7, 11), ("plain", 1, 5, 3, 1, 9), ("up", 2, 5, 9, 5, 6),
                                            ("up", 1, 3, 4, 1, 3), ("1x1", 3, 19, 7, 9, 4)])
def test_references_match_float64_autograd(kind, N, I, O, H, W):
    gen = torch.Generator().manual_seed(N * 100 + I + O + H * W)
    k = 1 if kind == "1x1" else 3
    x = torch.randn(N, I, H, W, generator=gen, dtype=D).requires_grad_(True)
    w = torch.randn(O, I, k, k, generator=gen, dtype=D).requires_grad_(True)
    s = (torch.randn(N, I, generator=gen, dtype=D) * 0.5 + 1).requires_grad_(True)
    d = (torch.rand(N, O, generator=gen, dtype=D) + 0.5).requires_grad_(True)
    xs = x * s[:, :, None, None]
    if kind == "plain":
        t = F.conv2d(xs, w, padding=1)
    elif kind == "up":
        t = F.conv_transpose2d(xs, w.transpose(0, 1), stride=2)  # [N,O,2H+1,2W+1]
    else:
        t = F.conv2d(xs, w)
    y = t * d[:, :, None, None]
    if kind == "up":
        f = torch.tensor([1.0, 3.0, 3.0, 1.0], dtype=D)
        f = f.ger(f) / 64
        y = F.conv2d(F.pad(y, [1, 1, 1, 1]), R.fir_ref(f)[None, None].repeat(O, 1, 1, 1), groups=O)
    gy = torch.randn(y.shape, generator=gen, dtype=D)
    G, gxs = torch.autograd.grad(y, (t, xs), gy, retain_graph=True)  # G = the cotangent of the conv output (g_z·d, FIR adjoint applied)
    gx, gw, gs, gd = torch.autograd.grad(y, (x, w, s, d), gy)
    taps = k * k
    wk = w.detach().permute(2, 3, 0, 1).reshape(taps, O, I)
    if kind == "plain":
        dg, _ = R.conv_dgrad_ref(G, wk.flip(0), I, H, W, 1, 1)
        gmap, xmap = (1, 0, 0), (1, 1, 1)
    elif kind == "up":
        dg, _ = R.conv_dgrad_ref(G, wk, I, H, W, 2, 0)
        gmap, xmap = (2, 1, 0), (1, 0, 0)
    else:
        dg, _ = R.conv_dgrad_ref(G, wk, I, H, W, 1, 0)
        gmap, xmap = (1, 0, 0), (1, 0, 0)
    _close(dg, gxs)
    g_s, _, g_x = R.mod_backward_ref(x.detach(), s.detach(), dg)
    _close(g_s, gs)
    _close(g_x, gx)
    r = R.conv_wgrad_ref(G, gmap, x.detach(), s.detach(), xmap, taps, (H, W), wk=wk, dscale=d.detach())
    _close(r["dw"].reshape(k, k, O, I).permute(2, 3, 0, 1), gw)
    _close(r["g_d"], gd)
    assert (r["abs_dw"] >= r["dw"].abs() - 1e-12).all() and (r["abs_g_d"] >= r["g_d"].abs() - 1e-12).all()


@pytest.mark.parametrize("act,clamp,with_ds", [(1, None, False), (1, 1.25, True), (0, 1.25, False), (0, None, True)])
def test_bias_act_rule_matches_autograd_away_from_kinks(act, clamp, with_ds):
    gen = torch.Generator().manual_seed(act * 10 + (clamp is not None) * 2 + with_ds)
    alpha, gain = 0.25, 1.5  # exact in float32: the reference takes the float32 values the ABI receives
    N, C, HW = 3, 5, 37
    z = torch.randn(N, C, HW, generator=gen, dtype=D) * 1.5
    a = torch.where(z > 0, z, z * (alpha if act == 1 else 1.0)).abs() * gain
    near = (z.abs() < 0.05) | ((a - (clamp or -10)).abs() < 0.05)
    z = torch.where(near, torch.full_like(z, 0.3), z).requires_grad_(True)
    y = TO.bias_act(z, act="lrelu" if act == 1 else "linear", alpha=alpha, gain=gain, clamp=clamp)
    gy = torch.randn(y.shape, generator=gen, dtype=D)
    gz, = torch.autograd.grad(y, z, gy)
    ds = torch.rand(N, C, generator=gen, dtype=D) + 0.5 if with_ds else None
    r = R.bias_act_backward_ref(y.detach(), gy, act, alpha, gain, clamp, ds)
    _close(r["g_z"], gz, 1e-15)
    _close(r["g_out"], gz * (ds[:, :, None] if with_ds else 1), 1e-15)
    _close(r["g_bias"], gz.sum(2), 1e-14)
    _close(r["g_noise"], gz.sum(1), 1e-14)
    if clamp is not None:
        assert (y.detach().abs() >= clamp).any() and (r["g_z"][y.detach().abs() >= clamp] == 0).all()


# ---- the gate's sensitivity --------------------------------------------------------------------------------------------------------
def _fails(name, bad, ref, absref, K):
    ratio = R.gate_ratio(bad, ref, absref, K)
    print(f"{name}: gate ratio {ratio:.3g} (c = {R.GATE_C:g})")
    assert not R.gate_passes(bad, ref, absref, K), name


def _largest(cases, key):
    return max(cases, key=key)


def test_gate_catches_wrong_dgrad():
    N, Ci, Co, Hi, Wi, Ho, Wo, taps, stride, pad = _largest(SC.DGRAD_CASES, lambda c: c[7] * c[1])
    K = taps * Ci
    gen = torch.Generator().manual_seed(1)
    g = torch.randn(N, Ci, Hi, Wi, generator=gen)
    wk = torch.randn(taps, Ci, Co, generator=gen)
    ref, absref = R.conv_dgrad_ref(g, wk, Co, Ho, Wo, stride, pad)
    out, _ = R.conv_dgrad_ref(g, wk, Co, Ho, Wo, stride, pad, dtype=torch.float32)
    print("float32 evaluation: gate ratio %.3g" % R.gate_ratio(out, ref, absref, K))
    assert R.gate_passes(out, ref, absref, K)
    t0, j = taps // 2, (Ci - 1) // 16

    def part(gg, t, chunk=None):  # the contribution of tap t (and of one 16-wide channel chunk of it)
        m = torch.zeros_like(wk)
        lo, hi = (16 * chunk, 16 * chunk + 16) if chunk is not None else (0, Ci)
        m[t, lo:hi] = wk[t, lo:hi]
        return R.conv_dgrad_ref(gg, m, Co, Ho, Wo, stride, pad, dtype=torch.float32)[0]
    _fails("K chunk dropped", out - part(g, t0, j), ref, absref, K)
    bad = out.clone()
    bad[:, 64 * ((Co - 1) // 64):] = 0
    _fails("last tile row zeroed", bad, ref, absref, K)
    bad = out.clone().reshape(N, Co, -1)
    bad[:, :, 64 * ((Ho * Wo - 1) // 64):] = 0
    _fails("last tile column zeroed", bad.reshape(out.shape), ref, absref, K)
    g_sh = F.pad(g, [1, 0])[..., :-1]  # one pixel to the right
    _fails("tap shifted by one pixel", out - part(g, t0) + part(g_sh, t0), ref, absref, K)


def test_gate_catches_wrong_wgrad():
    (kind, N, O, I, Hd, Wd), _, _ = _largest([c for c in SC.WGRAD_CASES if c[2]], lambda c: c[0][1] * c[0][4] * c[0][5])
    taps, gmap, xmap, gsz, xsz = SC.WGRAD_MAPS[kind]
    K = N * Hd * Wd
    slabs, slabK = R.sg_split(N, O, I, taps, Hd, Wd)
    assert N >= 2 and slabs >= 2
    gen = torch.Generator().manual_seed(2)
    g = torch.randn(N, O, *gsz(Hd, Wd), generator=gen)
    x = torch.randn(N, I, *xsz(Hd, Wd), generator=gen)
    s = torch.randn(N, I, generator=gen) * 0.5 + 1
    wk = torch.randn(taps, O, I, generator=gen)
    ds = torch.rand(N, O, generator=gen) + 0.5
    ref = R.conv_wgrad_ref(g, gmap, x, s, xmap, taps, (Hd, Wd), wk=wk, dscale=ds)
    r32 = R.conv_wgrad_ref(g, gmap, x, s, xmap, taps, (Hd, Wd), wk=wk, dscale=ds, dtype=torch.float32)
    Kd = (np.sqrt(Hd * Wd) + np.sqrt(taps * I)) ** 2
    dw, gd = r32["dw"], r32["g_d"]
    print("float32 evaluation: gate ratios dw %.3g, g_d %.3g" % (R.gate_ratio(dw, ref["dw"], ref["abs_dw"], K),
                                                                 R.gate_ratio(gd, ref["g_d"], ref["abs_g_d"], Kd)))
    assert R.gate_passes(dw, ref["dw"], ref["abs_dw"], K) and R.gate_passes(gd, ref["g_d"], ref["abs_g_d"], Kd)
    G, X = R.wgrad_operands(g, gmap, x, s, xmap, taps, (Hd, Wd), dtype=torch.float32)

    def pixels(n, lo, hi):  # the contribution of sample n's pixels [lo, hi) to dw
        return torch.einsum("top,tip->toi", G[n, :, :, lo:hi], X[n, :, :, lo:hi])
    _fails("K chunk dropped", dw - pixels(0, 32, 48), ref["dw"], ref["abs_dw"], K)
    bad = dw.clone()
    bad[:, 64 * ((O - 1) // 64):] = 0
    _fails("last tile row zeroed", bad, ref["dw"], ref["abs_dw"], K)
    bad = dw.clone()
    bad[:, :, 64 * ((I - 1) // 64):] = 0
    _fails("last tile column zeroed", bad, ref["dw"], ref["abs_dw"], K)
    t0 = taps // 2
    x_sh = F.pad(x, [1, 0])[..., :-1]
    sh = R.conv_wgrad_ref(g, gmap, x_sh, s, xmap, taps, (Hd, Wd), dtype=torch.float32)["dw"]
    bad = dw.clone()
    bad[t0] = sh[t0]
    _fails("tap shifted by one pixel", bad, ref["dw"], ref["abs_dw"], K)
    _fails("slab counted twice", dw + pixels(0, slabK, min(2 * slabK, Hd * Wd)), ref["dw"], ref["abs_dw"], K)
    _fails("samples swapped in g_d", gd[[1, 0] + list(range(2, N))], ref["g_d"], ref["abs_g_d"], Kd)


def test_gate_catches_wrong_mod_backward():
    N, C, HW = _largest(SC.MOD_CASES, lambda c: c[2])
    gen = torch.Generator().manual_seed(3)
    x, g = torch.randn(N, C, HW, generator=gen), torch.randn(N, C, HW, generator=gen)
    s = torch.randn(N, C, generator=gen)
    gs, ags, _ = R.mod_backward_ref(x, s, g)
    gs32, _, _ = R.mod_backward_ref(x, s, g, dtype=torch.float32)
    assert R.gate_passes(gs32, gs, ags, HW)
    _fails("K chunk dropped", gs32 - (x[..., 16:32] * g[..., 16:32]).sum(2), gs, ags, HW)
    bad = gs32.clone()
    bad[:, 64 * ((C - 1) // 64):] = 0
    _fails("last tile row zeroed", bad, gs, ags, HW)


def test_gate_catches_wrong_bias_act_backward():
    N, C, HW, act, alpha, gain, clamp, *_ = _largest([c for c in SC.BIAS_ACT_CASES if c[3] == 1], lambda c: c[0] * c[1] * c[2])
    gen = torch.Generator().manual_seed(4)
    y = torch.randn(N, C, HW, generator=gen)
    y.view(-1)[::7] = 0.0
    gy = torch.randn(N, C, HW, generator=gen)
    ref = R.bias_act_backward_ref(y, gy, act, alpha, gain, clamp)
    r32 = R.bias_act_backward_ref(y, gy, act, alpha, gain, clamp, dtype=torch.float32)
    assert R.ulp_distance(r32["g_out"], ref["g_out"]) <= R.ULP_MAX
    assert R.gate_passes(r32["g_bias"], ref["g_bias"], ref["abs_bias"], HW)
    assert R.gate_passes(r32["g_noise"], ref["g_noise"], ref["abs_noise"], C)
    bad = torch.where(y == 0, r32["g_out"] / R.f32(alpha), r32["g_out"])  # the lrelu slope flipped where y == 0
    print("slope flipped at y == 0: %.3g ulp" % R.ulp_distance(bad, ref["g_out"]))
    assert R.ulp_distance(bad, ref["g_out"]) > R.ULP_MAX
    _fails("bias sum: K chunk dropped", r32["g_bias"] - r32["g_z"][..., 16:32].sum(2), ref["g_bias"], ref["abs_bias"], HW)
    _fails("noise sum: channel slice dropped", r32["g_noise"] - r32["g_z"][:, 16:32].sum(1), ref["g_noise"], ref["abs_noise"], C)
    bad = r32["g_bias"].clone()
    bad[:, -1] = 0
    _fails("bias sum: last row zeroed", bad, ref["g_bias"], ref["abs_bias"], HW)


def test_matrix_covers_the_edges():
    """The kernel-level GPU matrix holds the listed tails, maps and slab layouts (the sg_split mirror is used only here and above)."""
    dg = SC.DGRAD_CASES
    assert {(c[7], c[8], c[9]) for c in dg} >= {(t, s, p) for t in (1, 9) for s in (1, 2) for p in (0, 1, 2)}
    assert {1, 15, 16, 17, 33, 130} <= {c[1] for c in dg} and {1, 3, 63, 64, 65, 130} <= {c[2] for c in dg}
    assert any(c[5] != c[6] and (c[5] * c[6]) % 64 and (c[5] * c[6]) % 16 for c in dg) and {1, 3} <= {c[0] for c in dg}
    wg = [c for c, _, _ in SC.WGRAD_CASES]
    assert set(SC.WGRAD_MAPS) == {c[0] for c in wg}
    assert {1, 15, 17, 63, 64, 65, 130} <= {c[2] for c in wg} | {c[3] for c in wg}
    assert any(c[4] * c[5] < 16 for c in wg) and any((c[4] * c[5]) % 16 for c in wg)
    ragged = [c for c in wg if R.sg_split(c[1], c[2], c[3], SC.WGRAD_MAPS[c[0]][0], c[4], c[5])[0] >= 3
              and (c[4] * c[5]) % R.sg_split(c[1], c[2], c[3], SC.WGRAD_MAPS[c[0]][0], c[4], c[5])[1]]
    assert len(ragged) >= 3, ragged
    assert any(c[1] == 3 and gd for c, _, gd in SC.WGRAD_CASES) and any(not s for _, s, _ in SC.WGRAD_CASES)
    assert {1, 7, 255, 256, 257, 4099} <= {c[2] for c in SC.MOD_CASES}
    ba = SC.BIAS_ACT_CASES
    assert {0, 1} == {c[3] for c in ba} and any(c[8] for c in ba) and any(c[7] for c in ba) and any(not c[7] for c in ba)
    assert {1, 15, 17, 96} <= {c[1] for c in ba if c[9]} and any(c[2] < 256 and (c[0] * c[2]) % 16 for c in ba if c[9])
