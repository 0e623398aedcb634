"""CPU (-m "not gpu"): the training loss without a device — the C ABI of its operators (include/p3d_loss.h, _lib.LOSS_SIGNATURES and the
library's exports; argument errors come back before any launch), the host wiring of panic3d_amd/loss.py on torch stand-ins of the
operators against the reference's own run (tests/golden/loss_phases.npz), the phase rules, and the float64 restatements and gates
that tests/test_hip_loss.py holds the kernels to: checked against torch's float64 autograd and against seeded faults.  On the parent
commit the module, the operators and the symbols do not exist."""
import os
import re

import pytest
import torch

import loss_cases as LC
import p3d_testing as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = torch.nn.functional


@pytest.fixture(scope="module")
def P():
    import panic3d_amd
    panic3d_amd.build()
    return panic3d_amd


@pytest.fixture(scope="module")
def golden():
    return T.load_golden("loss_phases.npz")


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_loss_header_table_and_exports_agree(P):
    hdr = open(os.path.join(ROOT, "include", "p3d_loss.h")).read()
    declared = set(re.findall(r"\b(p3d_[a-z0-9_]+)\s*\(", hdr))
    lib = P._lib
    assert declared == set(lib.LOSS_SIGNATURES)
    others = set(lib.SIGNATURES) | set(lib.GRAD_SIGNATURES) | set(lib.SYN_GRAD_SIGNATURES) | set(lib.PASTE_GRAD_SIGNATURES) | set(lib.DISC_SIGNATURES)
    assert not declared & others
    L = lib.lib()
    for name in declared:
        assert hasattr(L, name)
    assert "p3d_loss.hip" in P._build.SOURCES and os.path.join("..", "..", "include", "p3d_loss.h") in P._build.HEADERS
    assert "p3d_loss.hip" not in P._build.SYNTHESIS_UNIT and "p3d_loss.hip" not in P._build.RENDER_UNIT
    assert int(re.search(r"#define P3D_BLUR_MAX_TAPS (\d+)", hdr).group(1)) == lib.P3D_BLUR_MAX_TAPS == 127
    for name in ("Z", "X", "NORM"):
        assert int(re.search(rf"#define P3D_DEPTH_{name} (\d+)", hdr).group(1)) == getattr(lib, f"P3D_DEPTH_{name}")
    assert lib.P3D_ABI_VERSION == 9 and L.p3d_abi_version() == 9


def test_loss_argument_errors_without_gpu(P):
    L = P._lib.lib()
    p = 256  # never dereferenced: the checks come first
    blur = lambda taps=61, NC=3, H=8, W=8, x=p, f=p, y=p: L.p3d_blur_f32(x, NC, H, W, f, taps, y, None)
    assert blur(x=None) == -1 and blur(f=None) == -1 and blur(y=None) == -1 and blur(NC=0) == -1 and blur(H=0) == -1 and blur(W=-1) == -1
    assert blur(taps=60) == -2 and blur(taps=2) == -2 and blur(taps=129) == -2 and blur(taps=128) == -2 and blur(taps=0) == -2 and blur(taps=-1) == -2
    assert blur(H=1 << 16) == -2 and blur(NC=1 << 40) == -2

    l1 = lambda n=100, a=p, b=p, s=p, ws=p, wb=1 << 20: L.p3d_l1_f32(a, b, n, 1.0, s, None, ws, wb, None)
    assert l1(a=None) == -1 and l1(b=None) == -1 and l1(s=None) == -1 and l1(ws=None) == -1 and l1(n=0) == -1
    assert l1(n=1 << 41) == -2 and l1(wb=0) == -3
    assert L.p3d_l1_workspace_bytes(0) == 0 and L.p3d_l1_workspace_bytes(1) == 4 and L.p3d_l1_workspace_bytes(1 << 30) == 4096

    def vt(N=2, r=8, S=32, mode=0, wb=1 << 20, **ptr):
        a = dict(dict.fromkeys(("w", "xyz", "ga", "gx", "sums", "ws"), p), **ptr)
        return L.p3d_view_terms_f32(a["w"], a["xyz"], a["ga"], a["gx"], None, N, r, S, mode, 1.0, 1.0, a["sums"], None, None, a["ws"], wb, None)
    for k in ("w", "xyz", "ga", "gx", "sums", "ws"):
        assert vt(**{k: None}) == -1, k
    assert vt(N=0) == -1 and vt(r=0) == -1 and vt(S=0) == -1
    assert vt(r=33) == -2 and vt(r=9, S=8) == -2, "r > S"
    assert vt(mode=3) == -2 and vt(mode=-1) == -2, "a bad depth_mode"
    assert vt(S=1 << 15) == -2 and vt(wb=4) == -3
    assert L.p3d_view_terms_workspace_bytes(2, 8) == 2 * 2 * 4 and L.p3d_view_terms_workspace_bytes(3, 17) == 3 * 4 * 2 * 4
    assert L.p3d_view_terms_workspace_bytes(0, 8) == 0


# ---- the host wiring against the reference ----------------------------------------------------------------------------------------------
def _capture(P, monkeypatch):
    return lambda hook: monkeypatch.setattr(P.loss, "report", hook)


@pytest.mark.parametrize("name", sorted(LC.PHASE_CASES))
def test_phase_against_reference(P, monkeypatch, golden, name):
    LC.install_ops(monkeypatch, P.ops)
    reports, grads = LC.run_phase(P.StyleGAN2LossOrthoCondA, LC.PHASE_CASES[name], _capture(P, monkeypatch))
    LC.compare_with_fixture(golden, name, reports, grads)


def test_fixture_covers_every_phase_and_sigma(golden):
    names = {k.split("|")[0] for k in golden if "|" in k}
    assert names == set(LC.PHASE_CASES)
    assert {c["phase"] for c in LC.PHASE_CASES.values()} >= {"Gcond", "Gside-left", "Gside-right", "Gside-back", "Grand", "Gmain", "Greg", "Dmain",
                                                              "Gboth", "Dboth"}
    sig = lambda c: max(1 - c["cur_nimg"] / (c["kw"]["blur_fade_kimg"] * 1e3), 0) * c["kw"]["blur_init_sigma"]
    for fam in ("Gmain-s", "Gmain-masked-s", "Dmain-s"):
        s = sorted(sig(c) for n, c in LC.PHASE_CASES.items() if n.startswith(fam))
        assert s[0] == 0 and 1 < s[1] < 2 and s[2] == 10
    assert all(v > 0 for k, v in LC.LOSS_KW.items() if k.startswith("lambda_")) and len(LC.LAMBDAS) == 20
    for n in ("Gcond", "Grand", "Gside-left", "Gside-back", "Gmain-masked-s10"):  # the terms bite: no report is trivially zero
        for k, v in golden.items():
            if k.startswith(n + "|report|Loss/G/") and "signs" not in k:
                assert float(abs(v).max()) > 1e-4, k


def test_default_report_stores_detached_values(P, monkeypatch):
    LC.install_ops(monkeypatch, P.ops)
    monkeypatch.setattr(P.loss, "stats", {})
    G, D = LC.StandInG(LC.RK), LC.StandInD()
    case = LC.PHASE_CASES["Gcond"]
    loss = P.StyleGAN2LossOrthoCondA(device=torch.device("cpu"), G=G, D=D, augment_pipe=None, lpips_model=LC.lpips_stand_in, **case["kw"])
    loss.accumulate_gradients(phase="Gcond", gain=1.0, cur_nimg=0, **LC.loss_inputs())
    assert set(P.loss.stats) == {"Loss/G/cond/lpips", "Loss/G/cond/l1", "Loss/G/cond/alpha_l2", "Loss/G/cond/depth_l2", "Loss/G/cond"}
    assert all(not v.requires_grad and v.grad_fn is None for v in P.loss.stats.values())


def test_constructor_is_the_reference(P):
    import inspect
    sig = inspect.signature(P.StyleGAN2LossOrthoCondA.__init__)
    names = list(sig.parameters)[1:]
    assert names[:5] == ["device", "G", "D", "lpips_model", "augment_pipe"]
    defaults = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert defaults["r1_gamma"] == 10 and defaults["lambda_Gcond_lpips"] == 10.0 and defaults["lambda_Gcond_l1"] == 1.0
    assert defaults["neural_rendering_resolution_initial"] == 64 and defaults["gpc_reg_fade_kimg"] == 1000 and defaults["filter_mode"] == "antialiased"
    assert defaults["lossmask_mode_adv"] == "none" and defaults["paste_params_mode"] is None and len(names) == 45
    loss = P.StyleGAN2LossOrthoCondA(device=torch.device("cpu"), G=LC.StandInG(LC.RK), D=LC.StandInD(), lpips_model=LC.lpips_stand_in,
                                     paste_params_mode="Agrad")
    assert loss.paste_params["grad_sample"] is True and loss.paste_params["thresh_weight"] == 0.95 and loss.blur_raw_target
    assert all(hasattr(loss, n) for n in names) and loss.pl_mean.shape == () and loss.resample_filter.shape == (4, 4)
    assert P.loss.StyleGAN2LossOrthoCondA is P.StyleGAN2LossOrthoCondA


def _counting_loss(P, monkeypatch, rk, **kw):
    calls = []
    G, D = LC.StandInG(rk), LC.StandInD()
    for mod, meth in ((G, "f"), (G, "sample_mixed"), (D, "forward")):
        real = getattr(mod, meth)
        monkeypatch.setattr(mod, meth, lambda *a, _r=real, _m=meth, **k: (calls.append(_m), _r(*a, **k))[1])
    loss = P.StyleGAN2LossOrthoCondA(device=torch.device("cpu"), G=G, D=D, augment_pipe=None, lpips_model=LC.lpips_stand_in, **dict(LC.LOSS_KW, **kw))
    run = lambda phase: (calls.clear(), loss.accumulate_gradients(phase=phase, gain=1.0, cur_nimg=0, **LC.loss_inputs()), list(calls))[2]
    return run


def test_phase_remapping(P, monkeypatch):
    LC.install_ops(monkeypatch, P.ops)
    run = _counting_loss(P, monkeypatch, dict(LC.RK, density_reg=0.0), r1_gamma=0)
    assert run("Greg") == [] and run("Dreg") == [] and run("none") == []
    assert run("Gboth") == run("Gmain") == ["f", "forward"]
    assert run("Dboth") == run("Dmain") == ["f", "forward", "forward"]
    run = _counting_loss(P, monkeypatch, dict(LC.RK, density_reg=0.25, reg_type="l1"), r1_gamma=0)
    assert run("Greg") == ["sample_mixed"]
    assert run("Gboth") == ["f", "f", "f", "forward", "sample_mixed"]  # Gcond, Grand, Gmain, Greg
    run = _counting_loss(P, monkeypatch, dict(LC.RK, density_reg=0.25, reg_type="monotonic-fixed"), r1_gamma=0)
    assert run("Greg") == ["sample_mixed", "sample_mixed"]


def test_r1_raises_before_any_forward(P, monkeypatch):
    LC.install_ops(monkeypatch, P.ops)
    run = _counting_loss(P, monkeypatch, LC.RK, r1_gamma=10)
    for phase in ("Dreg", "Dboth"):
        with pytest.raises(RuntimeError, match="R1") as e:
            run(phase)
        assert str(e.value) == P.ops.R1_MESSAGE
    assert run("Dmain") == ["f", "forward", "forward"]
    assert "R1" in P.StyleGAN2LossOrthoCondA.__doc__


def test_lpips_weight_needs_a_model(P):
    mk = lambda **kw: P.StyleGAN2LossOrthoCondA(device=torch.device("cpu"), G=LC.StandInG(LC.RK), D=LC.StandInD(), lpips_model=None, **kw)
    with pytest.raises(ValueError, match="lpips_model"):
        mk()  # the default lambda_Gcond_lpips is 10
    with pytest.raises(ValueError, match="lambda_recon_lpips"):
        mk(lambda_Gcond_lpips=0, lambda_recon_lpips=0.5)
    assert mk(lambda_Gcond_lpips=0).lpips_model is None


def test_greg_style_mixing_uses_gen_z_and_gen_c(P, monkeypatch):
    """The reference names undefined variables there (loss_orthocondA.py:591): this package's runs."""
    LC.install_ops(monkeypatch, P.ops)
    run = _counting_loss(P, monkeypatch, dict(LC.RK, density_reg=0.25, reg_type="l1"), style_mixing_prob=1.0)
    assert run("Greg") == ["sample_mixed"]


def test_mask_view_orthofront_against_reference(P, golden):
    cond = LC.loss_inputs()["real_cond"]
    lmask = P.loss.mask_view_orthofront(cond["image_ortho_front_xyz"], cond["image_ortho_front_alpha"], cond["image_xyz"], cond["image_alpha"], LC.BOX_WARP)
    want = torch.from_numpy(golden["lmask"])
    assert torch.equal(lmask, want) and 0.05 < float(want.mean()) < 0.95 and not lmask.requires_grad


def test_morphology_is_min_and_max_over_the_in_bounds_window(P):
    g = torch.Generator().manual_seed(0)
    x = (torch.rand(2, 1, 9, 11, generator=g) > 0.4).float()
    for k in (1, 3, 5, 4):
        o = k // 2
        dil, ero = P.loss.dilation(x, k), P.loss.erosion(x, k)
        assert dil.shape == x.shape == ero.shape
        for y in range(9):
            for xx in range(11):
                win = x[:, :, max(y - o, 0):y - o + k, max(xx - o, 0):xx - o + k]
                assert torch.equal(dil[:, :, y, xx], win.amax(dim=(2, 3))) and torch.equal(ero[:, :, y, xx], win.amin(dim=(2, 3)))
    assert "kornia" in P.loss.dilation.__doc__ and "NOT pinned" in P.loss.dilation.__doc__


# ---- ops.blur under autograd ------------------------------------------------------------------------------------------------------------
def test_blur_wiring(P, monkeypatch):
    LC.install_ops(monkeypatch, P.ops)
    x = torch.randn(2, 3, 9, 12, generator=torch.Generator().manual_seed(1))
    assert P.ops.blur(x, 0) is x and P.ops.blur(x, 0.3) is x and P.ops.gaussian_filter(0.2) is None
    f = P.ops.gaussian_filter(10)
    ref = torch.arange(-30, 31).div(10).square().neg().exp2()
    assert f.numel() == 61 and torch.equal(f, ref / ref.sum())
    assert torch.equal(P.ops.blur(x, 1.5), LC.blur_torch(x, P.ops.gaussian_filter(1.5)))
    # the adjoint with an ASYMMETRIC filter, against autograd of the convolution; then once more through the backward (any order)
    fa = LC.blur_filter(5)
    xg = x.clone().requires_grad_(True)
    y = P.ops.blur_fir(xg, fa)
    assert y.grad_fn is not None and torch.equal(y.detach(), LC.blur_torch(x, fa))
    gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(2)).requires_grad_(True)
    gx, = torch.autograd.grad(y, xg, gy, create_graph=True)
    x2 = x.clone().requires_grad_(True)
    want, = torch.autograd.grad(LC.blur_torch(x2, fa), x2, gy.detach())
    assert LC.rel_l2(gx, want) < 1e-6
    ggy, = torch.autograd.grad(gx, gy, x)  # d/d gy of <A^T gy, x> = A x
    assert LC.rel_l2(ggy, LC.blur_torch(x, fa)) < 1e-6


def test_l1_and_view_terms_wiring(P, monkeypatch):
    LC.install_ops(monkeypatch, P.ops)
    g = torch.Generator().manual_seed(5)
    a, b = torch.randn(2, 3, 8, 8, generator=g), torch.randn(2, 3, 8, 8, generator=g)
    a[0, 0, 0, 0] = b[0, 0, 0, 0]
    ag = a.clone().requires_grad_(True)
    y = P.ops.l1_mean(ag, b)
    (y * 3).backward()
    assert torch.equal(y.detach(), P.ops.l1_mean(a, b)) and ag.grad[0, 0, 0, 0] == 0
    assert torch.allclose(ag.grad, 3 * torch.sign(a - b) / a.numel())
    c = LC.view_terms_case(32, 8, True)
    w, x = c["weights"].clone().requires_grad_(True), c["xyz"].clone().requires_grad_(True)
    for mode in ("z", "x", "norm"):
        t = P.ops.view_terms(w, x, c["gt_alpha"], c["gt_xyz"], mode, c["q"])
        assert t.shape == (2,) and torch.equal(t.detach(), P.ops.view_terms(c["weights"], c["xyz"], c["gt_alpha"], c["gt_xyz"], mode, c["q"]))
        gw, gx = torch.autograd.grad(2 * t[0] + 5 * t[1], [w, x])
        ref = LC.view_terms_f64(c["weights"], c["xyz"], c["gt_alpha"], c["gt_xyz"], mode, c["q"], 2 / 128, 5 / 128)
        assert LC.rel_l2(gw, ref["g_w"]) < 1e-5 and LC.rel_l2(gx, ref["g_x"]) < 1e-5, mode


# ---- the float64 restatements against torch's float64 autograd ---------------------------------------------------------------------------
@pytest.mark.parametrize("taps", LC.BLUR_TAPS)
def test_blur_f64_is_the_reference_filter(taps):
    f = LC.blur_filter(taps)
    for H, W in LC.blur_shapes((32, 64)):
        x, g = LC.blur_input(3, H, W)
        x64 = x.double().requires_grad_(True)
        y = LC.blur_torch(x64, f.double())
        assert LC.rel_l2(LC.blur_f64(x, f), y.detach()) < 1e-13
        gx, = torch.autograd.grad(y, x64, g.double())
        assert LC.rel_l2(LC.blur_adjoint_f64(g, f), gx) < 1e-13


@pytest.mark.parametrize("S,r", LC.VT_SHAPES)
@pytest.mark.parametrize("mode", ["z", "x", "norm"])
def test_view_terms_f64_is_the_reference_formula(S, r, mode):
    """Against float64 autograd of the reference's own sequence of torch calls; and the seeded inputs leave the comparison all but a
    few texels (the cap the device test holds itself to)."""
    for with_q in (False, True):
        c = LC.view_terms_case(S, r, with_q)
        d = {k: (v.double() if v is not None else None) for k, v in c.items()}
        count = c["weights"].numel()
        ref = LC.view_terms_f64(c["weights"], c["xyz"], c["gt_alpha"], c["gt_xyz"], mode, c["q"], 1 / count, 1 / count)
        assert float(ref["tight_z"].double().mean()) <= LC.VT_MAX_TIGHT and float(ref["tight_m"].double().mean()) <= LC.VT_MAX_TIGHT
        assert 0.1 < float(ref["m"].double().mean()) < 1 and bool(ref["mz"].any()) and not bool(ref["mz"].all()), "the masks must be mixed"
        terms, gw, gx = LC.view_terms_impl_torch(d["weights"], d["xyz"], d["gt_alpha"], d["gt_xyz"], mode, d["q"], True)
        keep_m, keep_z = ~ref["tight_m"], ~ref["tight_z"].expand_as(gx)
        if not ref["tight_z"].any():
            assert LC.rel_l2(ref["sums"] / count, terms) < 1e-6  # (torch's float64 resize takes its taps in float64: 1e-7 apart)
        # (the texel the case puts at almost zero distance turns the taps' 1e-7 into 1e-5 of its unit vector in mode norm)
        assert LC.rel_l2(ref["g_w"][keep_m], gw[keep_m]) < 1e-6 and LC.rel_l2(ref["g_x"][keep_z], gx[keep_z]) < 1e-4


def test_l1_f64(P):
    g = torch.Generator().manual_seed(9)
    a, b = torch.randn(1000, generator=g), torch.randn(1000, generator=g)
    a[3] = b[3]
    a64 = a.double().requires_grad_(True)
    s = (a64 - b.double()).abs().sum()
    s.backward()
    ref = LC.l1_f64(a, b, 1.0)
    assert float((ref["sum"] - s.detach()).abs()) < 1e-10 and torch.equal(ref["g_a"], a64.grad) and ref["g_a"][3] == 0


# ---- the gates notice seeded faults --------------------------------------------------------------------------------------------------------
def test_blur_gate_fails_seeded_faults():
    K = lambda taps: 2 * taps
    for taps, (H, W) in ((3, (33, 31)), (61, (33, 65)), (127, (5, 7))):
        f = LC.blur_filter(taps)
        x, g = LC.blur_input(2, H, W)
        ref, absref = LC.blur_f64(x, f), LC.blur_absref(x, f)
        assert LC.gate("blur", LC.blur_f64(x, f).float(), ref, absref, K(taps)) == []
        assert LC.gate("blur", LC.blur_torch(x, f), ref, absref, K(taps)) == []
        assert LC.gate("blur transposed", LC.blur_f64(x, f, fault="transposed").float(), ref, absref, K(taps)) != []
        gref, gabs = LC.blur_adjoint_f64(g, f), LC.blur_absref(g, f.flip(0))
        assert LC.gate("adjoint", LC.blur_adjoint_f64(g, f).float(), gref, gabs, K(taps)) == []
        assert LC.gate("adjoint unflipped", LC.blur_adjoint_f64(g, f, fault="unflipped").float(), gref, gabs, K(taps)) != []


def test_view_terms_gate_fails_seeded_faults():
    for (S, r), mode, fault, where in (((40, 19), "z", "halo", "g_w"), ((40, 19), "norm", "halo", "sums[0]"), ((32, 8), "z", "mz", "g_x"),
                                       ((33, 8), "norm", "mz", "sums[1]"), ((20, 6), "x", "mz", "g_x")):
        c = LC.view_terms_case(S, r, True)
        args = (c["weights"], c["xyz"], c["gt_alpha"], c["gt_xyz"], mode, c["q"], 0.01, 0.02)
        ref = LC.view_terms_f64(*args)
        assert LC.view_terms_gate(LC.view_terms_f32(*args), ref, mode) == []
        bad = LC.view_terms_gate(LC.view_terms_f32(*args, fault=fault), ref, mode)
        assert any(b.startswith(where) for b in bad), (S, r, mode, fault, bad)
