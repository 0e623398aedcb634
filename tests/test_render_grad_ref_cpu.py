"""CPU (-m "not gpu"): the float64 references of the renderer / point-decode backward (tests/render_grad_ref.py), the designed matrix
(tests/render_grad_cases.py) and the gate tests/test_hip_render_grad_edges.py applies with them.

1. The references are right: they agree with the reference's own fp32 autograd (tests/golden/grad_*.npz, grad_run_model.npz) within
   REL_TOL, at the merged depths and mask decisions of the exact contract (the CPU oracle: the library forward's bits).
2. The gate is trustworthy: on every case a float32 evaluation of the same restatement agrees with the float64 one to a quarter of
   REL_TOL_FP64 per tensor, so the reference's own error and the cases' conditioning leave the kernel three quarters of the gate.
3. The gate is tight enough to matter: each seeded defect of the float32 restatement fails it on a named case.
4. The matrix is not vacuous: touched maps, mask fractions, tap classes, dead chunks and zero-weight rays are what the cases claim."""
import functools

import numpy as np
import pytest
import torch

import p3d_testing as T
import render_grad_cases as RC
import render_grad_ref as R
from test_hip_render_grad import GRAD_CASES, REL_TOL, REL_TOL_FP64

RENDER = {c[0]: c for c in RC.RENDER_CASES}
DECODE = {c[0]: c for c in RC.DECODE_CASES}


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle as o
    o.build()
    return o


@functools.lru_cache(maxsize=None)
def _render(name, orc):
    c = RC.build_render(RENDER[name])
    sigma = RC.oracle_sigma(orc, c, RC.render_sigma_points(c).numpy())
    return c, sigma, RC.render_ref(c, sigma)


@functools.lru_cache(maxsize=None)
def _decode(name, orc):
    c = RC.build_decode(DECODE[name])
    sigma = RC.oracle_sigma(orc, c, c["coords"].numpy())
    return c, sigma, RC.decode_ref(c, sigma)


def _fmt(errs):
    return {k: f"{v:.2e}" for k, v in errs.items()}


# ---- 2 + 4: conditioning and non-vacuity, case by case ---------------------------------------------------------------------------
def _frac_ok(x):
    return 0.10 <= x <= 0.90


@pytest.mark.parametrize("name", list(RENDER))
def test_render_case_is_well_conditioned_and_not_vacuous(orc, name):
    c, sigma, (gp, gm, touched) = _render(name, orc)
    g32 = RC.render_ref(c, sigma, dtype=torch.float32)
    errs, stray, finite = R.gate_errors(g32[0], g32[1], gp, gm, touched)
    print(f"render {name}: float32 vs float64 {_fmt(errs)}, touched {touched.mean():.2f}")
    assert finite and stray == 0 and all(torch.isfinite(x).all() for x in [gp] + gm)
    assert max(errs.values()) <= REL_TOL_FP64 / 4, errs
    masked = RC.masks_from_sigma(sigma).reshape(c["N"], c["R"], c["S"])
    if all(x is None for x in c["cot"]):
        assert not touched.any() and not gp.any()
    else:
        assert _frac_ok(touched.mean()), touched.mean()
        assert gp.abs().sum() > 0 and (c["o"]["binarize"] or gm[2][0].abs().sum() > 0)
    if name in RC.MASK_CASES:
        frac = float((sigma == -1000.0).mean())  # (binarize overwrites every density: the -1000 share of its two constants)
        assert _frac_ok(frac), frac
        if c["o"]["binarize"]:
            assert masked.all()
    else:
        assert not masked.any()
    if name in RC.MIX_CASES:
        cls = R.tap_classes(RC.render_sigma_points(c).numpy(), c["H"], c["W"], c["o"]["box_warp"], c["o"]["plane_mode"])
        fr = [float((cls == k).mean()) for k in range(3)]
        assert all(_frac_ok(f) for f in fr), fr
    if name == "crop_cull":
        assert 0 < int(masked.all(-1).sum()) < c["R"], "the scene must hold fully masked rays (wsum == 0) and others"
    if name == "repeat":
        t = c["depths"]
        assert ((t[..., 1:] == t[..., :-1]).all(-1)).sum() > 0 and ((t[..., 1:] == t[..., :-1]).any(-1)).all()
    if name == "zeros":  # a k_g_mlp step whose 64 lanes are all dead, next to live ones
        dead = np.repeat((c["cot"][0].abs().sum(-1) + sum(x.abs().sum(-1) for x in c["cot"][1:]) == 0).numpy().reshape(1, -1), c["S"], 0)
        chunks = dead.reshape(-1)[:dead.size // 64 * 64].reshape(-1, 64)
        assert chunks.all(1).any() and not chunks.all()
        assert (c["cot"][0][:, 1::3] == 0).all() and (c["cot"][0][:, :, 3::4] == 0).all()
    if name == "centres":  # every sample's weights on the (x, y) and (x, z) planes are one 1 and three 0
        q = RC.render_sigma_points(c).numpy().reshape(-1, 3).astype(np.float64)
        for a, b in ((0, 1), (0, 2)):
            w = R.plane_taps64(q[:, a], q[:, b], c["H"], c["W"])[2]
            assert ((w == 1).sum(0) == 1).all() and ((w == 0).sum(0) == 3).all()
    if c["o"]["per_view"]:  # ranges well apart: another view's range would cut every g_depth of this one
        t = c["depths"]
        assert all(float(t[v].max()) < float(t[v + 1].min()) - 1 for v in range(c["N"] - 1))


@pytest.mark.parametrize("name", list(DECODE))
def test_decode_case_is_well_conditioned_and_not_vacuous(orc, name):
    c, sigma, (gp, gm, touched) = _decode(name, orc)
    g32 = RC.decode_ref(c, sigma, dtype=torch.float32)
    errs, stray, finite = R.gate_errors(g32[0], g32[1], gp, gm, touched)
    print(f"decode {name}: float32 vs float64 {_fmt(errs)}, touched {touched.mean():.2f}")
    assert finite and stray == 0
    assert max(errs.values()) <= REL_TOL_FP64 / 4, errs
    masked = RC.masks_from_sigma(sigma)
    if c["g_sigma"] is None and c["g_rgb"] is None:
        assert not touched.any() and not gp.any()
    else:
        assert _frac_ok(touched.mean()), touched.mean()
    if c["o"]["crop"] or c["o"]["cull"] or c["o"]["binarize"]:
        frac = float((sigma == -1000.0).mean())
        assert _frac_ok(frac), frac
    else:
        assert not masked.any()
    if name == "mix_5x9":
        cls = R.tap_classes(c["coords"].numpy(), c["H"], c["W"], c["o"]["box_warp"], c["o"]["plane_mode"])
        fr = [float((cls == k).mean()) for k in range(3)]
        assert all(_frac_ok(f) for f in fr), fr
    if name == "centres":
        q = c["coords"].numpy().reshape(-1, 3).astype(np.float64)
        w = R.plane_taps64(q[:, 0], q[:, 1], c["H"], c["W"])[2]
        assert (((w == 1).sum(0) == 1) & ((w == 0).sum(0) == 3)).mean() > 0.5


def test_matrix_covers_the_edges():
    rc = RC.RENDER_CASES
    assert {1, 63, 64, 65, 257} <= {c[2] for c in rc if c[1] == 1}
    assert any(c[1] * c[2] * (c[3] + c[4]) > 64 * 1024 and c[1] * c[2] * (c[3] + c[4]) < 64 * 2048 for c in rc)
    assert any((c[3], c[4]) == (2, 0) for c in rc) and any((c[3] + c[4]) % 2 for c in rc) and any(c[4] == 0 and c[3] > 2 for c in rc)
    assert {(1, 3), (5, 9), (16, 8), (32, 32)} <= {(c[5], c[6]) for c in rc}
    assert {"all", "feat", "depth", "wsum", "xyz", "none", "zeros"} == {c[8] for c in rc}
    opt = lambda k, v: any(c[7].get(k) == v for c in rc)
    assert opt("plane_mode", 0) and opt("white_back", True) and opt("fsig", False) and opt("depths", "repeat") and opt("depths", "centres")
    assert any(c[7].get("crop") and c[7].get("cull") for c in rc) and all(any(c[7].get(k) and len([m for m in ("crop", "cull", "binarize") if c[7].get(m)]) == 1
                                                                              for c in rc) for k in ("crop", "cull", "binarize"))
    assert any(c[1] == 3 and c[2] == 37 and c[7].get("per_view") and c[7].get("shared") for c in rc)
    assert any(c[1] == 3 and c[2] == 37 and c[7].get("per_view") and not c[7].get("shared") for c in rc)
    dc = RC.DECODE_CASES
    assert {1, 63, 65} <= {c[2] for c in dc if c[1] == 1} and any(c[1] == 2 and c[2] == 100 for c in dc)
    assert any(c[1] == 3 and c[5].get("shared") for c in dc) and {"both", "sigma", "rgb", "none"} == {c[6] for c in dc}
    assert any(c[5].get("plane_mode") == 0 for c in dc) and any(c[5].get("fsig") is False for c in dc)


# ---- 1: the restatements against the reference's own autograd ---------------------------------------------------------------------
def test_tap_sampler_is_grid_sample():
    """The tap-by-tap sampler the mutations use is F.grid_sample (values and gradients), outside, border and interior alike."""
    c = RC.build_decode(DECODE["mix_5x9"])
    masked = np.zeros((c["N"], c["M"]), bool)
    a = RC.decode_ref(c, masked.astype(np.float32))
    b = RC.decode_ref(c, masked.astype(np.float32), mut={"sampler": "taps"})
    errs, stray, finite = R.gate_errors(b[0], b[1], a[0], a[1], a[2])
    assert finite and stray == 0 and max(errs.values()) <= 1e-12, errs


def test_decode_restatement_matches_the_reference(orc):
    g = T.load_golden("grad_run_model.npz")
    m = {k[5:]: g[k].item() for k in g if k.startswith("meta_")}
    N, M, seed = int(m["N"]), int(m["M"]), int(m["seed"])
    planes = T.make_planes(seed, N, int(m["H"]), int(m["W"]), smooth=int(m["smooth"]))
    assert T.checksum(planes) == str(g["planes_checksum"])
    mlp = [torch.from_numpy(x) for x in orc.prescale_mlp(*T.make_decoder_params(seed + 1, 1.0, 1.0), 1.0)]
    coords = torch.from_numpy(T.make_points(seed + 2, N, M))
    gen = torch.Generator().manual_seed(seed + 3)
    gs, gr = torch.randn(N, M, 1, generator=gen), torch.randn(N, M, 32, generator=gen)
    ro = dict(T.RENDERING_KWARGS, use_triplane=int(m["use_triplane"]))
    gp, gm, touched = R.decode_restate64(torch.from_numpy(planes), mlp, coords, gs, gr, np.zeros((N, M), bool), ro, bool(m["force_sigmoid"]))
    gains = (1 / np.sqrt(32), 1.0, 1 / np.sqrt(64), 1.0)  # the fixture differentiates the raw parameters
    errs = {"planes": R.rel_l2(gp, g["grad_planes"])}
    for k, x, gn in zip(("g_w0", "g_b0", "g_w1", "g_b1"), gm, gains):
        errs[k] = R.rel_l2(x * gn, g[k])
    print("run_model", _fmt(errs))
    assert max(errs.values()) <= REL_TOL, errs
    assert not np.any(g["grad_planes"][~np.broadcast_to(touched[:, :, None], g["grad_planes"].shape)]), "the touched map misses a texel"


@pytest.mark.parametrize("name", GRAD_CASES)
def test_render_restatement_matches_the_reference(orc, name):
    """The fixtures hold no merged depths: the exact contract's (the CPU oracle's) stand in, as on the GPU."""
    g = T.load_golden(name + ".npz")
    m = {k[5:]: g[k].item() for k in g if k.startswith("meta_")}
    N, Sc, Sf, seed = int(m["N"]), int(m["Sc"]), int(m["Sf"]), int(m["seed"])
    planes = T.make_planes(seed, N, int(m["H"]), int(m["W"]), scale=float(m["plane_scale"]), smooth=int(m["smooth"]))
    assert T.checksum(planes) == str(g["planes_checksum"])
    mlp = orc.prescale_mlp(*T.make_decoder_params(seed + 1, 1.0, float(m["sigma_gain"])), 1.0)
    R_ = g["rays_o"].shape[1]
    jit, u = T.make_random_draws(seed + 2, N, R_, Sc, Sf)
    ro = dict(T.RENDERING_KWARGS, depth_resolution=Sc, depth_resolution_importance=Sf, use_triplane=int(m["use_triplane"]),
              white_back=bool(m["white_back"]))
    opts = orc.make_opts(ro, float(m["crop"]) or None, float(m["cull"]) or None, float(m["binarize"]) or None, bool(m["force_sigmoid"]))
    *out, d = orc.render(planes, g["rays_o"], g["rays_d"], jit, u, mlp, opts, dumps=True)
    depths = d["depths_coarse"] if Sf == 0 else np.take_along_axis(np.concatenate([d["depths_coarse"], d["depths_fine"]], 1), d["perm"].astype(np.int64), 1)
    assert (np.diff(depths, axis=1) >= 0).all()
    o, dd, t = (torch.from_numpy(np.ascontiguousarray(x)) for x in (g["rays_o"], g["rays_d"], depths.reshape(N, R_, -1)))
    pts = R.points32(o, dd, t).reshape(N, -1, 3).numpy()
    sigma, _ = orc.decode(planes, pts, mlp, ro["box_warp"], ro["use_triplane"], opts.flags, opts.crop_limit, opts.cull_thresh, density_only=True)
    gen = torch.Generator().manual_seed(seed + 3)
    cot = [torch.randn(N, R_, k, generator=gen) for k in (32, 1, 1, 3)]
    gp, gm, touched = R.restate64(torch.from_numpy(planes), [torch.from_numpy(x) for x in mlp], o, dd, t, torch.from_numpy(sigma), None, ro,
                                  cot, False, bool(m["force_sigmoid"]), touched=True)
    gains = (1 / np.sqrt(32), 1.0, 1 / np.sqrt(64), 1.0)
    errs = {"planes": R.rel_l2(gp, g["grad_planes"])}
    for k, x, gn in zip(("g_w0", "g_b0", "g_w1", "g_b1"), gm, gains):
        if np.isfinite(g[k]).all():
            errs[k] = R.rel_l2(x * gn, g[k])
    print(name, _fmt(errs))
    assert torch.isfinite(gp).all() and max(errs.values()) <= REL_TOL, errs


# ---- 3: the gate's sensitivity ---------------------------------------------------------------------------------------------------
def _sample_mask(c, fn):
    """bool [N, R*S] over a render case's samples from fn(view, ray, sample index, the kernel's sample-major index)."""
    N, R_, S = c["N"], c["R"], c["S"]
    n, r, i = np.meshgrid(np.arange(N), np.arange(R_), np.arange(S), indexing="ij")
    return torch.from_numpy(fn(n, r, i, i * (N * R_) + n * R_ + r).reshape(N, R_ * S))


def _interior_tap(c, pts):
    """(bool [N,M] selecting one sample, plane 1, tap 0) with all four taps of that plane in range."""
    cls = R.tap_classes(pts, c["H"], c["W"], c["o"]["box_warp"], c["o"]["plane_mode"])[:, 1]
    sel = np.zeros(cls.shape, bool)
    sel[np.flatnonzero(cls == 2)[len(np.flatnonzero(cls == 2)) // 2]] = True
    return torch.from_numpy(sel.reshape(pts.shape[:2])), 1, 0


def _mutations():
    last_chunk = lambda c: _sample_mask(c, lambda n, r, i, g: g >= (c["N"] * c["R"] * c["S"]) // 64 * 64)
    one = lambda c: _sample_mask(c, lambda n, r, i, g: (r == 0) & (i == 5))
    pts = lambda c: RC.render_sigma_points(c).numpy()
    return [  # (defect, kind, case, mut from the case)
        ("one sample's contribution dropped", "render", "r1", lambda c: {"drop": one(c)}),
        ("the last partial chunk dropped", "render", "r63", lambda c: {"drop": last_chunk(c)}),
        ("the last partial chunk dropped (points)", "decode", "m65", lambda c: {"drop": torch.arange(65).view(1, 65) >= 64}),
        ("image 0 for every view", "render", "views_own", lambda c: {"image0": 1}),
        ("image 0 for every batch (points)", "decode", "n2_m100", lambda c: {"image0": 1}),
        ("plane 2's axes swapped", "render", "mix_5x9", lambda c: {"swap2": 1}),
        ("plane 2's axes swapped, plane_mode 0", "render", "r65", lambda c: {"swap2": 1}),
        ("a mask ignored", "render", "cull", lambda c: {"nomask": 1}),
        ("a mask ignored (crop)", "render", "crop", lambda c: {"nomask": 1}),
        ("a masked sample given its density gradient", "render", "binarize", lambda c: {"maskgrad": 1}),
        ("a masked point given its density gradient", "decode", "cull", lambda c: {"maskgrad": 1}),
        ("the white_back term dropped", "render", "r257", lambda c: {"nowhite": 1}),
        ("1.0 for 1.002", "render", "s_odd", lambda c: {"no1002": 1}),
        ("1.0 for 1.002 (points)", "decode", "clamped_rgb", lambda c: {"no1002": 1}),
        ("g_depth let through on a W == 0 ray", "render", "repeat", lambda c: {"depthW0": 1}),
        ("one tap written one texel to the right", "render", "r1", lambda c: {"tap": _interior_tap(c, pts(c))}),
        ("one tap written one texel to the right (points)", "decode", "m63", lambda c: {"tap": _interior_tap(c, c["coords"].numpy())}),
    ]


MUTATIONS = _mutations()


@pytest.mark.parametrize("k", range(len(MUTATIONS)), ids=[m[0] for m in MUTATIONS])
def test_gate_catches(orc, k):
    what, kind, name, make = MUTATIONS[k]
    c, sigma, (gp, gm, touched) = (_render if kind == "render" else _decode)(name, orc)
    ref = RC.render_ref if kind == "render" else RC.decode_ref
    mut = make(c)
    base = {"sampler": "taps"} if "tap" in mut else None
    ok = R.gate_errors(*ref(c, sigma, dtype=torch.float32, mut=base)[:2], gp, gm, touched)
    assert R.gate_passes(*ok, REL_TOL_FP64), "the float32 restatement itself must pass"
    errs, stray, finite = R.gate_errors(*ref(c, sigma, dtype=torch.float32, mut=mut)[:2], gp, gm, touched)
    print(f"{what}: caught by {kind} case '{name}': {_fmt(errs)}, non-zero untouched entries {stray}, finite {finite}")
    assert not R.gate_passes(errs, stray, finite, REL_TOL_FP64), what
