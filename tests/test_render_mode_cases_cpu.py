"""CPU: the case table of tests/render_mode_cases.py, before tests/test_hip_render_mode_edges.py trusts it on the GPU.

(1) Each case reaches what its row names: the plan (csrc/p3d_render_plan.hpp, through tests/render_plan_host.cpp) answers the
    instantiation, grid, block and tiling that render_mode_cases.expected_launch derives from the row alone.
(2) The table is complete: the instantiations the cases reach are all the plan can choose (a sweep of the plan's arguments), and
    those are the 44 that render_impl (csrc/p3d_kernels.hip) can launch.
(3) The scenes can fail: surfaces, empty rays, opacities on a mask threshold, rays that turn opaque before their last sample.
(4) The gate is sensitive: the final pass rebuilt from the oracle's dumps passes it; each seeded fault of the kind the tolerance
    mode or the tile mapping could have fails it.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import render_mode_cases as M
from host_build import CSRC, compile_host


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return compile_host(tmp_path_factory.mktemp("render_mode_cases"), "render_plan_host.cpp")


@pytest.fixture(scope="module")
def ops():
    import panic3d_amd
    return panic3d_amd.ops


def _plans(exe, requests):
    res = subprocess.run([exe], input="".join("p %d %d %d %d %d %d %d %d\n" % tuple(r) for r in requests), capture_output=True, text=True,
                         timeout=600)
    assert res.returncode == 0, res.stderr[-4000:]
    out = res.stdout.splitlines()
    assert len(out) == len(requests)
    keys = ("grid", "block", "lds", "tile_w", "tiles_x", "tiles_per_img", "ntiles", "lds_rows", "swz", "blocked")
    plans = []
    for line in out:
        f = line.split()
        plans.append(None if f[0] == "err" else dict(zip(keys, map(int, f[1:])), name=f[0]))
    return plans


@pytest.fixture(scope="module")
def case_plans(host, ops):
    reqs = [(c, fast) for c in M.CASES for fast in (False, True)]
    plans = _plans(host, [M.plan_request(ops, c, fast) for c, fast in reqs])
    return {(c["id"], fast): p for (c, fast), p in zip(reqs, plans)}


# ---- (1) -------------------------------------------------------------------------------------------------------------------------
def test_the_mask_band_and_the_termination_cut_are_the_header_s():
    with open(os.path.join(CSRC, "p3d_decode.hpp")) as f:
        src = f.read()
    m = re.search(r"#define\s+P3D_FAST_MASK_BAND\s+([0-9.eE+-]+)f", src)
    assert m and float(m.group(1)) == M.MASK_BAND
    m = re.search(r"#define\s+P3D_FAST_TD_CUT\s+([0-9.eE+-]+)\s", src)
    assert m and float(m.group(1)) == M.TD_CUT
    # the domain of the xyz bound follows from the cut: it takes at most half of the bound at the edge of the domain
    assert 2 * M.TD_CUT * (M.XYZ_DOMAIN + 1) <= 0.5 * M.FAST_MAX["xyz"]


def test_every_case_reaches_the_launch_its_row_names(case_plans):
    for (cid, fast), p in case_plans.items():
        c = M.CASE[cid]
        want = M.expected_launch(c, fast)
        assert p is not None, cid
        got = {k: p[k] for k in ("name", "tile_w", "tiles_x", "ntiles", "grid", "block")}
        assert got == {k: want[k] for k in got}, (cid, fast)
        assert (p["tile_w"] > 0) == (c["tile_w"] > 0), cid  # a tiled case really is launched on screen tiles


def test_the_shapes_reach_their_edges(case_plans):
    by_shape = {}
    for (cid, fast), p in case_plans.items():
        by_shape.setdefault(M.CASE[cid]["shape"], []).append((M.CASE[cid], fast, p))
    # list: a partial last tile at 8, 16 and 32 rays per wave, and the second view starts after it
    R = M.SHAPES["list"]["R"]
    assert all(R % rpw for rpw in (8, 16, 32))
    assert {M.expected_launch(c, f)["slots"] for c, f, _ in by_shape["list"]} == {1, 2, 4}
    assert all(p["tile_w"] == 0 and p["ntiles"] == 2 * -(-R // (32 // M.expected_launch(c, f)["slots"])) for c, f, p in by_shape["list"])
    # ... and small-launch workgroups of four waves whose last waves have no tile
    assert any(p["block"] == 256 and p["ntiles"] % 4 for c, f, p in by_shape["list"])
    # tiles: 3 resp. 6 tiles per row, on both kernels
    assert {(M.expected_launch(c, f)["slots"], p["tiles_x"]) for c, f, p in by_shape["tiles"] if p["tile_w"]} == {(1, 3), (2, 6), (4, 6)}
    # tail: swizzled blocks and an identity tail, a partial last tile
    for c, f, p in by_shape["tail"]:
        assert p["name"].startswith("k_render<") and p["swz"] > 0 and not p["blocked"]
        assert p["grid"] == 131 and p["grid"] > 8 * p["swz"] and p["grid"] % (8 * p["swz"]) != 0 and M.SHAPES["tail"]["R"] % 32 != 0
    assert {p["name"] for c, f, p in by_shape["tail"]} >= {"k_render<96,0,1,1,1>", "k_render<96,0,1,1,0>", "k_render<48,0,1,1,0>",
                                                          "k_render<64,0,1,1,0>", "k_render<64,0,1,0,0>"}
    # wide4: four-wave workgroups, a short last workgroup, an identity tail, a partial tile in every view
    for c, f, p in by_shape["wide4"]:
        assert (p["ntiles"], p["grid"], p["block"]) == (2055, 514, 256)
        assert p["ntiles"] % 4 != 0 and p["grid"] % 128 != 0 and p["grid"] % (8 * p["swz"]) == 2 and M.SHAPES["wide4"]["R"] % 32 != 0
    # blocked: the super-tile order over two views; blocked_tall: with tiles_x != tiles_y
    for shape, tiles_xy in (("blocked", (32, 32)), ("blocked_tall", (16, 64))):
        for c, f, p in by_shape[shape]:
            assert p["blocked"] == 1 and p["block"] == 256 and M.SHAPES[shape]["N"] == 2
            assert (p["tiles_x"], p["tiles_per_img"] // p["tiles_x"]) == tiles_xy and p["grid"] % (8 * p["swz"]) == 0


# ---- (2) -------------------------------------------------------------------------------------------------------------------------
def _launchable():
    """Every instantiation render_impl can name: k_render<NF, DUMP, FAST, EARLY, TCG> and k_render_slots<SLOTS, NF, FAST, WO>."""
    names = set()
    for nf in (48, 64, 96, 0):
        for F in (0, 1):
            names |= {f"k_render<{nf},1,{F},0,0>", f"k_render<{nf},0,{F},0,0>", f"k_render<{nf},0,{F},1,0>"}
            names |= {f"k_render_slots<{s},{nf},{F},0>" for s in (2, 4)}
    names |= {f"k_render<96,0,{F},1,1>" for F in (0, 1)}
    names |= {f"k_render_slots<4,{nf},1,1>" for nf in (48, 96)}
    return names


def test_the_table_reaches_every_instantiation_the_plan_can_choose(host, case_plans):
    from panic3d_amd import _lib as L
    bits = (L.P3D_FLAG_FAST_COLOR, L.P3D_FLAG_NO_PAIR, L.P3D_FLAG_PAIR16, L.P3D_FLAG_QUAD8, L.P3D_FLAG_WEIGHTS_ONLY,
            L.P3D_FLAG_NO_EARLY_OUT, L.P3D_FLAG_DISPARITY)
    reqs = []
    for N in (1, 2):
        for R, w in ((203, 0), (480, 24), (4187, 0), (16384, 128), (65536, 256), (262144, 512)):
            for Sc in (4, 48, 96, 100, 192):
                for Sf in (0, 7, 48, 64, 96, 136, 192):
                    for fm in range(128):
                        flags = sum(b for i, b in enumerate(bits) if fm >> i & 1)
                        reqs += [(N, R, w, Sc, Sf, flags, dl & 1, dl >> 1) for dl in range(4)]
    reachable = {p["name"] for p in _plans(host, reqs) if p is not None}
    launchable = _launchable()
    assert len(launchable) == 44 and reachable <= launchable
    # what the plan's rules cannot reach (nothing today) is derived by the sweep, not listed here
    print("launchable but never chosen by the plan:", sorted(launchable - reachable))
    reached = {p["name"] for p in case_plans.values()}
    assert reached == reachable, (sorted(reachable - reached), sorted(reached - reachable))
    assert len(reached) == 44 - len(launchable - reachable)


def test_every_option_set_meets_every_kernel_kind_and_the_single_extras_exist():
    kinds = {(M.expected_launch(c, True)["slots"], c["opt"]) for c in M.CASES if c["kind"] == "render"}
    assert kinds == {(s, o) for s in (1, 2, 4) for o in (0, 1, 2)}
    for shape in ("list", "tiles"):
        cs = [c for c in M.CASES if c["shape"] == shape]
        assert {(c["Sc"], c["Sf"]) for c in cs if c["kind"] == "render"} == set(M.RATES_SMALL)
        for rate in ((48, 48), (96, 96)):
            assert {(c["spacing"], c["small"], c["early"]) for c in cs if (c["Sc"], c["Sf"]) == rate and c["kind"] == "render"
                    and not c["per_view"] and not c["rng"]} == {(s, k, e) for s in ("fixed", "limits", "disparity")
                                                                for k in ("quad", "pair", False) for e in (True, False)}
        assert {(c["Sc"], c["spacing"], c["tile_w"] > 0) for c in cs if c["kind"] == "wo"} >= {(s, p, False) for s in (48, 96) for p in ("fixed", "limits")}
        assert any(c["kind"] == "dump" for c in cs)
    assert any(c["per_view"] and c["shape"] == "list" for c in M.CASES) and any(c["rng"] and c["shape"] == "tiles" for c in M.CASES)
    assert any(c["kind"] == "wo" and c["tile_w"] > 0 for c in M.CASES)


# ---- the final pass on the CPU, from the oracle's dumps ----------------------------------------------------------------------------
def _decode_sorted(oracle, case, mlp=None, no_threshold=False):
    """(sigma [NR,S], colours | xyz [NR,S,35], depths [NR,S]) of the merged samples, decoded at the dumped depths."""
    ref, inp = M.reference(case, dumps=True), M.inputs(case)
    t = ref["dumps"]["depths_sorted"]
    N, R = inp["o"].shape[:2]
    S = t.shape[1]
    pts = (inp["o"][:, :, None, :] + t.reshape(N, R, S, 1) * inp["d"][:, :, None, :]).astype(np.float32)  # mul, then add: renderer.py:179
    oo = oracle.make_opts(inp["ro"], **inp["kw"])
    flags = oo.flags & ~((oracle.FLAG_CULL | oracle.FLAG_BINARIZE) if no_threshold else 0)
    sigma, rgb = oracle.decode(inp["planes"], pts.reshape(N, R * S, 3), mlp or oracle.prescale_mlp(*inp["raw"]), M.BOX_WARP,
                               plane_mode=oo.plane_mode, flags=flags, crop_limit=oo.crop_limit, cull_thresh=oo.cull_thresh)
    return sigma.reshape(N * R, S), np.concatenate([rgb.reshape(N * R, S, 32), pts.reshape(N * R, S, 3)], -1), t


def _march(oracle, colors, sigma, t, white_back, td_cut=0.0, background=True):
    """ray_marcher.py:25-57 as oracle/p3d_oracle.c states it, with numpy sums; td_cut > 0: samples behind the point where the
    transmittance fell below it weigh nothing (the tolerance mode's termination).  Returns the four outputs and the transmittances."""
    f32 = np.float32
    dl, sm, tm = t[:, 1:] - t[:, :-1], (sigma[:, 1:] + sigma[:, :-1]) * f32(0.5), (t[:, 1:] + t[:, :-1]) * f32(0.5)
    rho = oracle.math_fn("softplus", sm - f32(1))
    alpha = f32(1) - oracle.math_fn("exp", -(rho * dl))
    step = ((f32(1) - alpha) + f32(1e-10)).astype(np.float64)
    Td = np.concatenate([np.ones((t.shape[0], 1)), np.cumprod(step, 1)[:, :-1]], 1)
    w = alpha * Td.astype(f32)
    w = np.where(Td < td_cut, f32(0), w)
    cm = (colors[:, 1:] + colors[:, :-1]) * f32(0.5)
    C, W, D = np.zeros((t.shape[0], colors.shape[2]), f32), np.zeros(t.shape[0], f32), np.zeros(t.shape[0], f32)
    f64 = np.float64
    for i in range(t.shape[1] - 1):  # in the oracle's order: C = fmaf(w, cm, C) (a product of two binary32 is exact in binary64)
        C = (w[:, i, None].astype(f64) * cm[:, i] + C).astype(f32)
        W = W + w[:, i]
        D = (w[:, i].astype(f64) * tm[:, i] + D).astype(f32)
    with np.errstate(invalid="ignore", divide="ignore"):
        depth = D / W
    depth = np.clip(np.where(np.isnan(depth), np.inf, depth), t.min(), t.max()).astype(f32)
    if white_back and background:
        C = (C + f32(1)) - W[:, None]
    C = C * f32(2) - f32(1)
    return dict(feat=C[:, :32], depth=depth[:, None], wsum=W[:, None], xyz=C[:, 32:]), Td


def _rebuilt(oracle, case, **kw):
    sigma, colors, t = _decode_sorted(oracle, case, mlp=kw.pop("mlp", None))
    sigma = kw.pop("sigma", sigma)
    return _march(oracle, colors, sigma, t, M.inputs(case)["ro"]["white_back"], **kw)[0]


def _opacity(oracle, case):
    """opacity of every merged sample before the threshold masks (renderer.py:150-153), NaN where the crop mask fired"""
    raw = _decode_sorted(oracle, case, no_threshold=True)[0]
    a = oracle.sigma2density(raw.reshape(-1)).reshape(raw.shape)
    return np.where(raw == -1000.0, np.nan, a), raw


# ---- (3) -------------------------------------------------------------------------------------------------------------------------
SCENE_RATE = {"list": (96, 96), "tiles": (96, 96), "tail": (96, 96), "wide4": (4, 4), "blocked": (4, 4), "blocked_tall": (4, 4)}


@pytest.mark.parametrize("shape", list(M.SHAPES))
def test_the_scenes_can_fail(oracle, shape):
    Sc, Sf = SCENE_RATE[shape]
    used = sorted({c["opt"] for c in M.CASES if c["shape"] == shape and (c["Sc"], c["Sf"]) == (Sc, Sf)})
    assert 0 in used
    for opt in used:
        case = M._case(shape, Sc, Sf, False, opt=opt)
        ref, inp = M.reference(case, dumps=True), M.inputs(case)
        w = ref["wsum"]
        sigma, colors, t = _decode_sorted(oracle, case)
        assert np.array_equal(sigma, ref["dumps"]["sigma_sorted"])  # the rebuild decodes what the oracle's final pass decoded
        Td = _march(oracle, colors, sigma, t, inp["ro"]["white_back"])[1]
        opaque = int((Td[:, :-1] < M.TD_CUT).any(1).sum())
        print(f"{shape} {Sc}+{Sf} o{opt}: mean wsum {w.mean():.3f}, {int((w == 0).sum())} empty rays of {w.size}, {opaque} opaque before the last sample")
        assert float(w.mean()) > 0.05 and opaque > 0
        # empty rays: the ones whose every sample is masked.  Outside the planes the decoder sees zero features and answers a
        # density of its own (sigma 42 to 55 in `wide4`), so a reversed ray is empty only where the crop mask (x and z, not y) or
        # the cull mask removes it; without masks (option set 2) no ray of a scene need be empty, and the check is made with them
        if opt != 2:
            assert int((w == 0).sum()) > 0
        if opt in (0, 1):  # cull / binarize: samples on the threshold, where the tolerance mode must re-decode
            a, _ = _opacity(oracle, case)
            near = np.abs(a - M.OPTION_SETS[opt]["kw"].get("cull_clouds", M.OPTION_SETS[opt]["kw"].get("binarize_clouds"))) < M.MASK_BAND
            print(f"   {int(near.sum())} samples within {M.MASK_BAND} of the threshold, on {int(near.any(1).sum())} rays")
            assert int(near.sum()) > 0


def _positions(o, d, t0, t1, Sc):
    """the largest |coordinate| of a sample position on rays o + t d (linear in t: at an end); the stratified depths reach from t0
    to t1 + (t1 - t0) / (Sc - 1), the last one jittered forward by up to one spacing"""
    t0, t1 = np.asarray(t0, np.float32)[..., None], np.asarray(t1, np.float32)[..., None]
    return float(max(np.abs(o + t0 * d).max(), np.abs(o + (t1 + (t1 - t0) / (Sc - 1)) * d).max()))


def test_every_rendered_scene_lies_inside_the_domain_of_the_xyz_bound():
    """Everything the gate renders — the scenes with their reversed rays, under fixed limits, per-ray limits and disparity
    spacing (the same range), and the sweep's configurations — keeps its sample positions within XYZ_DOMAIN per coordinate."""
    for shape in M.SHAPES:
        sc = M.scene(shape)
        N, R = sc["o"].shape[:2]
        rs, re = M._ray_limits(shape)
        Sc = min(c["Sc"] for c in M.CASES if c["shape"] == shape)
        far = max(_positions(sc["o"], sc["d"], np.full((N, R), T_START), np.full((N, R), T_END), Sc), _positions(sc["o"], sc["d"], rs, re, Sc))
        print(f"{shape}: sample positions within {far:.2f}")
        assert 1.0 < far <= M.XYZ_DOMAIN  # (and beyond the unit cube: the reversed rays are there)
    for seed in range(100, 124):
        c = M._random_config(seed)
        shp = c["o"].shape[:2]
        assert _positions(c["o"], c["d"], np.full(shp, c["ro"]["ray_start"]), np.full(shp, c["ro"]["ray_end"]),
                          c["ro"]["depth_resolution"]) <= M.XYZ_DOMAIN, seed


T_START, T_END = M.T.RENDERING_KWARGS["ray_start"], M.T.RENDERING_KWARGS["ray_end"]


@pytest.mark.parametrize("shape,Sc,Sf,opt", [("wide4", 4, 4, 0), ("list", 96, 96, 2), ("list", 96, 96, 1)])
def test_the_termination_alone_stays_inside_its_derived_share(oracle, shape, Sc, Sf, opt):
    """The final pass rebuilt from the oracle's dumps with nothing but the cut at TD_CUT, at the scenes whose weighted positions lie
    farthest out: what it leaves out is at most TD_CUT of wsum, 2 TD_CUT of a colour and 2 TD_CUT (|p| + 1) of xyz (+ the rebuild's own
    1e-6), half of the bound at most."""
    case = M._case(shape, Sc, Sf, False, opt=opt)
    ref = M.reference(case, dumps=True)
    _, colors, _ = _decode_sorted(oracle, case)
    pmax = float(np.abs(colors[..., 32:]).max())
    err = M.errors(_rebuilt(oracle, case, td_cut=M.TD_CUT), ref)
    print(f"{case['id']}: |p| <= {pmax:.2f}, the cut alone: " + "  ".join(f"{k} {v:.2e}" for k, v in err.items()))
    assert pmax <= M.XYZ_DOMAIN
    assert err["wsum"] <= M.TD_CUT + 1e-6 and err["feat"] <= 2 * M.TD_CUT + 1e-6 and err["xyz"] <= 2 * M.TD_CUT * (pmax + 1) + 1e-6
    assert err["xyz"] <= 0.5 * M.FAST_MAX["xyz"] + 1e-6


# ---- (4) -------------------------------------------------------------------------------------------------------------------------
FAULT_SCENES = [("list", 48, 48, 0), ("tiles", 96, 96, 0), ("list", 96, 96, 1)]


@pytest.mark.parametrize("shape,Sc,Sf,opt", FAULT_SCENES)
def test_the_gate_passes_the_rebuild_and_fails_every_seeded_fault(oracle, shape, Sc, Sf, opt):
    case = M._case(shape, Sc, Sf, False, opt=opt)
    ref, inp = M.reference(case, dumps=True), M.inputs(case)
    N, R = inp["o"].shape[:2]
    # the final pass from the dumps with oracle.decode + oracle.composite, then with the marcher above: both are the oracle's final pass
    sigma, colors, t = _decode_sorted(oracle, case)
    rgb, depth, w = oracle.composite(colors, sigma, t, white_back=inp["ro"]["white_back"])
    good = _rebuilt(oracle, case)
    for k, a in (("feat", rgb[:, :32]), ("depth", depth), ("wsum", w.sum(1)), ("feat", good["feat"]), ("depth", good["depth"]), ("wsum", good["wsum"])):
        assert float(np.abs(a.reshape(ref[k].shape) - ref[k]).max()) <= 1e-6, k
    assert M.gate(good, ref, exact=False) == []
    assert M.gate(ref, ref, exact=True) == [] and M.gate(ref, ref, exact=False) == []
    # one ulp of noise on the oracle's own outputs: inside the tolerance gate, outside the exact one
    rng = np.random.default_rng(1)
    noisy = {k: np.nextafter(ref[k], np.where(rng.integers(0, 2, ref[k].shape) > 0, np.inf, -np.inf).astype(np.float32)) for k in M.OUTPUTS}
    assert M.gate(noisy, ref, exact=False) == [] and len(M.gate(noisy, ref, exact=True)) == 4

    faults = {}
    # termination at Td < 1e-3 instead of the cut
    faults["termination at 1e-3"] = _rebuilt(oracle, case, td_cut=1e-3)
    assert M.gate(_rebuilt(oracle, case, td_cut=M.TD_CUT), ref, exact=False) == []  # ... while the stated cut is inside the bound
    # decoder weights rounded to f16: the low term of the two-term operands dropped
    w0, b0, w1, b1 = oracle.prescale_mlp(*inp["raw"])
    h = lambda w: w.astype(np.float16).astype(np.float32)  # noqa: E731
    faults["f16 weights"] = _rebuilt(oracle, case, mlp=(h(w0), b0, h(w1), b1))
    # the mask decision of the sample nearest the threshold flipped on every 10th ray
    o = M.OPTION_SETS[opt]["kw"]
    thr = o.get("cull_clouds", o.get("binarize_clouds"))
    a, raw = _opacity(oracle, case)
    sigma = np.array(ref["dumps"]["sigma_sorted"])
    flipped = 0
    for r in range(0, N * R, 10):
        if np.isnan(a[r]).all():
            continue
        i = int(np.nanargmin(np.abs(a[r] - thr)))
        sigma[r, i] = (raw[r, i] if "cull_clouds" in o else 1000.0) if sigma[r, i] == -1000.0 else -1000.0
        flipped += 1
    assert flipped > 10
    faults["flipped masks"] = _rebuilt(oracle, case, sigma=sigma)
    # the background term dropped
    assert inp["ro"]["white_back"]
    faults["no background"] = _rebuilt(oracle, case, background=False)
    # the rays of the last partial tile left at zero (per view, 32 rays per tile)
    if R % 32:
        z = {k: np.array(ref[k]) for k in M.OUTPUTS}
        for k in z:
            z[k][:, R // 32 * 32:] = 0
        faults["partial tile unwritten"] = z
    # the rays of one tile replaced by another tile's: the tile-mapping fault
    s = {k: np.array(ref[k]) for k in M.OUTPUTS}
    for k in s:
        s[k][0, 32:64] = s[k][0, 64:96]
    faults["tile rendered twice"] = s
    assert M.gate(s, ref, exact=True) != []
    for name, out in faults.items():
        bad = M.gate(out, ref, exact=False)
        print(f"{case['id']}: {name}: {bad}")
        assert bad, name


def test_the_gate_sees_a_non_finite_pattern_and_a_missing_output():
    ref = {k: np.zeros((1, 4, n), np.float32) for k, n in zip(M.OUTPUTS, (32, 1, 1, 3))}
    ref["depth"][0, 1] = np.inf
    got = {k: v.copy() for k, v in ref.items()}
    assert M.gate(got, ref, exact=False) == [] and M.gate(got, ref, exact=True) == []
    got["depth"][0, 1] = 3.0
    assert len(M.gate(got, ref, exact=False)) == 1
    got["depth"][0, 1] = -np.inf
    assert len(M.gate(got, ref, exact=False)) == 1
    got["depth"][0, 1] = np.inf
    got["feat"][0, 2, 5] = np.nan
    assert len(M.gate(got, ref, exact=False)) == 1 and len(M.gate(got, ref, exact=True)) == 1
    got["feat"], got["xyz"] = None, None  # a weights-only launch
    assert M.gate(got, ref, exact=False) == []
