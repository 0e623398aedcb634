"""The renderer's tolerance mode and tile mapping on every plan: the case table, the scenes, the references and the gate of
tests/test_render_mode_cases_cpu.py (CPU) and tests/test_hip_render_mode_edges.py (GPU).  Not collected.

A CASE is one launch shape with one kernel choice; both tests run it in the exact mode and in the tolerance mode
(P3D_FLAG_FAST_COLOR).  Its fields:
  shape    a row of SHAPES: the views, the ray count, the screen tiling and the plane size
  Sc, Sf   coarse / fine samples: a row of NF (which also names the fine-depth capacity of the instantiation)
  small    "quad" / "pair" / False / True (the library's size heuristic): ops.make_opts(small_launch_kernel=...)
  early    the exact early-outs on (production) or off (P3D_FLAG_NO_EARLY_OUT)
  spacing  "fixed" / "limits" (per-ray limits, ray_start = ray_end = 'auto') / "disparity"
  opt      a row of OPTION_SETS: masks, background, colour activation, plane convention
  kind     "render" / "dump" (a dump launch) / "wo" (a weights-only launch)
  tile_w   ray_tile_w of the launch (the shape's, or 0 for an untiled launch of an image)
  per_view P3D_FLAG_PER_VIEW_CLAMP;  rng: the draws are made inside the kernel (rng_seed)

The REFERENCE of a case is the oracle's render of the same inputs (reference()): one per (shape, rate, spacing, options, ...),
whatever kernel renders it.  The GATE (gate()) is the exact contract bit for bit, or the tolerance mode's stated bound on every ray.
"""
import functools

import numpy as np
import torch

import p3d_testing as T
from test_hip_parity import FAST_MAX, _random_config  # noqa: F401  (the ONE definition of the bound; the sweep's generator)

OUTPUTS = ("feat", "depth", "wsum", "xyz")
BOX_WARP = T.RENDERING_KWARGS["box_warp"]
# csrc/p3d_decode.hpp, read back from the header by the CPU test:
MASK_BAND = 2e-3   # P3D_FAST_MASK_BAND
TD_CUT = 5e-7      # P3D_FAST_TD_CUT: the tolerance mode drops a ray once its transmittance is below this, which leaves up to
                   # 2 * TD_CUT * (|position| + 1) out of xyz (white background) ...
XYZ_DOMAIN = 4.0   # ... so the xyz bound is stated for sample positions within this per coordinate: the cut takes at most half of it

# ---- shapes: the smallest that still reach each edge ---------------------------------------------------------------------------
# img = (width, height) of a screen image cut from a camera's rays; otherwise a ragged list of rays aimed at the box
SHAPES = {
    # a partial last tile at 8, 16 and 32 rays per wave (203 = 25 * 8 + 3 = 12 * 16 + 11 = 6 * 32 + 11); the second view starts
    # after a partial tile; odd non-square planes
    "list": dict(N=2, R=203, img=None, tile_w=0, H=33, W=47, seed=5100),
    # screen tiles of both kernels: 3 (8 x 4 pixels) resp. 6 (4 x 2, 4 x 4) tiles per row — no power of two
    "tiles": dict(N=1, R=24 * 20, img=(24, 20), tile_w=24, H=64, W=48, seed=5203),
    # grid 131 = 128 swizzled blocks + 3 identity blocks of one wave, the last tile partial
    "tail": dict(N=1, R=131 * 32 - 5, img=None, tile_w=0, H=40, W=56, seed=5300),
    # 3 x 685 = 2055 tiles on 4-wave workgroups: grid 514 = 4 * 128 + 2, the last workgroup has 3 tiles, a partial tile per view
    "wide4": dict(N=3, R=21900, img=None, tile_w=0, H=33, W=47, seed=5400),
    # two 256 x 128 images: 32 x 32 tiles each = 2 x 2 super-tiles, 2048 tiles, the blocked order over two views
    "blocked": dict(N=2, R=256 * 128, img=(256, 128), tile_w=256, H=64, W=48, seed=5500),
    # two 128 x 256 images: 16 x 64 tiles each, ONE column of super-tiles.  Not in the issue's table: its 256 x 128 `blocked` gives
    # 32 x 32 tiles, so tiles_x == tiles_y there, and only this shape reaches the blocked order with tiles_x != tiles_y
    "blocked_tall": dict(N=2, R=128 * 256, img=(128, 256), tile_w=128, H=48, W=64, seed=5205),
}

# (Sc, Sf) -> NF, the fine-depth capacity of the instantiation (p3d_render_plan.hpp): 48 / 96 exactly, Sf <= 64 padded to 64, else 0
NF = {(48, 48): 48, (96, 96): 96, (64, 96): 96, (12, 7): 64, (100, 96): 0, (20, 136): 0, (16, 0): 64, (4, 4): 64, (4, 0): 64}
RATES_SMALL = [(48, 48), (96, 96), (64, 96), (12, 7), (100, 96), (20, 136), (16, 0)]

OPTION_SETS = (
    dict(kw=dict(triplane_crop=0.1, cull_clouds=0.5, force_sigmoid=True), white_back=True, use_triplane=1),
    dict(kw=dict(triplane_crop=0.05, binarize_clouds=0.4, force_sigmoid=False), white_back=True, use_triplane=1),
    dict(kw=dict(force_sigmoid=False), white_back=False, use_triplane=0),
)
RNG_SEED = 0x0123_4567_89AB_CDEF


def _case(shape, Sc, Sf, small, early=True, spacing="fixed", opt=0, kind="render", tile_w=None, per_view=False, rng=False):
    tw = SHAPES[shape]["tile_w"] if tile_w is None else tile_w
    cid = f"{shape}-{Sc}p{Sf}-{ {False: 'wave32', True: 'auto'}.get(small, small)}-{'early' if early else 'all'}-{spacing}-o{opt}"
    cid += {"render": "", "dump": "-dump", "wo": "-wo"}[kind] + ("" if tw == SHAPES[shape]["tile_w"] else "-untiled")
    cid += ("-perview" if per_view else "") + ("-rng" if rng else "")
    return dict(id=cid, shape=shape, Sc=Sc, Sf=Sf, small=small, early=early, spacing=spacing, opt=opt, kind=kind, tile_w=tw,
                per_view=per_view, rng=rng)


def _build_cases():
    cases = []
    for si, shape in enumerate(("list", "tiles")):
        # every rate x kernel x early-outs, fixed spacing; the option sets rotate so that each meets each kernel kind at each NF
        for ri, (Sc, Sf) in enumerate(RATES_SMALL):
            for ki, small in enumerate(("quad", "pair", False)):
                for early in (True, False):
                    cases.append(_case(shape, Sc, Sf, small, early, opt=(si + ri + ki + early) % 3))
        # the other two spacings at 48+48 and 96+96 (with the 32-rays-per-wave kernel: the LDS-resident 96-key instantiation)
        for ri, (Sc, Sf) in enumerate(((48, 48), (96, 96))):
            for ki, small in enumerate(("quad", "pair", False)):
                for early in (True, False):
                    for pi, spacing in enumerate(("limits", "disparity")):
                        cases.append(_case(shape, Sc, Sf, small, early, spacing, opt=(si + ri + ki + early + pi) % 3))
        # dump launches (k_render<NF, DUMP>: every sample decoded, one instantiation per NF)
        for ri, (Sc, Sf) in enumerate(((48, 48), (96, 96), (12, 7), (100, 96))):
            cases.append(_case(shape, Sc, Sf, True, early=False, opt=(si + ri) % 3, kind="dump"))
        cases.append(_case(shape, 48, 48, True, early=False, spacing="limits", opt=si, kind="dump"))
        # weights-only launches (k_render_slots<4, 48 | 96, true, true>): the heuristic's choice and the forced one
        for Sc, Sf in ((48, 48), (96, 96)):
            for spacing in ("fixed", "limits"):
                for tw in sorted({SHAPES[shape]["tile_w"], 0}, reverse=True):
                    cases.append(_case(shape, Sc, Sf, True if spacing == "fixed" else "quad", spacing=spacing,
                                       opt=(si + (Sc == 96)) % 2, kind="wo", tile_w=tw))
    cases.append(_case("list", 48, 48, "quad", per_view=True))
    cases.append(_case("list", 96, 96, False, per_view=True))
    cases.append(_case("tiles", 48, 48, "quad", rng=True))
    cases.append(_case("tiles", 96, 96, False, rng=True, opt=1))
    # the swizzled grid with an identity tail
    for (Sc, Sf), spacing, opt in (((48, 48), "fixed", 0), ((12, 7), "fixed", 1), ((96, 96), "fixed", 0), ((96, 96), "limits", 1)):
        cases.append(_case("tail", Sc, Sf, False, spacing=spacing, opt=opt))
    cases.append(_case("tail", 12, 7, False, early=False, opt=2))
    # 4-wave workgroups with an identity tail and a short last workgroup; the blocked order
    for shape in ("wide4", "blocked", "blocked_tall"):
        cases.append(_case(shape, 4, 4, False))
    ids = [c["id"] for c in cases]
    assert len(set(ids)) == len(ids)
    return cases


CASES = _build_cases()
CASE = {c["id"]: c for c in CASES}


def ids(pred=lambda c: True):
    return [c["id"] for c in CASES if pred(c)]


# ---- what a case names: the launch, derived from the case's row alone (the CPU test holds the plan to it, the GPU test the launch) --
def rendering_options(case):
    o = OPTION_SETS[case["opt"]]
    ro = dict(T.RENDERING_KWARGS, depth_resolution=case["Sc"], depth_resolution_importance=case["Sf"], white_back=o["white_back"],
              use_triplane=o["use_triplane"])
    if case["spacing"] == "limits":
        ro["ray_start"] = ro["ray_end"] = "auto"
    elif case["spacing"] == "disparity":
        ro["disparity_space_sampling"] = True
    return ro, dict(o["kw"])


def hip_opts(ops, case, fast):
    ro, kw = rendering_options(case)
    return ops.make_opts(ro, early_out=case["early"], small_launch_kernel=case["small"], fast_color=fast, **kw)


def plan_request(ops, case, fast):
    """(N, R, ray_tile_w, Sc, Sf, flags, dumps, limits): the arguments of the plan (tests/render_plan_host.cpp's `p` line)."""
    from panic3d_amd import _lib
    s = SHAPES[case["shape"]]
    flags = hip_opts(ops, case, fast).flags | (_lib.P3D_FLAG_WEIGHTS_ONLY if case["kind"] == "wo" else 0)
    flags |= _lib.P3D_FLAG_PER_VIEW_CLAMP if case["per_view"] else 0
    return (s["N"], s["R"], case["tile_w"], case["Sc"], case["Sf"], flags, int(case["kind"] == "dump"), int(case["spacing"] == "limits"))


def expected_launch(case, fast):
    """The launch the case's row names: instantiation, samples per wave-step, tile_w, tiles_x, tiles, grid, block, full decode steps."""
    s = SHAPES[case["shape"]]
    N, R, Sc, Sf = s["N"], s["R"], case["Sc"], case["Sf"]
    nf, F = NF[(Sc, Sf)], int(bool(fast) and Sf > 0)
    small = case["small"]
    if small is True:  # the size heuristic: these shapes hold at most 8192 rays -> the four-slot kernel
        assert N * R <= 8192
        small = "quad"
    if case["kind"] == "dump":
        slots, name = 1, f"k_render<{nf},1,{F},0,0>"
    elif small is False:
        slots = 1
        tcg = int(nf == 96 and case["early"] and case["spacing"] == "fixed")
        name = f"k_render<{nf},0,{F},{int(case['early'])},{tcg}>"
    else:
        slots = 4 if small == "quad" else 2
        wo = case["kind"] == "wo" and F == 1  # the exact mode has no weights-only kernel: the hint is ignored there
        assert case["kind"] != "wo" or (slots == 4 and nf in (48, 96))
        name = f"k_render_slots<{slots},{nf},{F},{int(wo)}>"
    rpw = 32 // slots
    tw, th = (8, 4) if slots == 1 else (4, rpw // 4)
    tile_w = case["tile_w"]
    if tile_w:
        tiles_x, per_img = tile_w // tw, (tile_w // tw) * (R // tile_w // th)
    else:
        tiles_x, per_img = 0, -(-R // rpw)
    ntiles = N * per_img
    # waves per workgroup: the small-launch kernels run four; k_render one below 512 tiles per wave of the workgroup
    nw = 4 if slots > 1 else 4 if ntiles // 4 >= 512 else 2 if ntiles // 2 >= 512 else 1
    steps = -(-Sc // slots) + (-(-(Sc + Sf) // slots) if Sf > 0 else 0)
    return dict(name=name, slots=slots, tile_w=tile_w, tiles_x=tiles_x, ntiles=ntiles, grid=-(-ntiles // nw), block=64 * nw,
                steps_full=ntiles * steps)


# ---- scenes -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene(shape):
    """planes (smooth 8, scale 4), decoder (sigma gain 30) — the range of the golden fixtures, inside the documented domain of the
    tolerance decoder (csrc/p3d_decode.hpp) — and rays that look at the box, every 7th reversed so that it looks away from it.
    A reversed ray misses the planes, not the decoder: on zero features the decoder still answers a density, so such a ray is
    empty only where a mask removes its samples (the crop mask tests x and z: a ray that leaves along y keeps its weight, at
    positions up to 2.5 from the centre)."""
    s = SHAPES[shape]
    N, R, seed = s["N"], s["R"], s["seed"]
    planes = T.make_planes(seed, N, s["H"], s["W"], scale=4.0, smooth=8)
    raw = T.make_decoder_params(seed + 1, 1.0, 30.0)
    if s["img"] is None:  # as test_hip_parity._random_config: origins on the unit sphere, targets inside the box
        rng = np.random.default_rng(seed)
        o = rng.standard_normal((N, R, 3)); o /= np.linalg.norm(o, axis=-1, keepdims=True)
        tgt = rng.uniform(-0.3, 0.3, (N, R, 3)) * BOX_WARP
        d = tgt - o; d /= np.linalg.norm(d, axis=-1, keepdims=True)
        o, d = o.astype(np.float32), d.astype(np.float32)
    else:  # the middle rows of a perspective camera's square image, one camera per view
        from panic3d_amd import cameras
        w, h = s["img"]
        res = max(w, h)
        lab = torch.stack([cameras.camera_label(5.0 + 10 * n, 30.0 + 140 * n, 1.0, 30.0) for n in range(N)])
        o, d = cameras.rays_from_label(lab, res)
        y0, x0 = (res - h) // 2, (res - w) // 2
        cut = lambda t: t.reshape(N, res, res, 3)[:, y0:y0 + h, x0:x0 + w].reshape(N, R, 3).contiguous().numpy()  # noqa: E731
        o, d = cut(o), cut(d)
    d = d.copy()
    d[:, ::7] = -d[:, ::7]
    return dict(planes=planes, raw=raw, o=np.ascontiguousarray(o), d=np.ascontiguousarray(d))


@functools.lru_cache(maxsize=None)
def _ray_limits(shape):
    from panic3d_amd import cameras
    sc = scene(shape)
    rs, re = cameras.patch_ray_limits(*cameras.ray_limits_box(torch.from_numpy(sc["o"]), torch.from_numpy(sc["d"]), BOX_WARP))
    N, R = sc["o"].shape[:2]
    return rs.reshape(N, R).numpy(), re.reshape(N, R).numpy()


@functools.lru_cache(maxsize=None)
def _draws(shape, Sc, Sf, auto_limits, rng):
    s = SHAPES[shape]
    if rng:
        from oracle import oracle
        return oracle.device_draws(RNG_SEED, s["N"], s["R"], Sc, Sf)
    return T.make_random_draws(s["seed"] + 2, s["N"], s["R"], Sc, Sf, auto_limits=auto_limits)


def inputs(case):
    """Everything a render of the case takes, as numpy arrays (the draws are None where the kernel makes them)."""
    sc = scene(case["shape"])
    ro, kw = rendering_options(case)
    jit, u = _draws(case["shape"], case["Sc"], case["Sf"], case["spacing"] == "limits", case["rng"])
    return dict(sc, ro=ro, kw=kw, jit=jit, u=u if case["Sf"] > 0 else None,
                limits=_ray_limits(case["shape"]) if case["spacing"] == "limits" else None, rng_seed=RNG_SEED if case["rng"] else None)


# ---- the reference: the oracle's render, once per (shape, rate, spacing, options, clamp, draws) ------------------------------------
def reference_key(case):
    return (case["shape"], case["Sc"], case["Sf"], case["spacing"], case["opt"], case["per_view"], case["rng"])


@functools.lru_cache(maxsize=None)
def _reference(key, dumps):
    from oracle import oracle
    shape, Sc, Sf, spacing, opt, per_view, rng = key
    inp = inputs(_case(shape, Sc, Sf, False, spacing=spacing, opt=opt, per_view=per_view, rng=rng))
    oo = oracle.make_opts(inp["ro"], **inp["kw"])
    om = oracle.prescale_mlp(*inp["raw"])
    N, R = inp["o"].shape[:2]
    views = [slice(n, n + 1) for n in range(N)] if per_view else [slice(0, N)]  # per-view clamp: N calls of the reference
    outs = []
    for v in views:
        rows = slice(v.start * R, v.stop * R)
        outs.append(oracle.render(inp["planes"][v], inp["o"][v], inp["d"][v], inp["jit"][v], None if inp["u"] is None else inp["u"][rows],
                                  om, oo, dumps=dumps, ray_limits=None if inp["limits"] is None else tuple(x[v] for x in inp["limits"])))
    ref = {k: np.concatenate([o[i] for o in outs]) for i, k in enumerate(OUTPUTS)}
    for a in ref.values():
        a.setflags(write=False)
    if dumps:
        assert not per_view
        d = outs[0][4]
        d.pop("rgb_coarse")  # 32 floats per coarse sample: the one large dump, and nothing here reads it
        if Sf > 0:
            d["depths_sorted"] = np.take_along_axis(np.concatenate([d["depths_coarse"], d["depths_fine"]], 1), d["perm"], 1)
            d["sigma_sorted"] = np.take_along_axis(np.concatenate([d["sigma_coarse"], d["sigma_fine"]], 1), d["perm"], 1)
        else:
            d["depths_sorted"], d["sigma_sorted"] = d["depths_coarse"], d["sigma_coarse"]
        for a in d.values():
            a.setflags(write=False)
        ref["dumps"] = d
    return ref


def reference(case, dumps=False):
    """dict(feat, depth, wsum, xyz [, dumps]) of the oracle, read-only and shared by every case with the same inputs."""
    return _reference(reference_key(case), bool(dumps))


# ---- the gate --------------------------------------------------------------------------------------------------------------------
def errors(got, ref):
    """name -> the largest |got - oracle| over the finite entries (what the tolerance gate bounds), for every output in `got`."""
    out = {}
    for k in OUTPUTS:
        if got.get(k) is None:
            continue
        a, b = np.asarray(got[k]).reshape(np.asarray(ref[k]).shape), np.asarray(ref[k])
        ok = np.isfinite(a) & np.isfinite(b)
        out[k] = float(np.abs(a[ok].astype(np.float64) - b[ok]).max()) if ok.any() else 0.0
    return out


def gate(got, ref, exact):
    """The violations of a render (dict name -> array; a None output is not checked) against the oracle's (`ref`).
    exact: every output equal bit for bit (NaNs in the same places).
    tolerance mode: the non-finite pattern of every output identical to the oracle's, and on EVERY ray |got - oracle| <= FAST_MAX —
    no allowance of rays, no median clause."""
    bad = []
    for k in OUTPUTS:
        if got.get(k) is None:
            continue
        b = np.asarray(ref[k])
        a = np.asarray(got[k])
        if a.size != b.size:
            bad.append(f"{k}: shape {a.shape} for {b.shape}")
            continue
        a = a.reshape(b.shape)
        if exact:
            if not np.array_equal(a, b, equal_nan=True):
                ne = ~((a == b) | (np.isnan(a) & np.isnan(b)))
                rays = np.flatnonzero(ne.reshape(-1, a.shape[-1]).any(-1))
                bad.append(f"{k}: {rays.size} rays differ from the oracle's bits (first {rays[:4].tolist()}, max {errors({k: a}, ref)[k]:.3g})")
            continue
        fa, fb = np.isfinite(a), np.isfinite(b)
        same = (fa & fb) | (np.isnan(a) & np.isnan(b)) | (np.isinf(a) & np.isinf(b) & (np.signbit(a) == np.signbit(b)))
        if not same.all():
            bad.append(f"{k}: the non-finite pattern differs on {int((~same).reshape(-1, a.shape[-1]).any(-1).sum())} rays")
        err = np.where(fa & fb, np.abs(np.where(fa, a, 0).astype(np.float64) - np.where(fb, b, 0)), 0.0).reshape(-1, a.shape[-1]).max(-1)
        over = np.flatnonzero(err > FAST_MAX[k])
        if over.size:
            bad.append(f"{k}: {over.size} rays beyond {FAST_MAX[k]:g} (first {over[:4].tolist()}, max {err.max():.3g})")
    return bad
