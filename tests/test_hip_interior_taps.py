"""GPU: k_render's interior gather set-up (csrc/p3d_decode.hpp, INTERIOR; the launch's decision in csrc/p3d_render_plan.hpp) against
the generic one, bit for bit, and against the CPU oracle.

Where the crop keeps every bilinear tap of the x and z axes inside the planes, the decodes of k_render's early-out instantiations drop
the range tests of those axes and address a texel's neighbours through the load's immediate and scalar offsets.  The same operations
on the same operands: every case renders with the launch's own choice and with P3D_FLAG_GENERIC_TAPS, and the four outputs must be the
same BITS (NaNs included); the exact mode must also be the oracle's bits.  `stats["interior_taps"]` says which set-up ran.

Shapes, the smallest that reach every site: 16 x 16 planes of 32 channels with a crop of ONE texel (box_warp 0.7, crop 0.7 / 16: the plan
accepts with no margin to spare, the borders are a texel away); two views of 35 rays in one launch as a ray list (the second 32-ray tile
is partial); 48+48 samples, and 96+96 for the kernel that recomputes its coarse depths.  Per view 21 camera rays and 14 placed ones:

  x / z on the limit   origins with x (or z) exactly +L, -L and one float beyond each, direction (0, 1, 0): px = ox + t * 0 = ox for every
                       sample, so all samples of the first kind sit on the limit (decoded: |p| > L is false) and all of the second are cropped
  y leaves the planes  those rays run from y = -0.5 to y = +0.5 through a box of half-width 0.35: bottom and top, inside in x and z
  crossing             a ray along x with z on the limit and one along z with x on the limit: cropped, decoded, cropped
  NaN / inf            a NaN in the origin's x only, in z only, in y only, and an infinite direction (in y: the samples stay uncropped)

plane_mode 0 and 1 (plane 2 takes y as its column with 1), the exact and the tolerance mode.  A launch the plan refuses (W != H) must
report the generic set-up and give the same bits with and without the switch.  k_render_slots did not get the interior form (it keeps
the generic set-up), so no small-launch case here beyond the report.
"""
import functools

import numpy as np
import pytest
import torch

import p3d_testing as T

pytestmark = pytest.mark.gpu

OUTPUTS = ("feat", "depth", "wsum", "xyz")
BOX, CROP = 0.7, 0.7 / 16
L = np.float32(BOX / 2 - CROP)  # crop_limit as ops.make_opts makes it
KW = dict(triplane_crop=CROP, cull_clouds=0.5, force_sigmoid=True)
N_CAMERA, R = 21, 35


@pytest.fixture(scope="module")
def hip():
    import panic3d_amd
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    panic3d_amd._lib.lib()  # must load: no fallback
    return panic3d_amd


@pytest.fixture(autouse=True)
def stop_at_a_device_fault():
    """A device fault ends the session: nothing more is launched on a GPU that has faulted."""
    yield
    try:
        torch.cuda.synchronize()
    except Exception as e:  # noqa: BLE001
        pytest.exit(f"device fault: {e}", returncode=3)


def placed_rays():
    """(origins, directions) [14, 3] of the placed rays, and the index ranges of their kinds"""
    up, dn = np.nextafter(L, np.float32(np.inf)), np.nextafter(-L, np.float32(-np.inf))
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    o, d = [], []
    for x in (L, up, -L, dn):  # x on the limit / one float beyond
        o.append((x, -1.0, 0.05)); d.append((0.0, 1.0, 0.0))
    for z in (L, up, -L, dn):  # z
        o.append((-0.03, -1.0, z)); d.append((0.0, 1.0, 0.0))
    o.append((-1.0, 0.01, L)); d.append((1.0, 0.0, 0.0))   # along x, z on the limit
    o.append((-L, 0.02, -1.0)); d.append((0.0, 0.0, 1.0))  # along z, x on the limit
    o.append((nan, -1.0, 0.04)); d.append((0.0, 1.0, 0.0))
    o.append((0.02, -1.0, nan)); d.append((0.0, 1.0, 0.0))
    o.append((0.02, nan, 0.04)); d.append((0.0, 1.0, 0.0))
    o.append((0.02, -1.0, 0.04)); d.append((0.0, inf, 0.0))
    return np.array(o, np.float32), np.array(d, np.float32)


ON_LIMIT, BEYOND, CROSSING, NONFINITE = (0, 2, 4, 6), (1, 3, 5, 7), (8, 9), (10, 11, 12, 13)  # indices into the placed rays


@functools.lru_cache(maxsize=None)
def scene(Sc, Sf, H=16, W=16):
    import panic3d_amd as P
    from oracle import oracle
    planes = T.make_planes(9501, 1, H, W, scale=4.0, smooth=3)  # ONE subject, shared by the two views
    mlp = oracle.prescale_mlp(*T.make_decoder_params(9502, 1.0, 30.0))
    labels = torch.cat([P.cameras.camera_label(20.0 - 50.0 * v, 15.0, 1.0, 30.0)[None] for v in range(2)])
    co, cd = (x.numpy()[:, ::3][:, :N_CAMERA] for x in P.cameras.rays_from_label(labels, 8))
    po, pd = placed_rays()
    o = np.ascontiguousarray(np.concatenate([co, np.stack([po, po])], axis=1), np.float32)
    d = np.ascontiguousarray(np.concatenate([cd, np.stack([pd, pd])], axis=1), np.float32)
    assert o.shape == (2, R, 3)
    jit, u = T.make_random_draws(9503, 2, R, Sc, Sf)
    sc = dict(planes=planes, mlp=mlp, o=o, d=d, jit=jit, u=u)
    for a in (planes, o, d, jit, u) + tuple(mlp):
        a.setflags(write=False)
    return sc


def options(Sc, Sf, plane_mode):
    return dict(T.RENDERING_KWARGS, box_warp=BOX, depth_resolution=Sc, depth_resolution_importance=Sf, use_triplane=plane_mode)


@functools.lru_cache(maxsize=None)
def reference(Sc, Sf, plane_mode, H=16, W=16):
    """the oracle's four outputs"""
    from oracle import oracle
    sc = scene(Sc, Sf, H, W)
    ref = oracle.render(np.concatenate([sc["planes"]] * 2), sc["o"], sc["d"], sc["jit"], sc["u"], sc["mlp"],
                        oracle.make_opts(options(Sc, Sf, plane_mode), **KW))
    for a in ref:
        a.setflags(write=False)
    return dict(zip(OUTPUTS, ref))


def dev(a):
    return torch.from_numpy(np.array(a, np.float32)).cuda()  # (a copy: the shared scenes are read-only)


def render_both(hip, Sc, Sf, plane_mode, fast, H=16, W=16):
    """the launch's own choice and the forced generic set-up: ({name: tensor}, stats) each"""
    sc = scene(Sc, Sf, H, W)
    args = (hip.ops.planes_to_nhwc(dev(sc["planes"])), dev(sc["o"]), dev(sc["d"]), dev(sc["jit"]), dev(sc["u"]), tuple(dev(x) for x in sc["mlp"]))
    opts = hip.ops.make_opts(options(Sc, Sf, plane_mode), small_launch_kernel=False, fast_color=fast, **KW)
    res = []
    for o in (opts, hip.ops._with_flag(opts, hip._lib.P3D_FLAG_GENERIC_TAPS)):
        st = {}
        out = hip.ops.render(*args, o, stats=st)
        torch.cuda.synchronize()
        res.append((dict(zip(OUTPUTS, out)), st))
    return res


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("plane_mode", [0, 1])
def test_the_placed_rays_are_where_the_docstring_says(oracle, plane_mode):
    """What the launches below rely on, established on the inputs and on the oracle's outputs."""
    import panic3d_amd as P
    sc = scene(48, 48)
    o, d = sc["o"][0, N_CAMERA:], sc["d"][0, N_CAMERA:]
    t = np.linspace(0.5, 1.5, 97, dtype=np.float32)[:, None]
    for i in ON_LIMIT + BEYOND:
        px, pz = o[i, 0] + t * d[i, 0], o[i, 2] + t * d[i, 2]
        assert (px == o[i, 0]).all() and (pz == o[i, 2]).all()  # o + t * 0: every sample keeps the origin's x and z
        cropped = (np.abs(px) > L) | (np.abs(pz) > L)
        assert cropped.all() == (i in BEYOND) and cropped.any() == (i in BEYOND), i
        py = (o[i, 1] + t * d[i, 1]) * np.float32(2.0 / BOX)
        assert (py < -1).any() and (py > 1).any() and (np.abs(py) < 1).any()  # below, inside and above the planes
    opts = P.ops.make_opts(options(48, 48, plane_mode), **KW)
    assert np.float32(opts.crop_limit) == L and opts.plane_mode == plane_mode
    ref = reference(48, 48, plane_mode)
    w = ref["wsum"][:, N_CAMERA:, 0]
    assert (w[:, list(BEYOND)] == 0).all() and (w[:, list(ON_LIMIT)] > 0).any()  # cropped rays are empty, rays on the limit are not
    assert (w[:, list(CROSSING)] > 0).any()
    cam = ref["wsum"][:, :N_CAMERA, 0]
    assert (cam > 0.5).any() and (cam < 0.5).any()  # surfaces and (nearly) empty rays among the camera rays


@pytest.mark.parametrize("fast", [False, True], ids=["exact", "tolerance"])
@pytest.mark.parametrize("S,plane_mode", [(48, 0), (48, 1), (96, 1)])  # (one 96+96 case: the kernel that recomputes its coarse depths)
def test_interior_taps_are_the_generic_bits(hip, oracle, S, plane_mode, fast):
    (own, st_own), (gen, st_gen) = render_both(hip, S, S, plane_mode, fast)
    assert st_own["interior_taps"] is True and st_gen["interior_taps"] is False, (st_own, st_gen)
    assert st_own["small_launch_kind"] is None and st_own["decode_steps"] == st_gen["decode_steps"] < st_own["decode_steps_full"]
    for k in OUTPUTS:
        assert same_bits(own[k], gen[k]), (S, plane_mode, fast, k, int((own[k] != gen[k]).sum()))
    if not fast:
        ref = reference(S, S, plane_mode)
        for k in OUTPUTS:
            got = own[k].cpu().numpy()
            assert np.array_equal(got, ref[k], equal_nan=True), (S, plane_mode, k, int((got != ref[k]).sum()))


@pytest.mark.parametrize("fast", [False, True], ids=["exact", "tolerance"])
def test_a_refused_launch_runs_the_generic_set_up(hip, oracle, fast):
    """16 x 32 planes: W != H, the plan refuses; the switch then changes nothing, and the launch says which set-up it ran."""
    (own, st_own), (gen, st_gen) = render_both(hip, 48, 48, 1, fast, H=16, W=32)
    assert st_own["interior_taps"] is False and st_gen["interior_taps"] is False
    for k in OUTPUTS:
        assert same_bits(own[k], gen[k]), (fast, k)
    if not fast:
        ref = reference(48, 48, 1, 16, 32)
        for k in OUTPUTS:
            assert np.array_equal(own[k].cpu().numpy(), ref[k], equal_nan=True), k


def test_small_launches_report_the_generic_set_up(hip):
    """k_render_slots keeps the generic set-up: the report says so (its bits are test_hip_quad_gather.py's business)."""
    sc = scene(48, 48)
    args = (hip.ops.planes_to_nhwc(dev(sc["planes"])), dev(sc["o"]), dev(sc["d"]), dev(sc["jit"]), dev(sc["u"]), tuple(dev(x) for x in sc["mlp"]))
    st = {}
    hip.ops.render(*args, hip.ops.make_opts(options(48, 48, 1), small_launch_kernel="quad", **KW), stats=st)
    torch.cuda.synchronize()
    assert st["small_launch_kind"] == "quad" and st["interior_taps"] is False
