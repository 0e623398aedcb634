"""GPU: k_render's two draw rows loaded as 16-byte pieces and its stratified depths shared between the two halves of a wave
(csrc/p3d_kernels.hip, csrc/p3d_importance.hpp, the launch's decision in csrc/p3d_render_plan.hpp), bit for bit against the CPU oracle.

Where the launch allows it (no in-kernel draws, a 16-byte aligned base pointer, a row length that is a multiple of 8 floats) half h of a
wave requests its half of a ray's jitter row in front of the weight copy, makes the stratified depths [h * Sc/2, (h + 1) * Sc/2), and one
exchange gives both halves the ray's out-of-order flag (with the comparison across the cut) and extrema; the `u` half row comes as
pieces too, and the 96-key kernel without a coarse column reads the jitter row one batch of eight ahead.  The shapes are the smallest at
which a wrong split, a wrong piece or a stale prefetch shows:

  rays     R = 40 (the second 32-ray tile is partial: its inactive lanes load a valid row and store nothing) and R = 64 as an 8-wide
           image; two views in one launch (the second view's rows start R * Sc floats in)
  samples  48+48 (the production instantiation), 96+96 without the small-launch kernels (the kernel without a coarse column: twelve
           prefetched batches), 96+96 with per-ray limits (the LDS-resident 96-key kernel), 40+56 (the padded 64-key path, Sc/2 = 20),
           24+24 (three pieces per half), 20+13 (Sc % 8 != 0: the scalar loads), 12+48 (Sc % 8 != 0 while u qualifies)
  pointers jitter and u as contiguous views that start one float into a larger buffer (data_ptr() % 16 == 4: the scalar loads, the same
           bits), and jitter alone
  the cut  injected jitter values, asserted below on the oracle's own depths: rays whose only reversed pair is t[Sc/2 - 1] > t[Sc/2],
           rays whose only one lies inside half 0 / inside half 1, rays with their minimum in half 1 and their maximum in half 0, and
           most rays sorted, so that the wave's ballot sees a mix

Every case runs with the early-outs on and off; the dump kernel's depths_coarse, depths_fine and inds are compared in every entry (each
half writes its own), depths_sorted and the clamp range (tminmax) with them; the small-launch kernels, whose code does not take the
pieces, run on the same inputs; the tolerance mode stays inside FAST_MAX of the exact one.
"""
import functools

import numpy as np
import pytest
import torch

import p3d_testing as T
from test_hip_parity import FAST_MAX  # the ONE definition of the tolerance mode's bound

pytestmark = pytest.mark.gpu  # (every test of the file: the fault check below runs behind each of them)

OUTPUTS = ("feat", "depth", "wsum", "xyz")
# (Sc, Sf, per-ray limits)
CASES = {"S48": (48, 48, False), "S96_no_column": (96, 96, False), "S96_limits": (96, 96, True), "S40_56_padded": (40, 56, False),
         "S24": (24, 24, False), "S20_13_scalar": (20, 13, False), "S12_48_u_only": (12, 48, False)}
KW = dict(triplane_crop=0.16, cull_clouds=0.5, force_sigmoid=True)
RES = 8  # the image is 8 rays wide; R = 40 is its first five rows


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


def dev(a):
    return torch.from_numpy(np.array(a, np.float32)).cuda()  # (a copy: the shared scenes are read-only)


def off_by_one_float(a):
    """`a` on the device as a contiguous view that starts one float into a larger buffer: not 16-byte aligned, and not copied by ops._chk"""
    a = np.array(a, np.float32)  # (a copy: the shared scenes are read-only)
    buf = torch.zeros(a.size + 8, dtype=torch.float32, device="cuda")
    v = buf[1:1 + a.size].view(a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def options(case):
    Sc, Sf, limits = CASES[case]
    ro = dict(T.RENDERING_KWARGS, depth_resolution=Sc, depth_resolution_importance=Sf)
    if limits:
        ro["ray_start"] = ro["ray_end"] = "auto"
    return ro


# which rays of a view get which injection (the others keep torch.rand's values: sorted)
CUT, IN0, IN1, EXTREMA = (1, 9, 33, 38), (2, 17, 34), (5, 21, 39), (7, 12, 36)


def inject(jit, Sc):
    """jit [views, R, Sc, 1], in place.  A pair (1.5, 0.1) reverses the two neighbours it sits on and nothing else (the spacing is one
    depth_delta per index); -(Sc/2 + 3 + Sc/4) puts a depth of half 1 a quarter of the range in front of the ray's first (with per-ray
    limits: in front of every ray's first), 2 * Sc one of half 0 a whole range behind its last."""
    c = Sc // 2
    for r in CUT:
        jit[:, r, c - 1, 0], jit[:, r, c, 0] = 1.5, 0.1
    for r in IN0:
        jit[:, r, 2, 0], jit[:, r, 3, 0] = 1.5, 0.1
    for r in IN1:
        jit[:, r, c + 1, 0], jit[:, r, c + 2, 0] = 1.5, 0.1
    for r in EXTREMA:
        jit[:, r, c + 1, 0], jit[:, r, 1, 0] = -(c + 3.0 + Sc // 4), 2.0 * Sc


@functools.lru_cache(maxsize=None)
def scene(case, R, views=1):
    import panic3d_amd as P
    from oracle import oracle
    Sc, Sf, limits = CASES[case]
    planes = T.make_planes(9401, 1, 64, 64, scale=4.0, smooth=8)  # ONE subject: its planes are shared by the views
    mlp = oracle.prescale_mlp(*T.make_decoder_params(9402, 1.0, 30.0))
    labels = torch.cat([P.cameras.camera_label(15.0 - 30.0 * v, 25.0, 1.0, 30.0)[None] for v in range(views)])
    o, d = P.cameras.rays_from_label(labels, RES)
    o, d = (np.ascontiguousarray(x.numpy()[:, :R]) for x in (o, d))
    jit, u = T.make_random_draws(9403, views, R, Sc, Sf)
    jit, u = jit.copy(), u.copy()
    inject(jit, Sc)
    lim = None
    if limits:
        ro = options(case)
        rs, re = P.cameras.patch_ray_limits(*P.cameras.ray_limits_box(torch.from_numpy(o), torch.from_numpy(d), ro["box_warp"]))
        lim = tuple(np.ascontiguousarray(x.reshape(views, -1).numpy()) for x in (rs, re))
    sc = dict(planes=planes, mlp=mlp, o=o, d=d, jit=jit, u=u, lim=lim)
    for a in (planes, o, d, jit, u) + tuple(mlp) + (lim or ()):
        a.setflags(write=False)
    return sc


@functools.lru_cache(maxsize=None)
def reference(case, R, views=1):
    """the oracle's four outputs and its dumps"""
    from oracle import oracle
    sc = scene(case, R, views)
    *ref, dm = oracle.render(np.concatenate([sc["planes"]] * views), sc["o"], sc["d"], sc["jit"], sc["u"], sc["mlp"],
                             oracle.make_opts(options(case), **KW), dumps=True, ray_limits=sc["lim"])
    for a in ref + list(dm.values()):
        a.setflags(write=False)
    return dict(zip(OUTPUTS, ref)), dm


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def launch_args(hip, sc, jit=None, u=None):
    return (hip.ops.planes_to_nhwc(dev(sc["planes"])), dev(sc["o"]), dev(sc["d"]), dev(sc["jit"]) if jit is None else jit,
            dev(sc["u"]) if u is None else u, tuple(dev(x) for x in sc["mlp"]))


def check_all_kernels(hip, case, R, views, args, what):
    """every kernel of the launch against the oracle: the four outputs bit for bit, the dumps entry by entry, the tolerance mode"""
    sc = scene(case, R, views)
    ref, rdm = reference(case, R, views)
    Sc, Sf, _ = CASES[case]
    lim = None if sc["lim"] is None else tuple(dev(x) for x in sc["lim"])
    tile_w = RES if R == RES * RES else 0
    ro = options(case)
    exact = None
    for small in (False, "pair", "quad"):  # (the small-launch kernels keep their scalar loads: a regression check on the same inputs)
        for early in (True, False):
            st = {}
            out = hip.ops.render(*args, hip.ops.make_opts(ro, early_out=early, small_launch_kernel=small, **KW), ray_tile_w=tile_w, stats=st,
                                 ray_limits=lim)
            torch.cuda.synchronize()
            assert st["small_launch_kind"] == (small or None), st
            got = {k: v.cpu().numpy() for k, v in zip(OUTPUTS, out)}
            for k in OUTPUTS:
                assert same(got[k], ref[k]), (what, case, R, views, small, early, k, int((got[k] != ref[k]).sum()))
            if early and small is False:
                exact = got
                assert st["decode_steps"] < st["decode_steps_full"], st  # the early-outs did run
    # the dump kernel: each half writes the entries of its own depths and draws
    out = hip.ops.render(*args, hip.ops.make_opts(ro, small_launch_kernel=False, **KW), ray_tile_w=tile_w, dumps=True, ray_limits=lim)
    torch.cuda.synchronize()
    hdm = {k: v.cpu().numpy() for k, v in out[4].items()}
    for k, v in zip(OUTPUTS, out):
        assert same(v.cpu().numpy(), ref[k]), (what, case, R, views, "dumps", k)
    for k in ("depths_coarse", "depths_fine", "inds", "tminmax"):
        assert np.array_equal(hdm[k], rdm[k]), (what, case, R, views, k, int((hdm[k] != rdm[k]).sum()))
    all_d = np.concatenate([rdm["depths_coarse"], rdm["depths_fine"]], axis=1)
    assert np.array_equal(hdm["depths_sorted"], np.take_along_axis(all_d, rdm["perm"].astype(np.int64), axis=1)), (what, case, R, views)
    # the tolerance mode of the final pass against the exact one
    fast = hip.ops.render(*args, hip.ops.make_opts(ro, small_launch_kernel=False, fast_color=True, **KW), ray_tile_w=tile_w, ray_limits=lim)
    torch.cuda.synchronize()
    for k, v in zip(OUTPUTS, fast):
        v = v.cpu().numpy()
        assert np.array_equal(np.isfinite(v), np.isfinite(exact[k])), (what, case, R, views, k)
        err = np.abs(np.where(np.isfinite(v), v - exact[k], 0.0))
        assert err.max() <= FAST_MAX[k], (what, case, R, views, k, float(err.max()))


@pytest.mark.parametrize("case", list(CASES))
def test_the_injected_jitter_puts_the_disorder_where_the_halves_meet(oracle, case):
    """What the launches below rely on, established on the oracle's own depths."""
    Sc = CASES[case][0]
    c = Sc // 2
    t = reference(case, 40)[1]["depths_coarse"]
    rev = np.diff(t, axis=1) < 0  # rev[r, i]: t[i + 1] < t[i]
    for r in CUT:  # (a) the only disorder is across the cut
        assert rev[r].nonzero()[0].tolist() == [c - 1], (r, rev[r].nonzero())
    for r in IN0:  # (b) ... inside half 0
        assert rev[r].nonzero()[0].tolist() == [2] and 3 < c, (r, rev[r].nonzero())
    for r in IN1:  # ... inside half 1
        assert rev[r].nonzero()[0].tolist() == [c + 1], (r, rev[r].nonzero())
    for r in EXTREMA:  # (c) the minimum in half 1, the maximum in half 0
        assert t[r].argmin() == c + 1 and t[r].argmax() == 1, (r, t[r].argmin(), t[r].argmax())
    touched = set(CUT + IN0 + IN1 + EXTREMA)
    quiet = [r for r in range(40) if r not in touched]
    assert not rev[quiet].any() and len(quiet) > 20  # (d) most rays stay sorted, in both tiles
    assert all(any(lo <= r < lo + 32 for r in touched) and any(lo <= r < lo + 32 for r in quiet) for lo in (0, 32))
    # the clamp range of the call comes from injected extrema: its minimum from half 1, its maximum from half 0
    tmm = reference(case, 40)[1]["tminmax"]
    rmin, imin = np.unravel_index(t.argmin(), t.shape)
    rmax, imax = np.unravel_index(t.argmax(), t.shape)
    assert (rmin in EXTREMA and imin == c + 1 and tmm[0] == t.min()) and (rmax in EXTREMA and imax == 1 and tmm[1] == t.max())
    w = reference(case, 40)[0]["wsum"]
    assert (w == 0).any() and (w > 0.5).any()  # surfaces and empty rays


@pytest.mark.parametrize("R", [40, 64])
@pytest.mark.parametrize("case", list(CASES))
def test_draw_rows_match_the_oracle(hip, oracle, stop_at_a_device_fault, case, R):
    sc = scene(case, R)
    args = launch_args(hip, sc)
    assert args[3].data_ptr() % 16 == 0 and args[4].data_ptr() % 16 == 0
    check_all_kernels(hip, case, R, 1, args, "aligned")


@pytest.mark.parametrize("case,R", [("S48", 40), ("S96_no_column", 64)])
def test_two_views_in_one_launch(hip, oracle, stop_at_a_device_fault, case, R):
    """The second view's rows start R * Sc (R * Sf) floats into the tensors."""
    sc = scene(case, R, 2)
    check_all_kernels(hip, case, R, 2, launch_args(hip, sc), "two views")


@pytest.mark.parametrize("case,which", [("S48", "both"), ("S96_no_column", "both"), ("S48", "jitter")])
def test_rows_that_are_not_16_byte_aligned_take_the_scalar_loads(hip, oracle, stop_at_a_device_fault, case, which):
    """jitter and u (or jitter alone, u as pieces) one float into a larger buffer: the same bits."""
    sc = scene(case, 40)
    jit = off_by_one_float(sc["jit"])
    u = off_by_one_float(sc["u"]) if which == "both" else dev(sc["u"])
    assert jit.data_ptr() % 16 == 4 and u.data_ptr() % 16 == (4 if which == "both" else 0)
    check_all_kernels(hip, case, 40, 1, launch_args(hip, sc, jit, u), "misaligned " + which)
