"""GPU: the final walk of k_render with its two bit-row words and the previous sample's position kept in registers (csrc/p3d_kernels.hip,
the EARLY branch of the final loop), bit for bit against the CPU oracle.

The walk goes back to LDS for a word of the rows "merged sample q is known to carry sigma = -1000" / "... comes from the coarse list"
only when its position m enters the next 32-bit word: at the end of a jump over a run of known samples that reaches bit 31, and behind a
decoded sample that sat on bit 31.  The shapes are the smallest at which a stale or wrongly shifted word shows:

  rays     R = 40 (the second 32-ray tile is partial: lanes finished from step 0 on) and R = 64 as an 8-wide image
  lengths  S = Sc + Sf = 33 (the last sample alone in word 1), 64 (ends on a boundary), 96 (48+48, the production instantiation),
           96 as 40+56 (the padded 64-key path), 192 (96+96: without the small-launch kernels the plan takes the 96-key kernel that
           keeps no coarse depths in LDS)
  runs     triplane_crop at two values per length, picked so that (asserted below, on the oracle's own depths) some ray's leading run of
           known samples is longer than a word and stops inside a later one, some ray's run ends exactly on bit 31 of a word with a
           sample to decode behind it, and some ray is known from end to end; between the two values the ends of the runs move
  guard    binarize_clouds: a solid sample (sigma = 1000 > 602) blocks the jump behind it, the known samples that follow are consumed
           one per step, and the colour guard decodes them after all where the interval's weight is not zero

Every case runs on the 32-rays-per-wave kernel and on both small-launch kernels (whose walk is their own, and whose colour guard is the
shared one), with the early-outs and without them (P3D_FLAG_NO_EARLY_OUT: the same bits), and in tolerance mode against the exact one.
"""
import functools

import numpy as np
import pytest
import torch

import p3d_testing as T
from test_hip_parity import FAST_MAX  # the ONE definition of the tolerance mode's bound

pytestmark = pytest.mark.gpu  # (every test of the file: the fault check below runs behind each of them)

OUTPUTS = ("feat", "depth", "wsum", "xyz")
CASES = {"S33": (20, 13), "S64": (32, 32), "S96": (48, 48), "S96_padded": (40, 56), "S192": (96, 96)}
# triplane_crop, two values per length (the box is 0.7 wide: a crop of c leaves |x|, |z| <= 0.35 - c)
CROPS = {"S33": (0.15, 0.29), "S64": (0.16, 0.245), "S96": (0.16, 0.235), "S96_padded": (0.155, 0.26), "S192": (0.16, 0.26)}
RES = 8  # the image is 8 rays wide; R = 40 is its first five rows
BINARIZE = 0.4


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


def options(case):
    Sc, Sf = CASES[case]
    return dict(T.RENDERING_KWARGS, depth_resolution=Sc, depth_resolution_importance=Sf)


def masks(case, which):
    return dict(triplane_crop=CROPS[case][which], binarize_clouds=BINARIZE, force_sigmoid=True)


@functools.lru_cache(maxsize=None)
def scene(case, R):
    import panic3d_amd as P
    from oracle import oracle
    Sc, Sf = CASES[case]
    planes = T.make_planes(9301, 1, 64, 64, scale=4.0, smooth=8)
    mlp = oracle.prescale_mlp(*T.make_decoder_params(9302, 1.0, 30.0))
    o, d = P.cameras.rays_from_label(P.cameras.camera_label(15.0, 25.0, 1.0, 30.0)[None], RES)
    o, d = (np.ascontiguousarray(x.numpy()[:, :R]) for x in (o, d))
    jit, u = T.make_random_draws(9303, 1, R, Sc, Sf)
    sc = dict(planes=planes, mlp=mlp, o=o, d=d, jit=jit, u=u)
    for a in (planes, o, d, jit, u) + tuple(mlp):
        a.setflags(write=False)
    return sc


@functools.lru_cache(maxsize=None)
def reference(case, which, R):
    """the oracle's four outputs and, from its dumps, the length of every ray's leading run of known samples"""
    from oracle import oracle
    sc = scene(case, R)
    Sc, Sf = CASES[case]
    oo = oracle.make_opts(options(case), **masks(case, which))
    *ref, dm = oracle.render(sc["planes"], sc["o"], sc["d"], sc["jit"], sc["u"], sc["mlp"], oo, dumps=True)
    for a in ref:
        a.setflags(write=False)
    # merged sample q of a ray is entry perm[q] of [coarse | fine]; the kernel knows sigma = -1000 without a decode where the position is
    # cropped (binary32, no contraction: the kernel's own expression) and, for a coarse sample, where the coarse pass decoded a masked one
    # (in front of the first unknown sample the ray's transmittance is still 1: no dead-ray exception in a LEADING run)
    perm = dm["perm"].astype(np.int64)
    t = np.take_along_axis(np.concatenate([dm["depths_coarse"], dm["depths_fine"]], 1), perm, 1)
    assert (np.diff(t, axis=1) >= 0).all()
    ox, oz, dx, dz = (sc[k][0, :, i:i + 1] for k in "od" for i in (0, 2))
    lim = np.float32(oo.crop_limit)
    cropped = (np.abs(ox + t * dx) > lim) | (np.abs(oz + t * dz) > lim)
    masked_c = np.concatenate([dm["sigma_coarse"] == -1000.0, np.zeros((R, Sf), bool)], 1)
    known = cropped | np.take_along_axis(masked_c, perm, 1)
    lead = np.where(known.all(1), Sc + Sf, np.argmin(known, 1))
    return dict(zip(OUTPUTS, ref)), lead


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("case", list(CASES))
def test_the_crops_put_the_runs_where_the_words_end(oracle, case):
    """What the launches below rely on, established on the oracle's own depths."""
    S = sum(CASES[case])
    leads = [reference(case, which, 64)[1] for which in (0, 1)]
    both = np.concatenate(leads)
    print(case, "leading runs of known samples:", [sorted(set(x.tolist())) for x in leads])
    if S > 33:  # (with 33 samples a run longer than a word is the whole ray, and the runs that stop earlier are shorter than a word)
        assert ((both > 32) & (both < S) & (both % 32 != 0)).any(), "no run longer than a word that stops inside a later word"
        assert ((both % 32 == 0) & (both > 0) & (both < S)).any(), "no run that ends exactly on bit 31 with a sample to decode behind it"
    assert (both == S).any() and (both < S).any(), "no ray known from end to end, or none with a sample to decode"
    assert (leads[0] != leads[1]).any(), "the two crops leave every run where it was"
    for which in (0, 1):  # the scene has surfaces (solid samples: the blocked jump and the guard) and rays that stay empty
        w = reference(case, which, 64)[0]["wsum"]
        assert (w == 0).any() and (w > 0.5).any()


@pytest.mark.parametrize("R", [40, 64])
@pytest.mark.parametrize("which", [0, 1], ids=["crop_a", "crop_b"])
@pytest.mark.parametrize("case", list(CASES))
def test_walk_matches_the_oracle(hip, oracle, stop_at_a_device_fault, case, which, R):
    sc = scene(case, R)
    ref, _ = reference(case, which, R)
    pl, o, d, jit, u = (hip.ops.planes_to_nhwc(dev(sc["planes"])), dev(sc["o"]), dev(sc["d"]), dev(sc["jit"]), dev(sc["u"]))
    mlp = tuple(dev(x) for x in sc["mlp"])
    tile_w = RES if R == RES * RES else 0
    exact = None
    for small in (False, "pair", "quad"):
        for early in (True, False):
            st = {}
            opts = hip.ops.make_opts(options(case), early_out=early, small_launch_kernel=small, **masks(case, which))
            out = hip.ops.render(pl, o, d, jit, u, mlp, opts, ray_tile_w=tile_w, stats=st)
            torch.cuda.synchronize()
            assert st["small_launch_kind"] == (small or None), st
            got = {k: v.cpu().numpy() for k, v in zip(OUTPUTS, out)}
            for k in OUTPUTS:
                assert same(got[k], ref[k]), (case, which, R, small, early, k, int((got[k] != ref[k]).sum()))
            if early and small is False:
                exact = got
                assert st["decode_steps"] < st["decode_steps_full"], st  # the early-outs did run
        fast = hip.ops.render(pl, o, d, jit, u, mlp, hip.ops.make_opts(options(case), small_launch_kernel=small, fast_color=True, **masks(case, which)),
                              ray_tile_w=tile_w)
        torch.cuda.synchronize()
        for k, v in zip(OUTPUTS, fast):
            v = v.cpu().numpy()
            assert np.array_equal(np.isfinite(v), np.isfinite(exact[k])), (case, which, R, small, k)
            err = np.abs(np.where(np.isfinite(v), v - exact[k], 0.0))
            assert err.max() <= FAST_MAX[k], (case, which, R, small, k, float(err.max()))
