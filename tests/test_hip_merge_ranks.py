"""GPU: the 48-key k_render with its merge pre-pass by rank search (csrc/p3d_importance.hpp: p3d_merge_bits_ranks on a coarse column
in LDS) against the CPU oracle and against the same launch with the serial merge (P3D_FLAG_SERIAL_MERGE).

The pre-pass leaves two bit rows per ray: which merged sample is coarse, and whose density is known without a decode.  A wrong
is-coarse bit changes the outputs; a MISSING known bit only costs a decode and a surplus one drops a sample, so every case checks

* the four outputs with the early-outs on and off: the exact mode equal to the oracle (np.array_equal), the tolerance mode within
  FAST_MAX (test_hip_parity.py) of it on every ray;
* the same bits, and the same `stats["decode_steps"]`, as the launch with the serial merge;
* exact mode: the dump kernel's `depths_sorted` / `sigma_sorted` against the oracle's stages.

Shape: 64 x 64 planes, 48+48 samples (the 48-key kernel), two views of 9 x 9 rays on shared planes as a ray list: 81 rays per view
are two full 32-ray tiles and a partial one.  All inputs are seeded on the CPU.  Cases: crop on / off, cull on / off, binarize; a view
whose rays are all cropped; `u` rows of all 0 and all just below 1 (the fine samples in front of / behind the coarse list); on every
case repeated `u` values on some rays and jitter that reverses neighbouring coarse depths on others (the insertion-sort fallback,
which forgets the coarse pass's known bits); and a `u` tensor whose base is not 16-byte aligned, so that the row is read by scalar
loads.  A crop by position gives the fine samples' crop bits as runs at the ends of the sorted column, so these launches take the
deposit from counts; the bit-by-bit deposit runs on the GPU in the 96-key kernel (tests/test_hip_importance_split.py) and both are
compared on arbitrary bits on the host (tests/test_merge_ranks_cpu.py)."""
import functools

import numpy as np
import pytest
import torch

import p3d_testing as T
from test_hip_parity import FAST_MAX  # the ONE definition of the tolerance mode's bound

pytestmark = pytest.mark.gpu

OUTPUTS = ("feat", "depth", "wsum", "xyz")
SC = SF = 48
VIEWS, RES = 2, 9
R = RES * RES
CROP, CULL = dict(triplane_crop=0.1), dict(cull_clouds=0.5)
CASES = {
    "crop_cull": dict(kw=dict(CROP, **CULL)),
    "cull": dict(kw=CULL),
    "crop": dict(kw=CROP),
    "binarize": dict(kw=dict(CROP, binarize_clouds=0.5)),
    "cropped_view": dict(kw=dict(CROP, **CULL), cropped_view=True),
    "u_zero": dict(kw=dict(CROP, **CULL), u="zero"),
    "u_one": dict(kw=dict(CROP, **CULL), u="one"),
    "unaligned_u": dict(kw=dict(CROP, **CULL), unaligned=True),
}


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


def options():
    return dict(T.RENDERING_KWARGS, depth_resolution=SC, depth_resolution_importance=SF)


@functools.lru_cache(maxsize=None)
def scene(name):
    """The inputs of a case and the oracle's outputs and stages on them (read-only, computed once)."""
    import panic3d_amd as P
    from oracle import oracle
    case = CASES[name]
    planes = T.make_planes(9601, 1, 64, 64, scale=4.0, smooth=8)  # ONE subject, shared by the views
    raw = T.make_decoder_params(9602, 1.0, 30.0)
    labels = torch.cat([P.cameras.camera_label(-20.0 + 35.0 * v, 15.0 + 10.0 * v, 1.0, 30.0)[None] for v in range(VIEWS)])
    o, d = (x.numpy().copy() for x in P.cameras.rays_from_label(labels, RES))  # [VIEWS, R, 3]
    if case.get("cropped_view"):  # view 1: rays along y whose x lies beyond the crop limit — every sample cropped
        limit = np.float32(T.RENDERING_KWARGS["box_warp"] / 2 - CROP["triplane_crop"])
        o[1] = np.stack([np.full(R, limit * np.float32(1.05), np.float32), np.full(R, -1.0, np.float32),
                         np.linspace(-0.2, 0.2, R, dtype=np.float32)], axis=1)
        d[1] = np.array([0.0, 1.0, 0.0], np.float32)
    jit, u = (a.copy() for a in T.make_random_draws(9603, VIEWS, R, SC, SF))
    rng = np.random.default_rng(9604)
    rays = rng.permutation(VIEWS * R)
    jr = jit.reshape(VIEWS * R, SC)
    for r in rays[:40]:  # reversed neighbours in the coarse row, also at its ends
        for i in rng.choice(SC - 1, size=int(rng.integers(1, 3)), replace=False):
            jr[r, i], jr[r, i + 1] = 1.5, 0.1
    jr[rays[0], 0], jr[rays[0], 1] = 1.5, 0.1
    jr[rays[1], SC - 2], jr[rays[1], SC - 1] = 1.5, 0.1
    for r in rays[20:80]:  # repeated values (some of them on rays with reversed neighbours)
        k = int(rng.integers(0, 3))
        if k == 0:
            u[r, ::3] = u[r, 0]
            u[r, 1::3] = u[r, 1]
        elif k == 1:
            u[r, :] = u[r, 0]
        else:
            u[r] = np.sort(u[r])[::-1]
    if case.get("u") == "zero":
        u[:] = 0.0
    elif case.get("u") == "one":
        u[:] = np.float32(1.0) - np.float32(2.0 ** -24)
    mlp = oracle.prescale_mlp(*raw)
    ref = oracle.render(np.concatenate([planes] * VIEWS), o, d, jit, u, mlp, oracle.make_opts(options(), force_sigmoid=True, **case["kw"]),
                        dumps=True)
    sc = dict(planes=planes, raw=raw, o=o, d=d, jit=jit, u=u, ref=dict(zip(OUTPUTS, ref[:4])), stages=ref[4])
    for a in (planes, o, d, jit, u) + tuple(raw) + tuple(ref[:4]):
        a.setflags(write=False)
    return sc


def dev(a):
    return torch.from_numpy(np.array(a, np.float32)).cuda()  # (a copy: the shared scenes are read-only)


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("fast", [False, True], ids=["exact", "tolerance"])
@pytest.mark.parametrize("name", list(CASES))
def test_rank_merge_is_the_serial_merge_and_the_oracle(hip, oracle, name, fast):
    case, sc = CASES[name], scene(name)
    ops, ref = hip.ops, sc["ref"]
    mlp = ops.prescale_mlp(*(dev(x) for x in sc["raw"]), 1 / np.sqrt(32), 1.0, 1 / np.sqrt(64), 1.0)
    if case.get("unaligned"):  # the same values one float off a 16-byte boundary: the launch must read the row by scalar loads
        buf = torch.zeros(sc["u"].size + 4, dtype=torch.float32, device="cuda")
        u = buf[1:1 + sc["u"].size].view(VIEWS * R, SF)
        u.copy_(dev(sc["u"]))
        assert u.data_ptr() % 16 == 4 and u.is_contiguous()
    else:
        u = dev(sc["u"])
        assert u.data_ptr() % 16 == 0
    args = (ops.planes_to_nhwc(dev(sc["planes"])), dev(sc["o"]), dev(sc["d"]), dev(sc["jit"]), u, mlp)
    kw = dict(small_launch_kernel=False, fast_color=fast, force_sigmoid=True, **case["kw"])
    opts = ops.make_opts(options(), **kw)
    runs = {}
    for which, o in (("ranks", opts), ("serial", ops._with_flag(opts, hip._lib.P3D_FLAG_SERIAL_MERGE)),
                     ("no_early_out", ops.make_opts(options(), early_out=False, **kw))):
        st = {}
        out = ops.render(*args, o, ray_tile_w=0, stats=st)
        torch.cuda.synchronize()
        assert st["small_launch_kernel"] is False
        runs[which] = (dict(zip(OUTPUTS, out)), st)
    print(name, "tolerance" if fast else "exact", {k: v[1]["decode_steps"] for k, v in runs.items()}, "of", runs["ranks"][1]["decode_steps_full"])
    for which in ("ranks", "no_early_out"):
        for k in OUTPUTS:
            got = runs[which][0][k].cpu().numpy()
            if fast:
                err = np.abs(got.astype(np.float64) - ref[k]).reshape(VIEWS * R, -1).max(axis=1)
                print(f"  {which} {k}: max |got - oracle| {err.max():.3g} (bound {FAST_MAX[k]:g})")
                assert np.isfinite(got).all() and err.max() <= FAST_MAX[k], (name, which, k, float(err.max()), int((err > FAST_MAX[k]).sum()))
            else:
                assert np.array_equal(got, ref[k]), (name, which, k, int((got != ref[k]).sum()))
    # the rank search against the serial merge: the same bits and the same decodes
    for k in OUTPUTS:
        assert same_bits(runs["ranks"][0][k], runs["serial"][0][k]), (name, k)
    st = runs["ranks"][1]
    assert st["decode_steps"] == runs["serial"][1]["decode_steps"], (name, st, runs["serial"][1])
    # (a step is skipped only where NONE of a tile's 32 rays has a sample to decode: certain with the crop, which empties the ends of
    # every ray, and not without it)
    assert st["decode_steps"] < st["decode_steps_full"] if "triplane_crop" in case["kw"] else st["decode_steps"] <= st["decode_steps_full"]
    if not fast:
        out = ops.render(*args, ops.make_opts(options(), **kw), ray_tile_w=0, dumps=("depths_sorted", "sigma_sorted"))
        torch.cuda.synchronize()
        for k, a in zip(OUTPUTS, out):
            assert np.array_equal(a.cpu().numpy(), ref[k]), (name, "dumps", k)
        rdm = sc["stages"]
        all_d = np.concatenate([rdm["depths_coarse"], rdm["depths_fine"]], axis=1)
        all_s = np.concatenate([rdm["sigma_coarse"], rdm["sigma_fine"]], axis=1)
        assert np.array_equal(out[4]["depths_sorted"].cpu().numpy(), np.take_along_axis(all_d, rdm["perm"], axis=1))
        assert np.array_equal(out[4]["sigma_sorted"].cpu().numpy(), np.take_along_axis(all_s, rdm["perm"], axis=1))


def test_the_inputs_are_what_the_cases_claim(oracle):
    """Reversed coarse neighbours, tied fine depths, the fine samples in front of / behind the coarse list, an all-cropped view."""
    st = scene("crop_cull")["stages"]
    assert int((np.diff(st["depths_coarse"], axis=1) < 0).any(axis=1).sum()) >= 30
    assert int((np.diff(np.sort(st["depths_fine"], axis=1), axis=1) == 0).any(axis=1).sum()) >= 30
    assert float(scene("crop_cull")["ref"]["wsum"].mean()) > 0.05
    z, o = scene("u_zero")["stages"], scene("u_one")["stages"]
    assert (z["depths_fine"].max(axis=1) <= np.sort(z["depths_coarse"], axis=1)[:, 2]).all()   # in front of all but the first coarse samples
    assert (o["depths_fine"].min(axis=1) >= np.sort(o["depths_coarse"], axis=1)[:, -3]).all()  # behind all but the last
    cv = scene("cropped_view")
    assert (cv["ref"]["wsum"][1] == 0).all() and (cv["ref"]["wsum"][0] > 0).any()
