"""GPU: the fused renderer in the exact mode and in the tolerance mode (P3D_FLAG_FAST_COLOR) on every plan, against the CPU oracle, at
the cases of tests/render_mode_cases.py: ragged ray lists, screen tiles that are no power of two per row, N = 2 / 3, per-ray limits
and disparity spacing, every mask mode, both backgrounds and plane conventions, dump and weights-only launches, a swizzled grid
with an identity tail, four-wave workgroups whose last waves have no tile, and the blocked tile order over two views.

Gate (render_mode_cases.gate): the exact mode equals the oracle bit for bit; the tolerance mode has the oracle's non-finite pattern
and stays within FAST_MAX (test_hip_parity.py) of it on EVERY ray of every output.  Each test also asserts, through the launch's
`stats` and ops.render_plan_info, that the launch is the one the case names (tests/test_render_mode_cases_cpu.py holds the plan to
the same figures, and to the instantiation).

Measured on an MI355X (`pytest -s` prints them), worst |error| / bound: feat 0.286 and wsum 0.158 (blocked_tall-4p4-wave32-early-fixed-o0),
depth 0.280 (tail-12p7-wave32-all-fixed-o2), xyz 0.429 (tiles-96p96-pair-early-disparity-o2); DESIGN.md §4.5.
The case tail-12p7-wave32-early-fixed-o1 is the one that holds k_render<..., EARLY> to "a ray that has taken its last sample is done": its
rays end on a solid sample (binarize_clouds, sigma 1000) with the transmittance still above the cut.
Oracle time on the CPU for the large shapes at 4+4: wide4 0.9 s, blocked 0.7 s, blocked_tall 0.7 s — far below the ten seconds at which the
rate would have been lowered to 4+0, so the oracle comparison and the kernel-to-kernel comparison share the 4+4 launch.
"""
import functools

import numpy as np
import pytest
import torch

import render_mode_cases as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import panic3d_amd
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    panic3d_amd._lib.lib()  # must load: no fallback
    return panic3d_amd


@pytest.fixture(scope="module")
def worst():
    """the largest |error| / bound per output over the tolerance-mode renders of this module, printed at the end"""
    w = {}
    yield w
    for k in M.OUTPUTS:
        if k in w:
            print(f"\nWORST tolerance-mode {k}: err / bound = {w[k][0]:.3f} ({w[k][1]})", end="")
    print()


@pytest.fixture(autouse=True)
def stop_at_a_device_fault():
    """A device fault ends the session: nothing more is launched on a GPU that has faulted."""
    yield
    try:
        torch.cuda.synchronize()
    except Exception as e:  # noqa: BLE001
        pytest.exit(f"device fault: {e}", returncode=3)


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _scene_on_device(shape):
    import panic3d_amd as P
    sc = M.scene(shape)
    w0, b0, w1, b1 = (dev(x) for x in sc["raw"])
    mlp = P.ops.prescale_mlp(w0, b0, w1, b1, 1 / np.sqrt(32), 1.0, 1 / np.sqrt(64), 1.0)
    return dict(nhwc=P.ops.planes_to_nhwc(dev(sc["planes"])), o=dev(sc["o"]), d=dev(sc["d"]), mlp=mlp)


def _np(t):
    return None if t is None else t.cpu().numpy()


def launch(hip, case, fast, dumps=False, weights_only=False, rays=None, small=None):
    """One render of the case (rays: (view, first ray, ray count) renders that run of one view alone); asserts that the launch is the
    one the case names.  Returns (dict of numpy outputs [+ dumps], stats)."""
    inp, D = M.inputs(case), _scene_on_device(case["shape"])
    N, R = inp["o"].shape[:2]
    c = dict(case, small=case["small"] if small is None else small)
    opts = M.hip_opts(hip.ops, c, fast)
    nhwc, o, d, jit, u, lim = D["nhwc"], D["o"], D["d"], dev(inp["jit"]), dev(inp["u"]), inp["limits"]
    lim = None if lim is None else tuple(dev(x) for x in lim)
    if rays is not None:
        n, r0, cnt = rays
        nhwc, o, d, jit = nhwc[n:n + 1].contiguous(), o[n:n + 1, r0:r0 + cnt].contiguous(), d[n:n + 1, r0:r0 + cnt].contiguous(), jit[n:n + 1, r0:r0 + cnt].contiguous()
        u = None if u is None else u[n * R + r0:n * R + r0 + cnt].contiguous()
        assert lim is None
        N, R = 1, cnt
    st = {}
    out = hip.ops.render(nhwc, o, d, None if case["rng"] else jit, None if case["rng"] else u, D["mlp"], opts, ray_tile_w=case["tile_w"],
                         dumps=dumps, stats=st, per_view_clamp=case["per_view"], ray_limits=lim, rng_seed=inp["rng_seed"],
                         weights_only=weights_only)
    torch.cuda.synchronize()
    got = dict(zip(M.OUTPUTS, (_np(t) for t in out[:4])))
    if dumps:
        got["dumps"] = {k: v.cpu().numpy() for k, v in out[4].items()}
    if rays is None:  # the launch is the one the case names
        want = M.expected_launch(dict(c, kind="dump" if dumps else "wo" if weights_only else "render"), fast)
        popts = hip.ops._with_flag(opts, hip._lib.P3D_FLAG_WEIGHTS_ONLY) if weights_only else opts
        info = hip.ops.render_plan_info(N, R, case["tile_w"], popts, bool(dumps), lim is not None)
        assert tuple(info[:5]) == (want["slots"], want["ntiles"], want["steps_full"], want["grid"], want["block"]), (case["id"], fast, info)
        assert st["tiles"] == want["ntiles"] and st["decode_steps_full"] == want["steps_full"], (case["id"], st)
        assert st["small_launch_kind"] == {1: None, 2: "pair", 4: "quad"}[want["slots"]], (case["id"], st)
        if not dumps:  # (a dump launch keeps no count)
            assert 0 < st["decode_steps"] <= st["decode_steps_full"], (case["id"], st)
            if not case["early"]:
                assert st["decode_steps"] == st["decode_steps_full"], (case["id"], st)
    return got, st


def report(worst, label, got, ref):
    err = M.errors(got, ref)
    print(f"{label}: " + "  ".join(f"{k} {err[k]:.2e} = {err[k] / M.FAST_MAX[k]:.3f} x bound" for k in err))
    for k, e in err.items():
        if e / M.FAST_MAX[k] > worst.get(k, (-1.0, ""))[0]:
            worst[k] = (e / M.FAST_MAX[k], label)


def check_both_modes(hip, worst, case):
    ref = M.reference(case)
    exact, _ = launch(hip, case, fast=False)
    assert M.gate(exact, ref, exact=True) == [], case["id"]
    fast, _ = launch(hip, case, fast=True)
    same = all(np.array_equal(fast[k], exact[k], equal_nan=True) for k in M.OUTPUTS)
    if case["Sf"] == 0:  # a single pass is the reference's coarse pass: it stays exact
        assert same, case["id"]
    else:
        report(worst, case["id"], fast, ref)
        assert M.gate(fast, ref, exact=False) == [], case["id"]
        assert not same or float(ref["wsum"].max()) == 0.0, case["id"]  # it really is the other decoder
    return exact


@pytest.mark.parametrize("cid", M.ids(lambda c: c["kind"] == "render" and c["shape"] in ("list", "tiles", "tail")))
def test_case_in_both_modes(hip, worst, cid):
    check_both_modes(hip, worst, M.CASE[cid])


@pytest.mark.parametrize("cid", M.ids(lambda c: c["kind"] == "dump"))
@pytest.mark.parametrize("fast", [False, True])
def test_dump_launch(hip, worst, cid, fast):
    """In both modes everything the importance resampling produces is the oracle's, bit for bit; the four outputs pass the gate."""
    case = M.CASE[cid]
    ref = M.reference(case, dumps=True)
    got, _ = launch(hip, case, fast, dumps=True)
    od, hd = ref["dumps"], got["dumps"]
    for k in ("depths_coarse", "sigma_coarse", "weights_coarse", "inds", "depths_fine", "depths_sorted", "tminmax") + (() if fast else ("sigma_sorted",)):
        assert np.array_equal(hd[k].reshape(od[k].shape), od[k]), (cid, k)
    assert np.array_equal(hd["depth_unclamped"], od["depth_unclamped"], equal_nan=True) or fast
    if fast:
        report(worst, f"{cid} (tolerance)", got, ref)
    assert M.gate(got, ref, exact=not fast) == [], cid


@pytest.mark.parametrize("cid", M.ids(lambda c: c["kind"] == "wo"))
def test_weights_only_launch(hip, worst, cid):
    """k_render_slots<4, 48 | 96, true, true>: no colours, and the wsum / depth bits of the full tolerance-mode launch of the same kernel;
    the exact mode has no such kernel and ignores the hint."""
    case = M.CASE[cid]
    ref = M.reference(case)
    wo, _ = launch(hip, case, fast=True, weights_only=True)
    assert wo["feat"] is None and wo["xyz"] is None
    full, _ = launch(hip, case, fast=True)
    assert np.array_equal(wo["wsum"], full["wsum"]) and np.array_equal(wo["depth"], full["depth"], equal_nan=True), cid
    report(worst, f"{cid} (weights only)", wo, ref)
    assert M.gate(wo, ref, exact=False) == [] and M.gate(full, ref, exact=False) == [], cid
    exact, _ = launch(hip, case, fast=False, weights_only=True)
    assert exact["feat"] is None and M.gate(exact, ref, exact=True) == [], cid


@functools.lru_cache(maxsize=None)
def _sweep_config(seed):
    """The sweep's configuration as test_hip_parity._random_config makes it, and the oracle's render of it."""
    from oracle import oracle
    c = M._random_config(seed)
    ref = oracle.render(c["planes"], c["o"], c["d"], c["jit"], c["u"], oracle.prescale_mlp(*c["raw"], lr_mul=c["lr_mul"]),
                        oracle.make_opts(c["ro"], **c["kw"]))
    return c, dict(zip(M.OUTPUTS, ref))


@pytest.mark.parametrize("small", ["quad", "pair", False])
@pytest.mark.parametrize("seed", range(100, 124))
def test_random_configs_in_tolerance_mode(hip, worst, seed, small):
    """The randomised sweep of test_hip_parity.test_render_random_configs_bit_exact with fast_color=True, under the same gate."""
    c, ref = _sweep_config(seed)
    w0, b0, w1, b1 = (dev(x) for x in c["raw"])
    lr = c["lr_mul"]
    mlp = hip.ops.prescale_mlp(w0, b0, w1, b1, lr / np.sqrt(32), lr, lr / np.sqrt(64), lr)
    opts = hip.ops.make_opts(c["ro"], early_out=c["early_out"], small_launch_kernel=small, fast_color=True, **c["kw"])
    st = {}
    out = hip.ops.render(hip.ops.planes_to_nhwc(dev(c["planes"])), dev(c["o"]), dev(c["d"]), dev(c["jit"]), dev(c["u"]), mlp, opts,
                         ray_tile_w=c["tile_w"], stats=st)
    got = dict(zip(M.OUTPUTS, (_np(t) for t in out)))
    assert st["small_launch_kind"] == (small or None)
    Sf = c["ro"]["depth_resolution_importance"]
    if Sf > 0:
        report(worst, f"sweep seed {seed} {small} {c['ro']['depth_resolution']}+{Sf}", got, ref)
    assert M.gate(got, ref, exact=Sf == 0) == [], (seed, small)


@pytest.mark.parametrize("cid", M.ids(lambda c: c["shape"] in ("wide4", "blocked", "blocked_tall")))
def test_large_grid_in_both_modes_and_against_the_small_launch_kernels(hip, worst, cid):
    """Both modes against the oracle; and in the exact mode the same rays, rendered view by view in runs of at most 16384 rays
    through the small-launch kernels (8 rays x 4 samples and 16 x 2, alternating), give the same feat / wsum / xyz bits — kernel
    against kernel, no reference.  (depth is clamped to the range of the CALL: it is compared with the oracle only.)"""
    case = M.CASE[cid]
    exact = check_both_modes(hip, worst, case)
    s = M.SHAPES[case["shape"]]
    N, R = s["N"], s["R"]
    step = 16384  # 512 tiles of 32 rays: the largest small launch; 64 rows of 256 / 128 rows of 128 pixels: whole screen tiles
    kinds = set()
    for n in range(N):
        for i, r0 in enumerate(range(0, R, step)):
            small = ("quad", "pair")[(n + i) % 2]
            cnt = min(step, R - r0)
            part, st = launch(hip, case, fast=False, rays=(n, r0, cnt), small=small)
            assert st["small_launch_kind"] == small and st["tiles"] == (cnt // (32 // {"quad": 4, "pair": 2}[small]) if case["tile_w"]
                                                                       else -(-cnt // (32 // {"quad": 4, "pair": 2}[small])))
            kinds.add(small)
            for k in ("feat", "wsum", "xyz"):
                assert np.array_equal(part[k][0], exact[k][n, r0:r0 + cnt], equal_nan=True), (cid, k, n, r0)
    assert kinds == {"quad", "pair"}
