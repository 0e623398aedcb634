"""GPU: k_render with the per-ray importance work shared between the two halves of a wave (csrc/p3d_importance.hpp) against the
CPU oracle, BIT-EXACT (np.array_equal): the four outputs from the production kernels with the early-outs on and off, and the
stage dumps `inds`, `depths_fine`, `depths_sorted`, `sigma_sorted` from the dump kernel — on inputs that stress the split
together: 48+48 and 96+96 (the 96-key production kernel with and without its coarse-depth column: plain spacing, per-ray limits,
disparity spacing), a ray count that is no multiple of 32, several views on shared planes, `u` rows with repeated values and
values that sit exactly on cdf edges, and jitter that reverses neighbouring coarse depths.  All inputs are seeded on the CPU."""
import numpy as np
import pytest
import torch

import p3d_testing as T

pytestmark = pytest.mark.gpu

KW = dict(triplane_crop=0.1, cull_clouds=0.5, force_sigmoid=True)


@pytest.fixture(scope="module")
def hip():
    import panic3d_amd
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    panic3d_amd._lib.lib()  # must load: no fallback
    return panic3d_amd


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _cdf_rows(weights):
    """The kernel's cdf (include/p3d_numerics.h: renderer.py:328-370) restated on the oracle's coarse weights [NR, Sc - 1]:
    float32 terms, both sums sequential in binary64.  Rows [NR, Sc - 2]; cdf[0] = 0."""
    w = weights.astype(np.float32)
    m = np.maximum(w[:, :-1], w[:, 1:])
    v = ((m[:, :-1] + m[:, 1:]) * np.float32(0.5) + np.float32(0.01)) + np.float32(1e-5)
    fsum = np.cumsum(v.astype(np.float64), axis=1)[:, -1].astype(np.float32)
    pdf = (v / fsum[:, None]).astype(np.float32)
    cdf = np.cumsum(pdf.astype(np.float64), axis=1).astype(np.float32)
    return np.concatenate([np.zeros((w.shape[0], 1), np.float32), cdf], axis=1)


def _case(hip, oracle, Sc, Sf, branch, views, res, seed):
    """Inputs with every stress at once.  Returns (planes, o, d, jit, u, raw, ro, limits)."""
    ro = dict(T.RENDERING_KWARGS, depth_resolution=Sc, depth_resolution_importance=Sf)
    labels = torch.cat([hip.cameras.camera_label(-20.0 + 25.0 * v, 15.0 + 10.0 * v, 1.0, 30.0)[None] for v in range(views)])
    o, d = hip.cameras.rays_from_label(labels, res)  # [views, res * res, 3]: res odd -> the ray count is no multiple of 32
    limits = None
    if branch == "auto_limits":
        ro["ray_start"] = ro["ray_end"] = "auto"
        rs, re = hip.cameras.patch_ray_limits(*hip.cameras.ray_limits_box(o.cuda(), d.cuda(), ro["box_warp"]))
        limits = (rs.reshape(views, -1).cpu().numpy(), re.reshape(views, -1).cpu().numpy())
    elif branch == "disparity":
        ro["disparity_space_sampling"] = True
    planes = T.make_planes(seed, 1, 64, 64, scale=4.0, smooth=8)  # ONE subject: its planes are shared by all views
    raw = T.make_decoder_params(seed + 1, 1.0, 30.0)
    R = res * res
    jit, u = T.make_random_draws(seed + 2, views, R, Sc, Sf, auto_limits=branch == "auto_limits")
    jit, u = jit.copy(), u.copy()
    rng = np.random.default_rng(seed + 3)
    rays = rng.permutation(views * R)
    jr = jit.reshape(views * R, Sc)
    for r in rays[:80]:  # reversed neighbours in the coarse row, also at its ends
        for i in rng.choice(Sc - 1, size=int(rng.integers(1, 3)), replace=False):
            jr[r, i], jr[r, i + 1] = 1.5, 0.1
    o_np, d_np = o.numpy(), d.numpy()
    oo, om = oracle.make_opts(ro, **KW), oracle.prescale_mlp(*raw)
    pl = np.concatenate([planes] * views)
    first = oracle.render(pl, o_np, d_np, jit, u, om, oo, dumps=True, ray_limits=limits)[4]
    cdf = _cdf_rows(first["weights_coarse"])
    for r in rays[40:200]:  # (some of them rays with reversed neighbours)
        k = int(rng.integers(0, 4))
        if k == 0:    # repeated values: a third of the row is one value, the rest two others
            u[r, ::3] = u[r, 0]
            u[r, 1::3] = u[r, 1]
        elif k == 1:  # exactly on cdf edges, the first (0) and interior ones, some of them twice
            e = rng.choice(cdf.shape[1] - 1, size=Sf // 2, replace=True)
            u[r, rng.choice(Sf, size=Sf // 2, replace=False)] = cdf[r, e]
        elif k == 2:  # every draw the same
            u[r, :] = u[r, 0]
        else:         # descending row: the sorted order is the reverse of the draw order; the two halves' keys interleave
            u[r] = np.sort(u[r])[::-1]
    u = np.clip(u, 0.0, np.float32(1.0) - np.float32(2.0 ** -24)).astype(np.float32)
    return planes, o, d, jit, u, raw, ro, limits


CASES = [(48, 48, "plain", 1, 23), (48, 48, "auto_limits", 2, 15), (48, 48, "disparity", 1, 23), (96, 96, "plain", 2, 15),
         (96, 96, "auto_limits", 1, 23), (96, 96, "disparity", 1, 15)]


@pytest.mark.parametrize("Sc,Sf,branch,views,res", CASES)
def test_split_importance_bit_exact(hip, oracle, Sc, Sf, branch, views, res):
    planes, o, d, jit, u, raw, ro, limits = _case(hip, oracle, Sc, Sf, branch, views, res, 5000 + Sc + views)
    oo, om = oracle.make_opts(ro, **KW), oracle.prescale_mlp(*raw)
    ref = oracle.render(np.concatenate([planes] * views), o.numpy(), d.numpy(), jit, u, om, oo, dumps=True, ray_limits=limits)
    rdm = ref[4]
    w0, b0, w1, b1 = (dev(x) for x in raw)
    mlp = hip.ops.prescale_mlp(w0, b0, w1, b1, 1 / np.sqrt(32), 1.0, 1 / np.sqrt(64), 1.0)
    nhwc = hip.ops.planes_to_nhwc(dev(planes))  # [1, ...]: shared by the views
    lim = None if limits is None else tuple(dev(x) for x in limits)
    args = (nhwc, o.cuda(), d.cuda(), dev(jit), dev(u), mlp)
    outs = {}
    for early in (True, False):  # the production kernels: 32 rays per wave forced, a ragged ray list (no tiling)
        st = {}
        outs[early] = hip.ops.render(*args, hip.ops.make_opts(ro, small_launch_kernel=False, early_out=early, **KW), ray_tile_w=0,
                                     stats=st, ray_limits=lim)
        assert st["small_launch_kernel"] is False
        for name, a, b in zip(("feat", "depth", "wsum", "xyz"), outs[early], ref):
            assert np.array_equal(a.cpu().numpy(), b), (name, "early_out", early)
    for a, b in zip(outs[True], outs[False]):
        assert torch.equal(a, b)
    # the dump kernel: the stages behind the split
    out = hip.ops.render(*args, hip.ops.make_opts(ro, small_launch_kernel=False, **KW), ray_tile_w=0, dumps=True, ray_limits=lim)
    hdm = {k: v.cpu().numpy() for k, v in out[4].items()}
    for name, a, b in zip(("feat", "depth", "wsum", "xyz"), out, ref):
        assert np.array_equal(a.cpu().numpy(), b), (name, "dumps")
    assert np.array_equal(hdm["inds"], rdm["inds"])
    assert np.array_equal(hdm["depths_fine"], rdm["depths_fine"])
    all_d = np.concatenate([rdm["depths_coarse"], rdm["depths_fine"]], axis=1)
    all_s = np.concatenate([rdm["sigma_coarse"], rdm["sigma_fine"]], axis=1)
    assert np.array_equal(hdm["depths_sorted"], np.take_along_axis(all_d, rdm["perm"], axis=1))
    assert np.array_equal(hdm["sigma_sorted"], np.take_along_axis(all_s, rdm["perm"], axis=1))
    # the inputs are what they claim: surfaces, reversed coarse neighbours, fine depths that tie
    assert float(ref[2].mean()) > 0.05
    assert int((np.diff(rdm["depths_coarse"], axis=1) < 0).any(axis=1).sum()) >= 40
    assert int((np.diff(np.sort(rdm["depths_fine"], axis=1), axis=1) == 0).any(axis=1).sum()) >= 40
