"""GPU: the quad-cooperative gather of the render kernels (csrc/p3d_decode.hpp: the DPP-weighted fold, the two-stage quad transpose and
the once-per-decode colour widening) against the CPU oracle, bit for bit, at the smallest launches that reach each edge of a quad:

  tile     one 8 x 4 screen tile
  ragged   40 rays, untiled: the last 32-ray tile has 8 live lanes, so six of its quads hold no ray at all
  w12      12 x 4 rays: a width that is no multiple of the 8-wide tile
  leaving  a view whose rays leave the planes: at the edge some taps of a sample, and some samples of a quad, are out of bounds
  crop     a crop limit that cuts through the tile: live and suppressed lanes share a quad

each at 48+48, 96+96 and 16+40 samples (the 64-key instantiation, padded), on k_render and on k_render_slots forced to 16 rays x 2
samples (P3D_FLAG_PAIR16) and to 8 rays x 4 samples (P3D_FLAG_QUAD8), with the early-outs on and off and both values of force_sigmoid.
The oracle renders each (shape, rate, force_sigmoid) once.  (tests/test_quad_transpose_cpu.py proves the routing itself on the CPU.)
"""
import functools

import numpy as np
import pytest
import torch

import p3d_testing as T

pytestmark = pytest.mark.gpu

OUTPUTS = ("feat", "depth", "wsum", "xyz")
RATES = [(48, 48), (96, 96), (16, 40)]
BOX = T.RENDERING_KWARGS["box_warp"]
PLANE_H, PLANE_W = 40, 56
# shape -> camera (elevation, azimuth, fov) and image resolution; (x0, y0, w, h) of the rays cut from the image; ray_tile_w; masks; the
# decoder's seed — one whose density on all-zero features is masked (sigma < 1 under cull_clouds = 0.5), so that space outside the planes
# is empty and the outputs depend on the samples inside and at the edge (a decoder that is solid on zero features ends every ray at its
# first sample)
SHAPES = {
    "tile": dict(cam=(5.0, 30.0, 30.0), res=16, cut=(4, 6, 8, 4), tile_w=8, kw=dict(triplane_crop=0.1, cull_clouds=0.5), decoder=7104),
    "ragged": dict(cam=(10.0, 200.0, 30.0), res=16, cut=(3, 5, 10, 4), tile_w=0, kw=dict(triplane_crop=0.05, binarize_clouds=0.4), decoder=7104),
    "w12": dict(cam=(-15.0, 100.0, 30.0), res=16, cut=(2, 6, 12, 4), tile_w=12, kw=dict(cull_clouds=0.5), decoder=7101),
    # a wide camera, no crop mask: the rays at the rim of the image pass the planes' edges with their gathers live
    "leaving": dict(cam=(20.0, 35.0, 50.0), res=16, cut=(8, 6, 8, 4), tile_w=0, kw=dict(cull_clouds=0.5), decoder=7101),
    # crop limit 0.35 - 0.2 = 0.15: the right half of the image crosses it inside the tile
    "crop": dict(cam=(0.0, 0.0, 30.0), res=16, cut=(8, 6, 8, 4), tile_w=8, kw=dict(triplane_crop=0.2, cull_clouds=0.5), decoder=7104),
}


@functools.lru_cache(maxsize=None)
def scene(shape):
    import panic3d_amd as P
    s = SHAPES[shape]
    seed = 7100 + sorted(SHAPES).index(shape)
    elev, azim, fov = s["cam"]
    o, d = P.cameras.rays_from_label(P.cameras.camera_label(elev, azim, 1.0, fov)[None], s["res"])
    x0, y0, w, h = s["cut"]
    cut = lambda t: np.ascontiguousarray(t.reshape(1, s["res"], s["res"], 3)[:, y0:y0 + h, x0:x0 + w].reshape(1, w * h, 3).numpy())  # noqa: E731
    return dict(planes=T.make_planes(seed, 1, PLANE_H, PLANE_W, scale=4.0, smooth=8), raw=T.make_decoder_params(s["decoder"], 1.0, 30.0),
                o=cut(o), d=cut(d), seed=seed)


def options(shape, Sc, Sf):
    return dict(T.RENDERING_KWARGS, depth_resolution=Sc, depth_resolution_importance=Sf)


@functools.lru_cache(maxsize=None)
def draws(shape, Sc, Sf):
    sc = scene(shape)
    return T.make_random_draws(sc["seed"] + 2, 1, sc["o"].shape[1], Sc, Sf)


@functools.lru_cache(maxsize=None)
def reference(shape, Sc, Sf, force_sigmoid):
    from oracle import oracle
    sc = scene(shape)
    jit, u = draws(shape, Sc, Sf)
    ref = oracle.render(sc["planes"], sc["o"], sc["d"], jit, u, oracle.prescale_mlp(*sc["raw"]),
                        oracle.make_opts(options(shape, Sc, Sf), force_sigmoid=force_sigmoid, **SHAPES[shape]["kw"]))
    for a in ref[:4]:
        a.setflags(write=False)
    return dict(zip(OUTPUTS, ref[:4]))


def coarse_positions(shape, Sc=48):
    """sample positions [R][Sc][3] at the unjittered coarse depths"""
    sc = scene(shape)
    t = np.linspace(T.RENDERING_KWARGS["ray_start"], T.RENDERING_KWARGS["ray_end"], Sc, dtype=np.float32)
    return sc["o"][0][:, None, :] + t[None, :, None] * sc["d"][0][:, None, :]


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
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def on_device(shape):
    import panic3d_amd as P
    sc = scene(shape)
    mlp = P.ops.prescale_mlp(*(dev(x) for x in sc["raw"]), 1 / np.sqrt(32), 1.0, 1 / np.sqrt(64), 1.0)
    return dict(nhwc=P.ops.planes_to_nhwc(dev(sc["planes"])), o=dev(sc["o"]), d=dev(sc["d"]), mlp=mlp)


def test_the_shapes_are_what_they_say():
    """ragged: 40 rays; leaving / crop: inside one group of four consecutive rays, at one coarse depth, the property the case names."""
    assert [scene(s)["o"].shape[1] for s in ("tile", "ragged", "w12", "leaving", "crop")] == [32, 40, 48, 32, 32]
    assert 40 % 32 == 8
    # leaving: plane 0 samples (x, y) -> texel coordinates (grid_sample, align_corners=False); a sample is partly outside when its 2 x 2
    # taps straddle the border: ix in (-1, 0) or (W - 1, W) (likewise iy), wholly outside beyond
    p = coarse_positions("leaving") * (2.0 / BOX)
    ix, iy = (p[..., 0] + 1) * PLANE_W / 2 - 0.5, (p[..., 1] + 1) * PLANE_H / 2 - 0.5
    inside = (ix > -1) & (ix < PLANE_W) & (iy > -1) & (iy < PLANE_H)
    whole = (ix >= 0) & (ix <= PLANE_W - 1) & (iy >= 0) & (iy <= PLANE_H - 1)
    partly = inside & ~whole
    q = lambda m: m.reshape(-1, 4, m.shape[-1])  # noqa: E731  [group of four rays][ray][depth]
    assert (q(partly).any(1) & q(whole).any(1)).any(), "no quad with a partly-outside and a wholly-inside sample"
    assert (q(~inside).any(1) & q(inside).any(1)).any(), "no quad with an outside and an inside sample"
    # crop: |x| or |z| beyond the limit suppresses a lane
    p = coarse_positions("crop")
    lim = BOX / 2 - SHAPES["crop"]["kw"]["triplane_crop"]
    cropped = (np.abs(p[..., 0]) > lim) | (np.abs(p[..., 2]) > lim)
    assert (q(cropped).any(1) & q(~cropped).any(1)).any(), "no quad with a cropped and a live sample"


@pytest.mark.parametrize("small", [False, "pair", "quad"], ids=["k_render", "pair16", "quad8"])
@pytest.mark.parametrize("rate", RATES, ids=lambda r: f"{r[0]}p{r[1]}")
@pytest.mark.parametrize("shape", list(SHAPES))
def test_bit_exact_against_the_oracle(hip, shape, rate, small):
    Sc, Sf = rate
    D, s = on_device(shape), SHAPES[shape]
    jit, u = (dev(x) for x in draws(shape, Sc, Sf))
    for force_sigmoid in (True, False):
        ref = reference(shape, Sc, Sf, force_sigmoid)
        assert float(ref["wsum"].max()) > 0.0  # (something is rendered)
        for early in (True, False):
            opts = hip.ops.make_opts(options(shape, Sc, Sf), early_out=early, small_launch_kernel=small, force_sigmoid=force_sigmoid, **s["kw"])
            st = {}
            out = hip.ops.render(D["nhwc"], D["o"], D["d"], jit, u, D["mlp"], opts, ray_tile_w=s["tile_w"], stats=st)
            torch.cuda.synchronize()
            assert st["small_launch_kind"] == (small or None), st
            if not early:
                assert st["decode_steps"] == st["decode_steps_full"], st
            for name, t in zip(OUTPUTS, out):
                got = t.cpu().numpy().reshape(ref[name].shape)
                assert np.array_equal(got, ref[name], equal_nan=True), (shape, rate, small, force_sigmoid, early, name,
                                                                        int((got != ref[name]).reshape(got.shape[0] * got.shape[1], -1).any(-1).sum()))
