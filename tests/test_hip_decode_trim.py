"""GPU: the exact decode's two instruction trims against the CPU oracle, bit for bit (compared as uint32; a NaN matches any NaN).

A. The clamps of softplus / sigmoid as one v_med3_f32 each (csrc/p3d_math.hpp, P3D_CLAMP_MED3).  The median is maxnum's value on every
   input that is no signalling NaN only if the hardware treats NaN, +-0 and subnormals the way the header says: this test establishes
   it on the decoder's own pre-activations, which is where the instruction runs (test 1).
B. The cull / binarize decision from raw sigma outside the band of csrc/p3d_cull_band.hpp, the full evaluation inside (p3d_apply_masks,
   csrc/p3d_decode.hpp): points whose sigma crosses the band in steps of a few floats (test 2), and whole launches of the three render
   kernels with every sample inside the band, just below it and just above it (test 3).
"""
import functools
import subprocess

import numpy as np
import pytest
import torch

import p3d_testing as T
from host_build import compile_host

pytestmark = pytest.mark.gpu

BOX = T.RENDERING_KWARGS["box_warp"]
F32 = np.float32


def bits(u):
    return np.array([u], np.uint32).view(np.float32)[0]


def nxt(x, n):
    """the float n floats above x (below for n < 0); x != 0"""
    u = np.array([x], np.float32).view(np.uint32)[0].astype(np.int64)
    return bits(np.uint32(u + (n if x > 0 else -n)))


SUB_MIN, SUB_MAX = bits(0x00000001), bits(0x007FFFFF)
QNAN_POS, QNAN_NEG = bits(0x7FC00000), bits(0xFFC00000)
# The values every clamp site must see.  -|x| meets the clamp's bound P3D_EXP_LO = -200 at x = +-200: those and their two neighbours.
SPECIALS = np.array([0.0, SUB_MIN, -SUB_MIN, SUB_MAX, -SUB_MAX, -200.0, nxt(F32(-200.0), 1), nxt(F32(-200.0), -1), 200.0, nxt(F32(200.0), 1),
                     nxt(F32(200.0), -1), 20.0, -20.0, 88.0, -88.0, 1e30, -1e30, np.inf, -np.inf, QNAN_POS, QNAN_NEG], np.float32)


def same_bits(got, ref):
    got, ref = np.ascontiguousarray(got, np.float32).reshape(-1), np.ascontiguousarray(ref, np.float32).reshape(-1)
    return (got.view(np.uint32) == ref.view(np.uint32)) | (np.isnan(got) & np.isnan(ref))


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


@pytest.fixture(scope="module")
def band(tmp_path_factory):
    """(s_lo, s_hi) of csrc/p3d_cull_band.hpp at the threshold 0.5, from a host program compiled from the header"""
    exe = compile_host(tmp_path_factory.mktemp("cull_band"), "cull_band_host.cpp")
    out = subprocess.run([exe, "0.5"], capture_output=True, text=True, timeout=60, check=True).stdout.split()
    return F32(float.fromhex(out[1])), F32(float.fromhex(out[2]))


# ---------------------------------------------------------------------------------------------------------------- 1. decode_features
# How each pre-activation is reached (or_decode_features: X = ((f0 + f1) + f2) / 3; pre[n] = b0[n] + sum_k w0[n][k] X[k] by fma, b0 first):
#   layer1  rows of all-(+0) features: X = +0, every product w0 * X is +0 (w0 > 0 and finite), so pre[n] = b0[n] + 0 = b0[n] exactly,
#           and b0 holds SPECIALS (NaN and +-inf included: they pass through the additions of +0).  b0 = -0 would come out as +0, so a
#           second half of the rows has all-(-0) features: X = -0, products -0, and -0 + -0 = -0: there the unit with b0 = -0 sees -0.
#           All weights of both layers are positive, so that the hidden values +inf (softplus(inf)) meet no zero weight: no 0 * inf.
#   layer2  b0 = -1e30 everywhere and +0 features: pre = -1e30, softplus = 0 + log1p(exp(-200)) = +0 exactly, so every hidden value is
#           +0 and o[j] = b1[j] + sum_n w1[j][n] * 0 = b1[j] exactly; b1[1:] holds SPECIALS.  The colour row of -0 has NEGATIVE weights:
#           its products are -0 and -0 + -0 = -0 (with positive ones it would reach the sigmoid as +0).
#   random  4096 rows of random features through a random decoder: the values of ordinary use.
def feature_cases():
    g = np.random.default_rng(8801)
    pos = lambda *s: g.uniform(0.05, 1.0, s).astype(np.float32)  # noqa: E731
    n = len(SPECIALS)
    zero_rows = np.zeros((1, 3, 64, 32), np.float32)
    zero_rows[:, :, 32:] = -0.0
    b0 = g.standard_normal(64).astype(np.float32)
    b0[:n], b0[n] = SPECIALS, -0.0
    b0[n + 1:2 * n + 1] = SPECIALS  # once more, in other accumulator registers
    layer1 = (pos(64, 32), b0, pos(33, 64), g.standard_normal(33).astype(np.float32))
    b1 = g.standard_normal(33).astype(np.float32)
    b1[1:n + 1], b1[n + 1] = SPECIALS, -0.0
    w1 = pos(33, 64)
    w1[n + 1] = -w1[n + 1]
    layer2 = (pos(64, 32), np.full(64, -1e30, np.float32), w1, b1)
    raw = T.make_decoder_params(8802)
    from oracle import oracle
    return {"layer1": (zero_rows, layer1), "layer2": (zero_rows[:, :, :32], layer2),
            "random": (g.standard_normal((1, 3, 4096, 32)).astype(np.float32) * 2, oracle.prescale_mlp(*raw))}


@pytest.mark.parametrize("force_sigmoid", [True, False])
def test_decode_features_at_the_clamps_edge_values(hip, oracle, force_sigmoid):
    n = len(SPECIALS)
    for name, (feats, mlp) in feature_cases().items():
        rs, rr = oracle.decode_features(feats, mlp, force_sigmoid=force_sigmoid)
        if name == "layer2" and force_sigmoid:  # the values do reach the sigmoid: its limits come out
            col = {float(v) if np.isfinite(v) else str(v): rr[0, 0, i] for i, v in enumerate(SPECIALS)}
            assert col["inf"] == 1.0 and col["-inf"] == 0.0 and abs(col[0.0] - 0.5) < 1e-6 and abs(col[20.0] - 1.0) < 1e-6
            assert 0.0 < col[-88.0] < 1e-37 and abs(rr[0, 0, n] - 0.5) < 1e-6  # (the last one: -0)
        gs, gr = hip.ops.decode_features(dev(feats), tuple(dev(x) for x in mlp), force_sigmoid=force_sigmoid)
        torch.cuda.synchronize()
        ok_s, ok_r = same_bits(gs.cpu().numpy(), rs), same_bits(gr.cpu().numpy(), rr).reshape(-1, 32)
        assert ok_s.all(), (name, "sigma", int((~ok_s).sum()), np.flatnonzero(~ok_s)[:8])
        assert ok_r.all(), (name, "rgb", int((~ok_r).sum()), np.argwhere(~ok_r)[:8])


# ---------------------------------------------------------------------------------------------------------------- 2. point decode
# 2 x 2 planes (the smallest that hold a ramp).  Channel 0 of the xy plane is 0 in its left column and 1 in its right one, every other
# channel of every plane a constant: between the two texel centres the bilinear sample of channel 0 is a ramp in x.  Hidden unit 0 reads
# only that channel, with gain 6e-3, and the sigma row reads only hidden unit 0 (weight 1): over the 4096 points, sigma = b1[0] +
# softplus(2e-3 * ramp) rises by about 1e-3, some 2.4e-7 = two to four floats a point, and b1[0] puts the crossing of 1 mid-way.
RAMP_M = 4096


@functools.lru_cache(maxsize=None)
def ramp_scene():
    g = np.random.default_rng(8803)
    planes = np.broadcast_to(g.standard_normal((1, 3, 32, 1, 1)).astype(np.float32), (1, 3, 32, 2, 2)).copy()
    planes[0, :, 0] = 0.0
    planes[0, 0, 0, :, 1] = 1.0
    w0, b0, w1, b1 = (x.copy() for x in oracle_mlp(8804))
    w0[0], w0[:, 0] = 0.0, 0.0
    w0[0, 0], b0[0] = 6e-3, 0.0
    w1[0] = 0.0
    w1[0, 0] = 1.0
    b1[0] = 1.0 - np.log(2.0) - 0.5e-3
    pts = np.zeros((1, RAMP_M, 3), np.float32)
    half = 0.25 * BOX  # texel centres of a 2-wide plane: grid x = -+0.5, position -+box / 4
    pts[0, :, 0] = np.linspace(-half, half, RAMP_M, dtype=np.float64).astype(np.float32) * F32(0.999)
    pts[0, :, 1:] = g.uniform(-0.1, 0.1, (RAMP_M, 2)).astype(np.float32)
    for a in (planes, pts):
        a.setflags(write=False)
    return planes, (w0, b0, w1, b1), pts


def oracle_mlp(seed):
    from oracle import oracle
    return oracle.prescale_mlp(*T.make_decoder_params(seed))


@pytest.mark.parametrize("mask", ["cull_clouds", "binarize_clouds"])
def test_point_decode_across_the_band(hip, oracle, band, mask):
    planes, mlp, pts = ramp_scene()
    s_lo, s_hi = band
    raw, _ = oracle.decode(planes, pts, mlp, BOX, plane_mode=1, flags=oracle.FLAG_FORCE_SIGMOID)
    raw = raw.reshape(-1)
    inside = (raw >= s_lo) & (raw <= s_hi)
    below, above = (raw < s_lo) & (raw > s_lo - 1e-3), (raw > s_hi) & (raw < s_hi + 1e-3)
    steps = np.abs(np.diff(raw.view(np.uint32).astype(np.int64)))
    print("in the band %d, within 1e-3 below %d, above %d; steps of %d..%d floats, median %d" % (
        inside.sum(), below.sum(), above.sum(), steps.min(), steps.max(), np.median(steps)))
    assert inside.sum() >= 32 and below.sum() >= 32 and above.sum() >= 32 and np.median(steps) <= 8
    oo = oracle.make_opts(T.RENDERING_KWARGS, force_sigmoid=True, **{mask: 0.5})
    rs, rr = oracle.decode(planes, pts, mlp, BOX, plane_mode=1, flags=oo.flags, crop_limit=oo.crop_limit, cull_thresh=oo.cull_thresh)
    masked = rs.reshape(-1) == -1000.0
    assert masked[below].all() and not masked[above].any() and 0 < masked.sum() < RAMP_M
    opts = hip.ops.make_opts(T.RENDERING_KWARGS, force_sigmoid=True, **{mask: 0.5})
    pl = hip.ops.planes_to_nhwc(dev(planes))
    gs, gr = hip.ops.triplane_decode(pl, dev(pts), tuple(dev(x) for x in mlp), opts)
    torch.cuda.synchronize()
    ok_s, ok_r = same_bits(gs.cpu().numpy(), rs), same_bits(gr.cpu().numpy(), rr)
    assert ok_s.all(), (mask, int((~ok_s).sum()), np.flatnonzero(~ok_s)[:8], raw[~ok_s][:8])
    assert ok_r.all(), (mask, int((~ok_r).sum()))
    gd, _ = hip.ops.triplane_decode(pl, dev(pts[:, :1000]), tuple(dev(x) for x in mlp), opts, density_only=True)
    assert same_bits(gd.cpu().numpy(), rs[:, :1000]).all()


# ---------------------------------------------------------------------------------------------------------------- 3. the render kernels
# Constant planes and an all-zero sigma row: sigma = b1[0] + sum 0 * h = b1[0] exactly at every sample of every ray (outside the planes
# too, where the features are zero), so one launch holds every wave of the kernel on one side of the wave-uniform decision.
RENDER_SC, RENDER_SF = 12, 12
OUTPUTS = ("feat", "depth", "wsum", "xyz")


def render_options():
    return dict(T.RENDERING_KWARGS, depth_resolution=RENDER_SC, depth_resolution_importance=RENDER_SF)


@functools.lru_cache(maxsize=None)
def render_scene():
    import panic3d_amd as P
    g = np.random.default_rng(8805)
    planes = np.broadcast_to(g.standard_normal((1, 3, 32, 1, 1)).astype(np.float32), (1, 3, 32, 8, 8)).copy()
    o, d = P.cameras.rays_from_label(P.cameras.camera_label(10.0, 40.0, 1.0, 30.0)[None], 16)
    cut = lambda t: np.ascontiguousarray(t.reshape(1, 16, 16, 3)[:, 4:12].reshape(1, 128, 3).numpy())  # noqa: E731  16 x 8 rays
    w0, b0, w1, b1 = (x.copy() for x in oracle_mlp(8806))
    w1[0] = 0.0
    jit, u = T.make_random_draws(8807, 1, 128, RENDER_SC, RENDER_SF)
    return dict(planes=planes, o=cut(o), d=cut(d), mlp=(w0, b0, w1, b1), jit=jit, u=u)


def render_sigmas(s_lo, s_hi):
    return {"inside": F32(1.0), "below": nxt(s_lo, -4), "above": nxt(s_hi, 4)}


@functools.lru_cache(maxsize=None)
def render_reference(sigma):
    from oracle import oracle
    sc = render_scene()
    w0, b0, w1, b1 = sc["mlp"]
    b1 = b1.copy()
    b1[0] = sigma
    ref = oracle.render(sc["planes"], sc["o"], sc["d"], sc["jit"], sc["u"], (w0, b0, w1, b1),
                        oracle.make_opts(render_options(), force_sigmoid=True, cull_clouds=0.5))
    for a in ref[:4]:
        a.setflags(write=False)
    return b1, dict(zip(OUTPUTS, ref[:4]))


@pytest.mark.parametrize("early", [True, False], ids=["early", "all_samples"])
@pytest.mark.parametrize("small", [False, "pair", "quad"], ids=["k_render", "pair16", "quad8"])
def test_render_kernels_on_each_side_of_the_band(hip, oracle, band, small, early):
    sc = render_scene()
    s_lo, s_hi = band
    sig = render_sigmas(s_lo, s_hi)
    assert s_lo <= sig["inside"] <= s_hi and sig["below"] < s_lo and sig["above"] > s_hi
    pl, o, d, jit, u = (hip.ops.planes_to_nhwc(dev(sc["planes"])), dev(sc["o"]), dev(sc["d"]), dev(sc["jit"]), dev(sc["u"]))
    opts = hip.ops.make_opts(render_options(), early_out=early, small_launch_kernel=small, force_sigmoid=True, cull_clouds=0.5)
    for where in ("inside", "below", "above"):
        b1, ref = render_reference(float(sig[where]))
        if where == "below":
            assert float(ref["wsum"].max()) == 0.0  # every sample culled
        if where == "above":
            assert float(ref["wsum"].min()) > 0.0  # none
        w0, b0, w1, _ = sc["mlp"]
        st = {}
        out = hip.ops.render(pl, o, d, jit, u, tuple(dev(x) for x in (w0, b0, w1, b1)), opts, ray_tile_w=16, stats=st)
        torch.cuda.synchronize()
        assert st["small_launch_kind"] == (small or None), st
        for name, t in zip(OUTPUTS, out):
            ok = same_bits(t.cpu().numpy(), ref[name])
            assert ok.all(), (where, small, early, name, int((~ok).sum()))
