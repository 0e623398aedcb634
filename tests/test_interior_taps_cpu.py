"""CPU: the launch's interior-taps decision (p3d_render_interior_taps, csrc/p3d_render_plan.hpp).

k_render's interior gather set-up (csrc/p3d_decode.hpp) drops the range tests of the x and z axes because a decoded sample has
|p| <= crop_limit there, and the launch allows it only where the kernel's binary32 chain

    q = p * coord_scale;  ix = (q + 1) * half - 0.5          half = 0.5 * W, no contraction

puts floor(ix) >= 0 at p = -crop_limit and floor(ix) + 1 <= W - 1 at p = +crop_limit.  That the two ends bound every |p| <= crop_limit
is a monotonicity argument about the chain's operations (the header's comment); this test pins it to the arithmetic: a host program
compiled from the plan header alone (tests/interior_taps_host.cpp, contraction off) sweeps the chain over every float within 2^16
floats of -L and of +L and every 4096th bit pattern of [-L, L], and numpy's binary32 restates the same chain over the same windows.
A sweep, not a proof.

Geometries (box_warp, crop, W): the benchmark's; a crop of one texel; crops for which the se tap of +L is exactly the last texel
(the plan must accept) and exactly one past it (must refuse); the same at the nw tap of -L; other plane sizes; W != H; no crop flag;
the test switch; a non-positive scale.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from host_build import CSRC, ROOT

CROP, GENERIC = 1, 131072
# name: (box_warp, triplane_crop, H, W, flags, coord_scale override)
GEOMETRIES = {
    "bench": (0.7, 0.1, 256, 256, CROP, None),
    "one_texel_256": (0.7, 0.7 / 256, 256, 256, CROP, None),
    "one_texel_16": (0.7, 0.7 / 16, 16, 16, CROP, None),
    "tests_16": (0.7, 0.16, 16, 16, CROP, None),
    "se_is_last_texel": (0.7, 0.7 / 256 * 0.51, 256, 256, CROP, None),
    "se_is_one_past": (0.7, 0.7 / 256 * 0.49, 256, 256, CROP, None),
    "se_is_last_texel_64": (1.0, 1.0 / 64 * 0.51, 64, 64, CROP, None),
    "se_is_one_past_64": (1.0, 1.0 / 64 * 0.49, 64, 64, CROP, None),
    "no_crop_margin": (0.7, 0.0, 256, 256, CROP, None),
    "odd_plane": (0.9, 0.05, 37, 37, CROP, None),
    "wide": (0.7, 0.1, 256, 128, CROP, None),
    "tall": (0.7, 0.1, 128, 256, CROP, None),
    "no_crop_flag": (0.7, 0.1, 256, 256, 0, None),
    "test_switch": (0.7, 0.1, 256, 256, CROP | GENERIC, None),
    "negative_scale": (0.7, 0.1, 256, 256, CROP, -2.0 / 0.7),
    "zero_scale": (0.7, 0.1, 256, 256, CROP, 0.0),
}
f32 = np.float32


def opts_of(name):
    """coord_scale and crop_limit as ops.make_opts makes them"""
    bw, crop, H, W, flags, scale = GEOMETRIES[name]
    return f32(2.0 / bw if scale is None else scale), f32(bw / 2 - float(crop)), H, W, flags


def chain(p, scale, W):
    """the kernel's chain in numpy's binary32 (every operation rounded once)"""
    p = np.asarray(p, f32)
    q = p * f32(scale)
    return (q + f32(1.0)) * f32(0.5 * W) - f32(0.5)


def sweep_points(L):
    bl = int(np.asarray(L, f32).view(np.uint32))
    w = 1 << 16
    inner = max(bl - w, 0)
    near = np.arange(inner, bl + w + 1, dtype=np.int64).astype(np.uint32).view(f32)
    across = np.arange(0, inner, 4096, dtype=np.int64).astype(np.uint32).view(f32)
    pos = np.concatenate([across, near])
    p = np.concatenate([-pos[::-1], pos])
    return p[np.abs(p) <= L]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("interior_taps") / "interior_taps_host")
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++")
    if cxx is None:
        import panic3d_amd
        cxx = panic3d_amd._build._hipcc()
    # tests/host_build.py's command with contraction off, as the library's host code is compiled
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", "-I", CSRC,
                           os.path.join(ROOT, "tests", "interior_taps_host.cpp"), "-o", exe])
    args = []
    for name in GEOMETRIES:
        s, L, H, W, flags = opts_of(name)
        args += [float(s).hex(), float(L).hex(), str(H), str(W), str(flags)]
    out = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120, check=True).stdout.strip().split("\n")
    assert len(out) == len(GEOMETRIES)
    res = {}
    for name, line in zip(GEOMETRIES, out):
        f = line.split()
        res[name] = dict(accept=int(f[0]), lo_end=float.fromhex(f[1]) if "0x" in f[1] else float(f[1]),
                         hi_end=float.fromhex(f[2]) if "0x" in f[2] else float(f[2]),
                         lo=float.fromhex(f[3]) if "0x" in f[3] else float(f[3]), hi=float.fromhex(f[4]) if "0x" in f[4] else float(f[4]),
                         n=int(f[5]), bad=int(f[6]))
    return res


def test_the_plan_accepts_and_refuses_the_geometries_it_should(host):
    want = dict(bench=1, one_texel_256=1, one_texel_16=1, tests_16=1, se_is_last_texel=1, se_is_one_past=0, se_is_last_texel_64=1,
                se_is_one_past_64=0, no_crop_margin=0, odd_plane=1, wide=0, tall=0, no_crop_flag=0, test_switch=0, negative_scale=0,
                zero_scale=0)
    assert {k: v["accept"] for k, v in host.items()} == want
    # the edge cases are what their names say, by numpy's own evaluation of the chain at +L
    for name, se in (("se_is_last_texel", 255), ("se_is_one_past", 256), ("se_is_last_texel_64", 63), ("se_is_one_past_64", 64)):
        s, L, H, W, _ = opts_of(name)
        assert np.floor(chain(L, s, W)) + 1 == se and host[name]["hi_end"] + 1 == se, name
    # the benchmark's texel range: taps 36 .. 219 of 256
    assert (host["bench"]["lo_end"], host["bench"]["hi_end"] + 1) == (36.0, 219.0)


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_the_two_ends_bound_the_chain_over_the_sweep(host, name):
    s, L, H, W, flags = opts_of(name)
    r = host[name]
    # numpy's chain at the two ends is the host program's
    assert np.floor(chain(-L, s, W)) == r["lo_end"] and np.floor(chain(L, s, W)) == r["hi_end"]
    p = sweep_points(L)
    assert len(p) == r["n"] and len(p) > (1 << 17)  # the same windows on both sides
    ix = chain(p, s, W)
    fl = np.floor(ix)
    assert fl.min() == r["lo"] and fl.max() == r["hi"]
    if s > 0:  # the monotonicity the decision rests on, over the sweep
        assert r["bad"] == 0 and not (np.diff(ix) < 0).any()
        assert r["lo"] == r["lo_end"] and r["hi"] == r["hi_end"]
    if r["accept"]:
        assert W == H and flags & CROP and s > 0
        assert fl.min() >= 0 and fl.max() + 1 <= W - 1  # every tap of every swept point inside the plane


def test_the_library_answers_the_same_decision():
    """p3d_render_taps_info: the decision of the launch itself, which also needs a kernel that has the interior form."""
    import ctypes as C
    import panic3d_amd as P
    L = P._lib.lib()
    assert P._lib.P3D_FLAG_GENERIC_TAPS == GENERIC
    hdr = open(os.path.join(ROOT, "include", "panic3d_hip.h")).read()
    assert f"#define P3D_FLAG_GENERIC_TAPS {GENERIC} " in hdr
    big, small = (1, 256, 256, 512 * 512, 512), (1, 256, 256, 64 * 64, 64)

    def ask(shape, name, extra=0, dumps=0, **kw):
        s, lim, H, W, flags = opts_of(name)
        N, _, _, R, w = shape
        o = P._lib.Opts(coord_scale=s, crop_limit=lim, Sc=48, Sf=48, flags=flags | extra, **kw)
        return L.p3d_render_taps_info(N, H, W, R, w, C.byref(o), dumps, 0)
    assert ask(big, "bench") == 1 and ask(big, "bench", plane_mode=1) == 1
    assert ask(big, "test_switch") == 0 and ask(big, "no_crop_flag") == 0 and ask(big, "wide") == 0 and ask(big, "se_is_one_past") == 0
    assert ask(big, "bench", extra=P._lib.P3D_FLAG_NO_EARLY_OUT) == 0 and ask(big, "bench", dumps=1) == 0  # every sample decoded
    assert ask(small, "bench") == 0 and ask(small, "bench", extra=P._lib.P3D_FLAG_NO_PAIR) == 1  # the small-launch kernels: generic
    assert L.p3d_render_taps_info(1, 256, 256, 4096, 64, None, 0, 0) == -1 and ask((1, 0, 0, 0, 64), "bench") == -1
