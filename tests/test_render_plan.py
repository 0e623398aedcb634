"""CPU: the host-side plan of a render launch (csrc/p3d_render_plan.hpp).  A host program compiled from the plan header alone, with
no device code, (1) reproduces the launches recorded from the renderer's launch code before the plan existed
(tests/golden/render_plans.json), (2) keeps its invariants over a sweep of shapes, sample counts, flags, dumps and per-ray limits,
and (3) follows the documented dispatch of the shapes that ship, below.  (4) The library's query p3d_render_plan_info answers the
same plans and error codes.  A GPU test checks that the launch the query names is the one that runs.

tests/golden/render_plans.json, one row per launch: N, R, ray_tile_w, Sc, Sf, flags, dumps, per-ray limits, then either the
P3D_E_* code or the instantiation, grid, block, dynamic LDS bytes, tile_w, tiles_x, tiles_per_img, ntiles, lds_rows, swz, blocked."""
import ctypes as C
import json
import os
import subprocess

import pytest

from host_build import ROOT, compile_host

FAST, NO_PAIR, PAIR16, QUAD8, WO, NO_EARLY, DISP = 512, 256, 16384, 32768, 65536, 32, 4096


def _rows():
    with open(os.path.join(ROOT, "tests", "golden", "render_plans.json")) as f:
        return json.load(f)


def _run(exe, lines):
    res = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-4000:]
    return res.stdout.splitlines()


def _parse(line):
    f = line.split()
    return [int(f[1])] if f[0] == "err" else [f[0]] + [int(x) for x in f[1:]]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return compile_host(tmp_path_factory.mktemp("render_plan"), "render_plan_host.cpp")


def test_plans_reproduce_the_recorded_launches(host):
    rows = _rows()
    assert len(rows) > 500 and {r[8] for r in rows if len(r) == 9} == {-1, -2}
    out = _run(host, ["p %d %d %d %d %d %d %d %d" % tuple(r[:8]) for r in rows])
    assert len(out) == len(rows)
    for r, o in zip(rows, out):
        assert _parse(o) == r[8:], r[:8]


def test_plans_keep_their_invariants_over_the_sweep(host):
    # per plan: dynamic LDS = the decoder image + the waves' rows, <= 160 KiB times the workgroups per CU it is packed for; grid x waves
    # covers ntiles (with no empty workgroup); ntiles x rays per tile >= N * R (screen tiles: exactly the image); the blocked order
    # only with whole 16 x 16-tile super-tiles and a multiple of 8 of them; no small-launch kernel with dumps or NO_PAIR; TCG only
    # for the plain stratified spacing (see render_plan_host.cpp)
    out = _run(host, ["v"])
    assert out[-1].startswith("v ") and int(out[-1].split()[1]) > 1000000


# The shapes that ship: (N, R, ray_tile_w, Sc, Sf, flags, dumps, per-ray limits) -> instantiation, grid, block, dynamic LDS bytes.
# k_render<NF, DUMP, FAST, EARLY, TCG>; k_render_slots<SLOTS, NF, FAST, WO>.
DISPATCH = {
    # bench.py: one 512^2 frame at 48+48, exact and tolerance: 2 x 4 waves per CU, blocked tile order
    "bench 512^2 48+48": ((1, 512 * 512, 512, 48, 48, 0, 0, 0), ("k_render<48,0,0,1,0>", 2048, 256, 70304)),
    "bench 512^2 48+48 tolerance": ((1, 512 * 512, 512, 48, 48, FAST, 0, 0), ("k_render<48,0,1,1,0>", 2048, 256, 78496)),
    # G.f's 128^2-ray views (tolerance mode, the package default): 8 rays x 4 samples per wave
    "view 128^2 48+48": ((1, 128 * 128, 128, 48, 48, FAST, 0, 0), ("k_render_slots<4,48,1,0>", 512, 256, 38560)),
    "view 128^2 96+96": ((1, 128 * 128, 128, 96, 96, FAST, 0, 0), ("k_render_slots<4,96,1,0>", 512, 256, 51744)),
    # paste_front's occlusion pass: the weights-only four-slot kernel
    "paste weights only 128^2 96+96": ((1, 128 * 128, 128, 96, 96, FAST | WO, 0, 0), ("k_render_slots<4,96,1,1>", 512, 256, 51744)),
    # 64^2 x 96+96 (<= 8192 rays): the four-slot kernel also in the exact mode
    "64^2 96+96": ((1, 64 * 64, 64, 96, 96, 0, 0, 0), ("k_render_slots<4,96,0,0>", 128, 256, 43552)),
    "64^2 96+96 tolerance": ((1, 64 * 64, 64, 96, 96, FAST, 0, 0), ("k_render_slots<4,96,1,0>", 128, 256, 51744)),
    # a dump launch: k_render with every sample decoded, one wave per workgroup at 512 tiles
    "dumps 128^2 48+48": ((1, 128 * 128, 128, 48, 48, 0, 1, 0), ("k_render<48,1,0,0,0>", 512, 64, 30368)),
    # per-ray limits at 96+96: the small launch is unchanged; the large one keeps the LDS-resident coarse depths (no TCG), 1 x 4 waves
    "limits 128^2 96+96": ((1, 128 * 128, 128, 96, 96, FAST, 0, 1), ("k_render_slots<4,96,1,0>", 512, 256, 51744)),
    "limits 512^2 96+96": ((1, 512 * 512, 512, 96, 96, FAST, 0, 1), ("k_render<96,0,1,1,0>", 2048, 256, 131232)),
    "512^2 96+96": ((1, 512 * 512, 512, 96, 96, FAST, 0, 0), ("k_render<96,0,1,1,1>", 2048, 256, 80544)),
}


def test_shipped_shapes_follow_the_dispatch_table(host):
    out = _run(host, ["p %d %d %d %d %d %d %d %d" % args for args, _ in DISPATCH.values()])
    got = {name: tuple(_parse(o)[:4]) for name, o in zip(DISPATCH, out)}
    assert got == {name: want for name, (_, want) in DISPATCH.items()}


@pytest.fixture(scope="module")
def L():
    import panic3d_amd
    panic3d_amd.build()
    return panic3d_amd._lib.lib()


def test_query_answers_the_plan_and_its_error_codes(L):
    from panic3d_amd._lib import Opts
    out = (C.c_int64 * 6)()
    for r in _rows():
        N, R, w, Sc, Sf, flags, d, l = r[:8]
        opts = Opts(Sc=Sc, Sf=Sf, flags=flags)
        rc = L.p3d_render_plan_info(N, R, w, C.byref(opts), d, l, out, 6)
        if len(r) == 9:
            assert rc == r[8], r[:8]
            continue
        assert rc == 0, r[:8]
        slots = 4 if r[8].startswith("k_render_slots<4") else 2 if r[8].startswith("k_render_slots<2") else 1
        steps = -(-Sc // slots) + (-(-(Sc + Sf) // slots) if Sf > 0 else 0)
        ntiles = r[15]
        assert list(out) == [slots, ntiles, ntiles * steps, r[9], r[10], r[11]], r[:8]
    opts = Opts(Sc=48, Sf=48)
    assert L.p3d_render_plan_info(1, 4096, 64, None, 0, 0, out, 6) == -1
    assert L.p3d_render_plan_info(1, 4096, 64, C.byref(opts), 0, 0, None, 6) == -1
    assert L.p3d_render_plan_info(1, 4096, 64, C.byref(opts), 0, 0, out, 5) == -1


@pytest.mark.gpu
@pytest.mark.parametrize("small", [False, "pair", "quad", True])
@pytest.mark.parametrize("fast", [False, True])
def test_launch_runs_what_the_query_names(small, fast):
    """Every sample decoded: the decode steps the kernel counts are the query's full count only if the launched kernel has the
    query's samples per wave-step and tiles."""
    import torch
    import p3d_testing as T
    import panic3d_amd as P
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    g = T.load_golden("render_32x32_16p16.npz")
    inp = T.golden_render_inputs(g)
    N, R = inp["rays_o"].shape[:2]
    side = int(round(R ** 0.5))
    opts = P.ops.make_opts(inp["ro"], early_out=False, small_launch_kernel=small, fast_color=fast, **inp["kw"])
    dev = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    w0, b0, w1, b1 = (dev(x) for x in inp["raw_mlp"])
    lr = inp["lr_mul"]
    mlp = P.ops.prescale_mlp(w0, b0, w1, b1, lr / 32 ** 0.5, lr, lr / 64 ** 0.5, lr)
    st = {}
    P.ops.render(P.ops.planes_to_nhwc(dev(inp["planes"])), dev(inp["rays_o"]), dev(inp["rays_d"]), dev(inp["jitter"]), dev(inp["u"]),
                 mlp, opts, ray_tile_w=side, stats=st,
                 ray_limits=None if inp["ray_limits"] is None else tuple(dev(x) for x in inp["ray_limits"]))
    info = P.ops.render_plan_info(N, R, side, opts, False, inp["ray_limits"] is not None)
    want = {False: 1, "pair": 2, "quad": 4}.get(small, info[0])
    assert info[0] == want and st["small_launch_kind"] == {1: None, 2: "pair", 4: "quad"}[want]
    assert st["tiles"] == info[1] and st["decode_steps"] == st["decode_steps_full"] == info[2]
