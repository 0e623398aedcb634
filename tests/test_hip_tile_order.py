"""GPU: k_render's tile order is a pure permutation of which wave renders which tile.  The smallest launches that take each
branch of the order (csrc/p3d_render_plan.hpp) — 256 x 256 rays: the balanced pieces; 256 x 128 rays: 4 super-tiles, the fallback
to runs of blocks; 2 views of 256 x 256 with a clamp range per view — at 48+48 with the surface bench scene, in the exact and the
tolerance mode: the screen-tiled launch (ray_tile_w = width) and the unstructured ray list (ray_tile_w = 0: the trivial order)
give the same bits in all four outputs from the same draws.

The wave-level decode-step count of the tiled launch is a property of the tiles, not of their order: when the environment names
a library built with -DP3D_TILE_ORDER_PARENT (P3D_TILE_ORDER_PARENT_LIB), a child process renders the same launches with it and
the counts must be equal; without one that comparison is left out."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import p3d_testing as T

pytestmark = pytest.mark.gpu

SC, SF = 48, 48
# name -> (views, width, height, per-view clamp)
LAUNCHES = {"256x256 pieces": (1, 256, 256, False), "256x128 fallback": (1, 256, 128, False), "2 x 256x256 per-view clamp": (2, 256, 256, True)}


def render_all(hip):
    """{(launch, mode): (tiled outputs, untiled outputs, decode steps of the tiled launch)}"""
    dev = torch.device("cuda")
    planes_np, raw = T.make_bench_scene("surface")
    nhwc1 = hip.ops.planes_to_nhwc(torch.from_numpy(planes_np).to(dev))
    mlp = hip.ops.prescale_mlp(*(torch.from_numpy(x).to(dev) for x in raw), 1 / np.sqrt(32), 1.0, 1 / np.sqrt(64), 1.0)
    ro = T.bench_rendering_kwargs(SC, SF)
    res = {}
    for name, (N, W, H, per_view) in LAUNCHES.items():
        labels = torch.stack([hip.cameras.camera_label(0.0, 20.0 + 70.0 * v, 1.0, 30.0) for v in range(N)])
        o, d = hip.cameras.rays_from_label(labels, W)  # W x W rays: the launch takes the top H rows
        R = W * H
        o, d = o[:, :R].contiguous().to(dev), d[:, :R].contiguous().to(dev)
        jit, u = T.make_random_draws(61, N, R, SC, SF)
        jit, u = torch.from_numpy(jit).to(dev), torch.from_numpy(u).to(dev)
        nhwc = nhwc1.expand(N, *nhwc1.shape[1:]).contiguous()
        for fast in (False, True):
            opts = hip.ops.make_opts(ro, fast_color=fast, **T.BENCH_KW)
            st = {}
            tiled = hip.ops.render(nhwc, o, d, jit, u, mlp, opts, ray_tile_w=W, stats=st, per_view_clamp=per_view)
            assert not st["small_launch_kernel"] and st["tiles"] == N * R // 32
            flat = hip.ops.render(nhwc, o, d, jit, u, mlp, opts, ray_tile_w=0, per_view_clamp=per_view)
            res[(name, "tolerance" if fast else "exact")] = (tiled, flat, st["decode_steps"])
    torch.cuda.synchronize()
    return res


@pytest.fixture(scope="module")
def rendered():
    import panic3d_amd
    assert torch.cuda.is_available()
    panic3d_amd._lib.lib()
    return render_all(panic3d_amd)


@pytest.mark.parametrize("mode", ["exact", "tolerance"])
@pytest.mark.parametrize("launch", list(LAUNCHES))
def test_tiled_launch_equals_the_ray_list(rendered, launch, mode):
    tiled, flat, steps = rendered[(launch, mode)]
    for name, a, b in zip(("feat", "depth", "wsum", "xyz"), tiled, flat):
        assert torch.equal(a, b), name
    wsum = tiled[2]
    assert 0.05 < float(wsum.mean()) < 0.999 and steps > 0  # hit and empty rays: uneven tiles


def test_decode_steps_do_not_depend_on_the_order(rendered):
    parent = os.environ.get("P3D_TILE_ORDER_PARENT_LIB")
    if not parent:
        return  # no library with the round-5 order at hand: nothing to compare with
    env = dict(os.environ, P3D_LIB=parent)
    out = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    theirs = json.loads(out.stdout.strip().splitlines()[-1])
    ours = {f"{k[0]} / {k[1]}": v[2] for k, v in rendered.items()}
    assert ours == theirs


if __name__ == "__main__":  # the child of test_decode_steps_do_not_depend_on_the_order: the library P3D_LIB names
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import panic3d_amd
    print(json.dumps({f"{k[0]} / {k[1]}": v[2] for k, v in render_all(panic3d_amd).items()}))
