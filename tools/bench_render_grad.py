#!/usr/bin/env python3
"""Timing of the renderer's backward pass (include/p3d_render_grad.h) on the surface bench scene; prints one JSON line.

Per size: forward ms without grad (today's kernel choice) and in grad mode (the depths_sorted dump: the every-sample kernel), the
backward ms (p3d_render_backward_f32, decoder and plane gradients), samples that ran the MLP backward, the atomic bytes they
issued (12 taps x 128 B each, an upper bound: taps out of range are skipped), the achieved atomic rate against the ~1.3 TB/s
chip-wide float-atomic floor, and torch autograd of the float64 restatement (tests/test_hip_render_grad.py) at the same merged
depths where it fits.  The per-kernel split (k_g_decode / k_g_ray / k_g_mlp / k_g_reduce) comes from a rocprofv3 kernel trace.

    python tools/bench_render_grad.py [--iters 5]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import p3d_testing as T  # noqa: E402

ATOMIC_FLOOR_TBS = 1.3


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    import panic3d_amd as P
    import test_hip_render_grad as TG
    dev = torch.device("cuda:0")
    P._lib.lib()
    planes_np, raw = T.make_bench_scene("surface")
    dec = TG.make_decoder(P, raw, True)
    rend = P.renderer.ImportanceRenderer(use_triplane=True)
    kw = {k: v for k, v in T.BENCH_KW.items() if k != "force_sigmoid"}
    base = torch.from_numpy(planes_np).to(dev)
    rows = []
    for res, Sc, Sf in ((128, 48, 48), (128, 96, 96), (512, 48, 48)):
        ro = T.bench_rendering_kwargs(Sc, Sf)
        o, d = P.cameras.rays_from_label(P.cameras.camera_label(0.0, 20.0, 1.0, 30.0)[None], res)
        o, d = o.to(dev), d.to(dev)
        N, R = o.shape[:2]
        torch.manual_seed(0)
        jitter, u = torch.rand(N, R, Sc, 1, device=dev), torch.rand(N * R, Sf, device=dev)
        cot = TG.cotangents(1, N, R)
        planes = base.detach().requires_grad_(True)

        def fwd_nograd():
            with torch.no_grad():
                rend(planes, dec, o, d, ro, jitter=jitter, u=u, **kw)

        def fwd_grad():
            return rend(planes, dec, o, d, ro, jitter=jitter, u=u, **kw)
        row = dict(res=res, Sc=Sc, Sf=Sf, forward_ms=round(timed(fwd_nograd, a.iters), 3), forward_grad_ms=round(timed(fwd_grad, a.iters), 3))
        opts = rend._opts(ro, dec, fast_color=P.renderer.DEFAULT_FAST_COLOR, **kw)
        with torch.no_grad():
            mlp = P.renderer.decoder_params(dec, live=False)
            nhwc = P.ops.planes_to_nhwc(base)
            *_, dm = P.ops.render(nhwc, o, d, jitter, u, mlp, opts, dumps=("depths_sorted", "sigma_sorted"))
        st = {}
        P.ops.render_backward(nhwc, o, d, dm["depths_sorted"], mlp, opts, cot, stats=st)
        row["backward_ms"] = round(timed(lambda: P.ops.render_backward(nhwc, o, d, dm["depths_sorted"], mlp, opts, cot), a.iters), 3)
        row["backward_decoder_only_ms"] = round(timed(lambda: P.ops.render_backward(nhwc, o, d, dm["depths_sorted"], mlp, opts, cot,
                                                                                   want_planes=False), a.iters), 3)
        row["samples"] = st["samples"]
        row["executed_samples"] = st["executed_samples"]
        row["executed_fraction"] = round(st["executed_samples"] / st["samples"], 4)
        atomic = st["executed_samples"] * 12 * 128
        row["atomic_bytes"] = atomic
        row["atomic_tb_s"] = round(atomic / (row["backward_ms"] * 1e-3) / 1e12, 3)
        row["atomic_floor_ms"] = round(atomic / (ATOMIC_FLOOR_TBS * 1e12) * 1e3, 3)
        row["scatter_share"] = round(1 - row["backward_decoder_only_ms"] / row["backward_ms"], 3)
        if not a.no_torch and res <= 128:
            try:
                row["torch_fp64_autograd_ms"] = round(timed(lambda: TG.restate64(base, mlp, o, d, dm["depths_sorted"].reshape(N, R, -1),
                                                                                 dm["sigma_sorted"], opts, ro, [c.double() for c in cot],
                                                                                 False, True), max(1, a.iters // 2)), 3)
            except torch.cuda.OutOfMemoryError:
                row["torch_fp64_autograd_ms"] = None
            torch.cuda.empty_cache()
        rows.append(row)
    print(json.dumps(dict(metric="render_backward", device=torch.cuda.get_device_name(0), atomic_floor_tb_s=ATOMIC_FLOOR_TBS, rows=rows)))


if __name__ == "__main__":
    main()
