#!/usr/bin/env python3
"""Timing of the 512^2 super-resolution's backward (SuperresolutionHybrid8XDC under autograd, TriPlaneGenerator.set_superresolution_grad;
DESIGN.md §4.9): 128^2 x 32 channels -> 512^2, 256 hidden channels, the case of tests/superres_grad_cases.py.  Prints one JSON line
and writes it to profiles/superres_grad_bench.json.

Per batch size: the no-grad forward, the grad-mode forward (the same bits) and the backward (sum(image * g) -> rgb, the feature image,
ws and every parameter), each the median of --iters runs timed with HIP events after a warm-up; and, as the baseline a user would
otherwise have, forward + backward of torch-ROCm autograd on an fp32 restatement of the same two blocks.

    python tools/bench_superres_grad.py [--iters 10] [--batches 1,4] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import superres_grad_cases as SRC  # noqa: E402
import synthesis_restatement as S  # noqa: E402


def ev_ms(fn, iters):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def restated(p, rgb, x, ws, filt, clamp):
    """superresolution.py:282-293 on networks_stylegan2.py's blocks in plain torch (constant noise)."""
    w = ws[:, -1]
    img = rgb
    for b in ("block0", "block1"):
        x = S._layer(p, b + ".conv0", x, w, 2, filt, clamp, None)
        x = S._layer(p, b + ".conv1", x, w, 1, filt, clamp, None)
        W = p[b + ".torgb.weight"]
        s = S._affine(p, b + ".torgb", w) * (1.0 / np.sqrt(W.shape[1]))
        v = (F.conv2d(x * s[:, :, None, None], W) + p[b + ".torgb.bias"][None, :, None, None]).clamp(-clamp, clamp)
        img = S._upfirdn_up2(img, filt) + v
    return img


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--batches", default="1,4")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "superres_grad_bench.json"))
    args = ap.parse_args()
    import panic3d_amd as P
    P._lib.lib()
    sr = SRC.fill(P.generator.SuperresolutionHybrid8XDC(**SRC.SR_KW)).cuda().eval()
    sr.record_grad = True
    filt = sr.block0.resample_filter
    rows = []
    for N in (int(b) for b in args.batches.split(",")):
        g = torch.Generator().manual_seed(N)
        rgb = torch.randn(N, 3, 128, 128, generator=g).cuda().requires_grad_(True)
        x = torch.randn(N, 32, 128, 128, generator=g).cuda().requires_grad_(True)
        ws = torch.randn(N, 3, 512, generator=g).cuda().requires_grad_(True)
        gi = torch.randn(N, 3, 512, 512, generator=g).cuda()

        def fwd_nograd():
            with torch.no_grad():
                sr(rgb, x, ws, noise_mode="const")

        def fwd_grad():
            sr(rgb, x, ws, noise_mode="const")
        times = []
        for i in range(args.iters + 1):
            out = sr(rgb, x, ws, noise_mode="const")
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out.backward(gi)
            b.record()
            torch.cuda.synchronize()
            if i:
                times.append(a.elapsed_time(b))
            for t in [rgb, x, ws] + list(sr.parameters()):
                t.grad = None
            del out
        pd = {n: t.detach().clone().requires_grad_(t.dtype.is_floating_point) for n, t in list(sr.named_parameters()) + list(sr.named_buffers())}
        ins = [t.detach().clone().requires_grad_(True) for t in (rgb, x, ws)]

        def torch_step():
            restated(pd, *ins, filt, 256.0).backward(gi)
        rows.append({"N": N, "fwd_nograd_ms": round(ev_ms(fwd_nograd, args.iters), 3), "fwd_grad_ms": round(ev_ms(fwd_grad, args.iters), 3),
                     "bwd_ms": round(statistics.median(times), 3),
                     "torch_autograd_fp32_fwd_bwd_ms": round(ev_ms(torch_step, args.iters), 3)})
        torch.cuda.empty_cache()
    line = json.dumps({"bench": "superres_grad", "module": "SuperresolutionHybrid8XDC 128^2 x 32 -> 512^2, 256 hidden, clamp 256", "rows": rows})
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
