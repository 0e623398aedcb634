#!/usr/bin/env python3
"""Timing of the front-view paste's forward and HIP backward (include/p3d_paste_grad.h) at the generator's sizes —
r = 128 render resolution, S = 512 illustration — for N = 1 and 4 views, beside torch autograd of the same post-process written as
the reference writes it (paste.paste_front_torch's differentiable part: interpolate, grid_sample, lerp) on the same inputs and the
same mask.  Prints one JSON line.

    python tools/bench_paste_grad.py [--iters 20] [--batches 1,4]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batches", default="1,4")
    args = ap.parse_args()
    import panic3d_amd as P
    from panic3d_amd import paste
    P._lib.lib()
    r, S, bw = 128, 512, 0.7
    rows = []
    for N in (int(b) for b in args.batches.split(",")):
        g = torch.Generator().manual_seed(N)
        c = lambda t: t.cuda()
        xyz = c(torch.randn(N, 3, r, r, generator=g) * 0.2).requires_grad_(True)
        front = c(torch.rand(N, 3, S, S, generator=g))
        weights, occ = c(torch.rand(N, 1, r, r, generator=g)), c(torch.rand(N, 1, r, r, generator=g))
        ro, rd = c(torch.randn(N, 3, r, r, generator=g)), c(F.normalize(torch.randn(N, 3, r, r, generator=g), dim=1))
        image = c(torch.randn(N, 3, S, S, generator=g)).requires_grad_(True)
        gi = c(torch.randn(N, 3, S, S, generator=g))
        a = (weights, xyz, occ, ro, rd, front, image, 0.4, 1e3, 0.5, 1e3, bw, True)

        def fwd_nograd():
            with torch.no_grad():
                P.ops.paste_front(*a)

        def fwd_grad():
            return P.ops.paste_front_grad(*a, grad_sample=True)
        mask = fwd_grad()["mask"]
        out = fwd_grad()["image"]

        def bwd():
            torch.autograd.grad(out, (image, xyz), gi, retain_graph=True)

        def torch_fwd():
            p = paste.sample_orthofront(front * 2 - 1, F.interpolate(xyz, S, mode="bilinear"), bw)
            return torch.lerp(image, p, mask)
        tout = torch_fwd()

        def torch_bwd():
            torch.autograd.grad(tout, (image, xyz), gi, retain_graph=True)
        rows.append({"N": N, "fwd_nograd_ms": round(ev_ms(fwd_nograd, args.iters), 4), "fwd_grad_ms": round(ev_ms(fwd_grad, args.iters), 4),
                     "bwd_ms": round(ev_ms(bwd, args.iters), 4), "torch_sample_lerp_fwd_ms": round(ev_ms(torch_fwd, args.iters), 4),
                     "torch_autograd_bwd_ms": round(ev_ms(torch_bwd, args.iters), 4)})
    print(json.dumps({"bench": "paste_grad", "r": r, "S": S, "grad_sample": True, "rows": rows}))


if __name__ == "__main__":
    main()
