#!/usr/bin/env python3
"""Timing of the synthesis network's backward (include/p3d_synthesis_grad.h) on the 256^2 triplane backbone (96 channels, channel
max 512, unconditioned); prints one JSON line and writes it to profiles/synthesis_grad_bench.json.

Per batch size: the no-grad forward, the grad-mode forward (the same bits, every layer writing its fp32 result) and the backward
(sum(planes * g) -> ws and every synthesis parameter), each the median of --iters runs timed with HIP events after a warm-up, and
the convolution FLOP count of the forward (the backward does twice that: data and weight gradients); and, as the baseline a user would
otherwise have, forward + backward of torch-ROCm autograd on the fp32 restatement of the same network (tests/synthesis_restatement.py).

    python tools/bench_synthesis_grad.py [--iters 10] [--batches 1,4] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import synthesis_restatement as R  # noqa: E402


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


def conv_flops(net, N):
    f = 0
    for res in net.block_resolutions:
        blk = getattr(net, f"b{res}")
        for lname in ("conv0", "conv1"):
            if hasattr(blk, lname):
                l = getattr(blk, lname)
                hw = (res // 2) ** 2 if l.up == 2 else res * res
                f += 2 * N * l.out_channels * l.in_channels * 9 * hw
        f += 2 * N * blk.torgb.out_channels * blk.torgb.in_channels * res * res
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--batches", default="1,4")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "synthesis_grad_bench.json"))
    args = ap.parse_args()
    import panic3d_amd as P
    P._lib.lib()
    torch.manual_seed(0)
    G = P.stylegan2.Generator(z_dim=512, c_dim=25, w_dim=512, img_resolution=256, img_channels=96, cond_mode="none",
                              mapping_kwargs={"num_layers": 2}, channel_base=32768, channel_max=512, num_fp16_res=0).cuda().eval()
    net = G.synthesis
    rows = []
    for N in (int(b) for b in args.batches.split(",")):
        ws = (torch.randn(N, net.num_ws, 512, device="cuda") * 0.5).requires_grad_(True)
        g = torch.randn(N, 96, 256, 256, device="cuda")

        def fwd_nograd():
            with torch.no_grad():
                net(ws, None, noise_mode="const")

        def fwd_grad():
            net(ws, None, noise_mode="const")
        holder = {}

        def prep():
            holder["out"] = net(ws, None, noise_mode="const")
        prep()
        torch.cuda.synchronize()
        times = []
        for i in range(args.iters + 1):
            prep()
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            holder["out"].backward(g)
            b.record()
            torch.cuda.synchronize()
            if i:
                times.append(a.elapsed_time(b))
            ws.grad = None
            for p in net.parameters():
                p.grad = None
        # the baseline a user would otherwise have: torch-ROCm autograd of the fp32 restatement (tests/synthesis_restatement.py)
        pd = {n: t.detach().clone().requires_grad_(t.dtype.is_floating_point) for n, t in list(net.named_parameters()) + list(net.named_buffers())}
        wsr = ws.detach().clone().requires_grad_(True)

        def torch_step():
            R.synthesis(pd, wsr, None, "none", net.block_resolutions, net.b8.resample_filter, None).backward(g)
        rows.append({"N": N, "fwd_nograd_ms": round(ev_ms(fwd_nograd, args.iters), 3), "fwd_grad_ms": round(ev_ms(fwd_grad, args.iters), 3),
                     "bwd_ms": round(statistics.median(times), 3), "fwd_conv_gflop": round(conv_flops(net, N) / 1e9, 2),
                     "torch_autograd_fp32_fwd_bwd_ms": round(ev_ms(torch_step, args.iters), 3)})
    line = json.dumps({"bench": "synthesis_grad", "backbone": "256^2 x 96ch, channel_max 512", "rows": rows})
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
