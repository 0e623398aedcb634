#!/usr/bin/env python3
"""Timing of LPIPS (include/p3d_lpips.h) at the trainer's size: batch 4 of 512 x 512 images against 4 targets, AlexNet
widths; prints one JSON line and writes it to profiles/lpips_bench.json.

The no-grad forward and forward + backward (the gradient of the mean distance with respect to the first image), each the median of
--iters runs timed with HIP events after a warm-up; next to them torch-ROCm's own fp32 composition of the same network on the same GPU
(tests/lpips_cases.distance: F.conv2d, F.max_pool2d, autograd).  `layers`: each trunk layer's forward and data gradient on its own at
the batch of 2N (forward) and N (backward), with the rate the forward reaches (2 K Co pixels FLOP over its time).  `launches`: the
kernels one call starts, counted from the operators it calls (the head's forward is two kernels) plus torch's concatenation of the pair.

    python tools/bench_lpips.py [--iters 20] [--batch 4] [--size 512] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import lpips_cases as LPC  # noqa: E402

KERNELS = {"_lpips_conv_relu_impl": 1, "_lpips_conv_relu_backward_impl": 1, "_lpips_pool_impl": 1, "_lpips_pool_backward_impl": 1,
           "_lpips_head_impl": 2, "_lpips_head_backward_impl": 1}


def ev_ms(fn, iters, warm=3):
    for _ in range(warm):
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
    return round(statistics.median(out), 4)


def count_launches(ops, fn):
    n, saved = [0], {}
    for name, kernels in KERNELS.items():
        saved[name] = getattr(ops, name)

        def wrapped(*a, _f=saved[name], _k=kernels, **k):
            n[0] += _k
            return _f(*a, **k)
        setattr(ops, name, wrapped)
    try:
        fn()
    finally:
        for name, f in saved.items():
            setattr(ops, name, f)
    return n[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lpips_bench.json"))
    args = ap.parse_args()
    import panic3d_amd as P
    P._lib.lib()
    ops = P.ops
    N, S = args.batch, args.size
    weights = LPC.make_weights(LPC.FULL, 7)
    model = LPC.fill_model(P.LPIPS(), weights).cuda()
    wd = [tuple(t.cuda() for t in layer) for layer in weights]
    x0, x1 = (t.cuda() for t in LPC.make_images(N, S, S, 1))
    x0g = x0.clone().requires_grad_(True)

    def ours_fwd():
        with torch.no_grad():
            model(x0, x1)

    def ours_step():
        x0g.grad = None
        model(x0g, x1).mean().backward()

    def torch_fwd():
        with torch.no_grad():
            LPC.distance(x0, x1, wd, torch.float32)

    def torch_step():
        x0g.grad = None
        LPC.distance(x0g, x1, wd, torch.float32).mean().backward()

    with torch.no_grad():
        agree = float(((model(x0, x1).flatten() - LPC.distance(x0, x1, wd, torch.float32)).abs() / LPC.distance(x0, x1, wd, torch.float32)).max())
    fwd_launches = count_launches(ops, ours_fwd) + 1  # + torch.cat of the pair
    step_launches = count_launches(ops, ours_step) + 1
    row = {"N": N, "size": S, "fwd_ms": ev_ms(ours_fwd, args.iters), "fwd_bwd_ms": ev_ms(ours_step, args.iters),
           "torch_fp32_fwd_ms": ev_ms(torch_fwd, args.iters), "torch_fp32_fwd_bwd_ms": ev_ms(torch_step, args.iters),
           "value_rel_diff_vs_torch_fp32": agree}
    layers, net = [], model.operands()
    x = torch.cat([x0, x1])
    flop_total = 0
    for l, (wk, bias, wkb, lin, k, stride, pad, pool_after) in enumerate(net["layers"]):
        fold = (net["shift"], net["scale"]) if l == 0 else (None, None)
        a = ops.lpips_conv_relu(x, wk, bias, k, stride, pad, *fold)
        g = torch.randn_like(a[:N])
        Ci, Hi, Wi = x.shape[1:]
        fwd = ev_ms(lambda: ops.lpips_conv_relu(x, wk, bias, k, stride, pad, *fold), args.iters)
        ones = torch.ones(N, device="cuda")
        # (as the distance's backward calls them: the head's backward finishes the cotangent, the layer's backward reads that one tensor)
        bwd = ev_ms(lambda: ops.lpips_conv_relu_backward(g, None, None, wkb, k, Ci, Hi, Wi, stride, pad, fold[1]), args.iters)
        hd = ev_ms(lambda: ops.lpips_head(a[:N], a[N:], lin), args.iters)
        hdb = ev_ms(lambda: ops.lpips_head_backward(a[:N], a[N:], lin, ones, g, True), args.iters)
        flop = 2 * k * k * Ci * a.shape[1] * a.shape[2] * a.shape[3] * a.shape[0]
        flop_total += flop
        layers.append({"layer": l + 1, "in": [Ci, Hi, Wi], "out": list(a.shape[1:]), "K": k * k * Ci, "fwd_ms": fwd, "fwd_tflops": round(flop / fwd / 1e9, 2),
                       "dgrad_ms": bwd, "head_ms": hd, "head_bwd_ms": hdb})
        x = ops.lpips_pool(a) if pool_after else a
        if pool_after:
            layers[-1]["pool_ms"] = ev_ms(lambda: ops.lpips_pool(a), args.iters)
            layers[-1]["pool_bwd_ms"] = ev_ms(lambda: ops.lpips_pool_backward(a[:N], x[:N]), args.iters)
    line = json.dumps({"bench": "lpips", "network": f"alex, batch {N} + {N} targets, {S}^2", "row": row, "fwd_gflop": round(flop_total / 1e9, 2),
                       "launches": {"fwd": fwd_launches, "fwd_bwd": step_launches}, "layers": layers})
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
