#!/usr/bin/env python3
"""Timing of the illustration-to-render module (include/p3d_rmline.h) at the real size: one 512 x 512 RGBA subject
through the line detector and the six-layer generator; prints one JSON line and writes it to profiles/rmline_bench.json.

  call_ms         RMLineWrapper.forward as generate.py would call it, wall clock with a synchronisation at the end;
  walk_ms         the one-call walk alone (p3d_rmline_forward_f32: mask kernel + layers), between two HIP events;
  mask_ms         the mask kernel alone, between two HIP events;
  layers          every layer on its own (the operator ops.rmline_conv on the layer's real input size), between two HIP events, with
                  the rate it reaches: 2 * 9 * Ci * Co * Ho * Wo FLOP over its time (the last layer computes 16 columns for its 3);
  torch_fp32_ms   torch-ROCm's own fp32 composition of the same FOLDED network on the same GPU (a torch DoG with F.conv2d and
                  F.max_pool2d, F.pad, F.conv2d, F.leaky_relu, torch.tanh, torch.lerp), between two HIP events;
each the median of --iters runs after a warm-up.  `launches`: the kernels one call of the walk starts, as the library counts them.

    python tools/bench_rmline.py [--iters 20] [--size 512] [--no-torch] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import rmline_cases as RC  # noqa: E402

F = torch.nn.functional


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


def wall_ms(fn, iters, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(iters):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return round(statistics.median(out), 4)


def torch_module(img, hull, folded, dog, depth):
    """The wrapper on torch's own operators, binary32, with the same folded weights."""
    image = RC.composite(img)
    p = {k: dog[k] for k in ("t", "sigma", "k", "epsilon", "kernel_factor")}
    mask = (RC.batch_dog(img, **p) > 0.5).float()
    mask = RC.dilation(mask, dog["d"]) * (hull == 0)
    x = F.pad(torch.cat([image * (1 - mask), hull], dim=1), (depth,) * 4, mode="replicate")
    for w, b, act, slope in folded:
        x = F.conv2d(x, w, b)
        x = F.leaky_relu(x, slope) if act == "leaky" else torch.tanh(x)
    return torch.cat([torch.lerp(image, x, mask), img[:, 3:]], dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rmline_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rmline needs an MI355X: the HIP path has no CPU fallback")
    import panic3d_amd as P
    P._lib.lib()
    ops = P.ops
    S = args.size
    seq = RC.make_generator(seed=5, **RC.DEFAULT_ARCH)
    model = RC.fill_model(P.RMLineGenerator(), RC.state_dict_of(seq)).cuda()
    wrap = P.RMLineWrapper(model)
    depth = model.gen_depth
    img = RC.smooth_image(1, 4, S, S, 1).cuda()
    hull = (RC.make_hull(1, S, S) != 0).float().cuda()
    out, more = wrap(img, face_hull=hull, return_more=True)
    prog = model.program()
    walk = lambda: ops._rmline_forward_impl(prog, img, hull, wrap.dog, None, depth, P._lib.P3D_RMLINE_FWD_MASK_INPUT | P._lib.P3D_RMLINE_FWD_LERP)
    row = {"size": S, "out": list(out.shape), "mask_mean": round(float(more["line_mask"].mean()), 4),
           "call_ms": wall_ms(lambda: wrap(img, face_hull=hull), args.iters), "walk_ms": ev_ms(walk, args.iters),
           "mask_ms": ev_ms(lambda: ops.rmline_mask(img, hull, wrap.dog), args.iters)}
    launches = prog.launches
    layers, flop_total = [], 0
    mask, image = more["line_mask"], more["image"]
    for i, (wk, b, act, slope) in enumerate(model.folded()):
        Ci, Co = wk.shape[1:]
        Hin = S + 2 * depth - 2 * i
        first, last = i == 0, i == depth - 1
        x = None if first else torch.randn(1, Hin, Hin, Ci, device="cuda")
        fn = lambda: ops.rmline_conv(x, wk, b, act, slope, stack=(image, mask, hull) if first else None, pad=depth if first else 0, planar=last,
                                     lerp=(image, mask) if last else None)
        ms = ev_ms(fn, max(args.iters // 2, 3))
        flop = 2 * 9 * Ci * Co * (Hin - 2) ** 2
        flop_total += flop
        pl = ops.rmline_conv_plan(Ci, Co)
        layers.append({"layer": i, "Ci": Ci, "Co": Co, "out": [Hin - 2, Hin - 2], "act": act, "rows": pl["rows"], "lds_bytes": pl["lds_bytes"], "ms": ms,
                       "tflops": round(flop / ms / 1e9, 2)})
    row["layers_ms"] = round(sum(l["ms"] for l in layers), 4)
    row["tflops_walk"] = round(flop_total / row["walk_ms"] / 1e9, 2)
    if not args.no_torch:
        folded = [(wk.reshape(3, 3, wk.shape[1], wk.shape[2]).permute(3, 2, 0, 1).contiguous(), b, act, slope) for wk, b, act, slope in model.folded()]
        with torch.no_grad():
            ref = torch_module(img, hull, folded, wrap.dog, depth)
            row["rel_l2_vs_torch_fp32"] = RC.rel_l2(out.cpu(), ref.cpu().double())
            row["torch_fp32_ms"] = ev_ms(lambda: torch_module(img, hull, folded, wrap.dog, depth), args.iters)
            row["walk_over_torch"] = round(row["walk_ms"] / row["torch_fp32_ms"], 3)
    line = json.dumps({"bench": "rmline", "network": f"DoG mask + 6 x conv3x3 (4-32-32-32-32-32-3), one {S}^2 RGBA subject", "row": row,
                       "gflop": round(flop_total / 1e9, 2), "launches": launches, "layers": layers})
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
