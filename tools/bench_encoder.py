#!/usr/bin/env python3
"""Timing of the conditioning encoder (include/p3d_encoder.h) at the real size: one 512 x 512 subject, 2 x 3 x 256^2
into a ResNet-50, PCA to 512 channels; prints one JSON line and writes it to profiles/encoder_bench.json.

  call_ms      ResnetFeatureExtractorPCA.forward as generate.py would call it, wall clock with a synchronisation at the end (the image's
               copy into the arena, ONE call into the library, the result's clone);
  kernels_ms   the table walk alone (p3d_encoder_forward_f32), between two HIP events;
  torch_fp32_ms   torch-ROCm's own fp32 composition of the same FOLDED network on the same GPU (F.interpolate, F.conv2d with the
               folded weight and bias, F.relu, F.max_pool2d), between two HIP events;
each the median of --iters runs after a warm-up.  `launches`: the kernels one call starts, counted from the table and its plans (a
split convolution is two).  `layers`: every convolution on its own under its plan, with the rate it reaches.

    python tools/bench_encoder.py [--iters 20] [--size 512] [--no-torch] [--out FILE]
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

import encoder_cases as EC  # noqa: E402

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


def torch_network(recs, img):
    """The same folded records on torch's own operators."""
    bufs = {0: img}
    for r in recs:
        x = bufs[r["src"]]
        if r["kind"] == "prepare":
            x = x[:, :3]
            x = F.interpolate(torch.cat([x, x.flip(dims=(-1,))]), size=r["out_shape"][2:], mode="bilinear", align_corners=False)
            y = (x - r["w"].view(1, 3, 1, 1)) / r["b"].view(1, 3, 1, 1)
        elif r["kind"] == "maxpool":
            y = F.max_pool2d(x, 3, 2, 1)
        else:
            y = F.conv2d(x, r["tw"], r["b"], stride=r["stride"], padding=(r["k"] - 1) // 2)
            if r["res"] is not None:
                y = y + bufs[r["res"]]
            if r["relu"]:
                y = F.relu(y)
        bufs[r["dst"]] = y
    return bufs[recs[-1]["dst"]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "encoder_bench.json"))
    args = ap.parse_args()
    import panic3d_amd as P
    P._lib.lib()
    ops = P.ops
    S = args.size
    sd = EC.make_weights(pca_dim=512, seed=7, **EC.FULL)
    rfe = P.ResnetFeatureExtractorPCA(None, 512)
    EC.fill_model(rfe.rfe, sd)
    rfe.cuda()
    img = EC.make_image((1, 3, S, S), 1).cuda()
    out = rfe(img)
    prog, outputs = rfe.rfe.program(img.shape, 256, ("pca",))
    recs = prog.records
    row = {"size": S, "out": list(out.shape), "call_ms": wall_ms(lambda: rfe(img), args.iters),
           "kernels_ms": ev_ms(lambda: ops._encoder_forward_impl(prog), args.iters)}
    launches, layers, flop_total = 0, [], 0
    for r in recs:
        if r["kind"] != "conv":
            launches += 1
            continue
        (N, Ci, H, W), (_, Co, Ho, Wo), k, s = r["shape"], r["out_shape"], r["k"], r["stride"]
        pl = ops.enc_conv_plan(N, Ci, Co, Ho, Wo, k, s, r["plan"])
        launches += 2 if pl["split"] > 1 else 1
        x = torch.randn(N, Ci, H, W, device="cuda")
        res = torch.randn(N, Co, Ho, Wo, device="cuda") if r["res"] is not None else None
        ms = ev_ms(lambda: ops.enc_conv(x, r["w"], r["b"], k, s, res, r["relu"], r["plan"]), max(args.iters // 2, 3))
        flop = 2 * k * k * Ci * Co * Ho * Wo * N
        flop_total += flop
        layers.append({"layer": r["name"], "Ci": Ci, "Co": Co, "out": [Ho, Wo], "k": k, "stride": s, "tile": 64 if pl["tile"] == 1 else 32,
                       "split": pl["split"], "workgroups": pl["workgroups"], "ms": ms, "tflops": round(flop / ms / 1e9, 2)})
    if not args.no_torch:
        for r in recs:
            if r["kind"] == "conv":
                r["tw"] = EC.from_wk(r["w"], r["k"])
        with torch.no_grad():
            ref = torch_network(recs, img)
            row["rel_l2_vs_torch_fp32"] = EC.rel_l2(out.cpu(), ref.cpu().double())
            row["torch_fp32_ms"] = ev_ms(lambda: torch_network(recs, img), args.iters)
    line = json.dumps({"bench": "encoder", "network": f"resnet50 + pca 512, one {S}^2 subject, 2 x 3 x 256^2", "row": row,
                       "gflop": round(flop_total / 1e9, 2), "launches": launches, "arena_mb": round(prog.arena.numel() * 4 / 2 ** 20, 1),
                       "layers": layers})
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
