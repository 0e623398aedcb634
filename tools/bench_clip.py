#!/usr/bin/env python3
"""Timing of CLIP's ViT-B/32 image tower (include/p3d_clip.h) at the evaluation's sizes: a pair of views (N = 2, what
one `clipsim` call of measure.py encodes) and a subject's worth (N = 28: 14 views, prediction and ground truth); prints one JSON line
and writes it to profiles/clip_bench.json.  Per batch size:

  walk_ms         the one-call walk of the preprocessed batch (p3d_clip_forward_f32), between two HIP events;
  call_ms         CLIPVisual.forward on 512^2 images as the evaluation would call it (front end + walk + the copy of the result), wall
                  clock with a synchronisation at the end;
  prepare_ms      the front end alone (two launches), between two HIP events;
  launches        the kernels one call of the walk starts (steps + split-K reductions);
  torch_fp32_ms   torch-ROCm's own fp32 composition of the same network on the same GPU (torch_tower below: F.conv2d for the patches,
                  F.layer_norm — one kernel per LayerNorm —, F.linear, explicit softmax attention by two batched matmuls), between two
                  HIP events; torch_fp32_call_ms the same as a synchronised wall-clock call;
  gbps_weights    351 MB of weights over walk_ms: the rate the weight-bound pair size reaches;
each the median of --iters runs after a warm-up.  Weights are seeded (no checkpoint is needed for a timing).

    python tools/bench_clip.py [--iters 20] [--no-torch] [--out FILE]
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

import clip_cases as CC  # noqa: E402


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


def torch_tower(sd, x, heads):
    """clip/model.py's VisionTransformer.forward on torch's own fp32 operators: the baseline the walk is timed against."""
    F = torch.nn.functional
    ln = lambda v, name: F.layer_norm(v, (v.shape[-1],), sd[name + ".weight"], sd[name + ".bias"], CC.EPS)
    w = sd["conv1.weight"]
    N, D = x.shape[0], w.shape[0]
    p = F.conv2d(x, w, stride=w.shape[-1]).reshape(N, D, -1).permute(0, 2, 1)
    v = ln(torch.cat([sd["class_embedding"].expand(N, 1, D), p], dim=1) + sd["positional_embedding"], "ln_pre")
    T = v.shape[1]
    i = 0
    while f"transformer.resblocks.{i}.ln_1.weight" in sd:
        b = f"transformer.resblocks.{i}"
        qkv = F.linear(ln(v, f"{b}.ln_1"), sd[f"{b}.attn.in_proj_weight"], sd[f"{b}.attn.in_proj_bias"])
        q, k, u = (t.reshape(N, T, heads, 64).transpose(1, 2) for t in qkv.split(D, dim=2))
        a = (torch.softmax(q @ k.transpose(-1, -2) * 0.125, dim=-1) @ u).transpose(1, 2).reshape(N, T, D)
        v = v + F.linear(a, sd[f"{b}.attn.out_proj.weight"], sd[f"{b}.attn.out_proj.bias"])
        f = F.linear(ln(v, f"{b}.ln_2"), sd[f"{b}.mlp.c_fc.weight"], sd[f"{b}.mlp.c_fc.bias"])
        v = v + F.linear(f * torch.sigmoid(1.702 * f), sd[f"{b}.mlp.c_proj.weight"], sd[f"{b}.mlp.c_proj.bias"])
        i += 1
    return ln(v[:, 0], "ln_post") @ sd["proj"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_clip needs an MI355X: the HIP path has no CPU fallback")
    import panic3d_amd as P
    P._lib.lib()
    sd = CC.make_weights(seed=1, **CC.FULL)
    model = P.CLIPVisual()
    model.load_state_dict(sd)
    model.cuda()
    sd_dev = {k: v.cuda() for k, v in sd.items()}
    weight_bytes = 4 * sum(p.numel() for p in model.parameters())
    rows = []
    for N in (2, 28):
        img = torch.rand(N, 3, 512, 512, generator=torch.Generator().manual_seed(N)).cuda()
        x = P.ops.clip_prepare(img, 224)
        prog, _ = model.program(N)
        out = model.encode_image(x)
        row = {"N": N, "launches": prog.launches, "walk_ms": ev_ms(lambda: P.ops._clip_forward_impl(prog), args.iters),
               "call_ms": wall_ms(lambda: model(img), args.iters), "prepare_ms": ev_ms(lambda: P.ops.clip_prepare(img, 224), args.iters)}
        row["gbps_weights"] = round(weight_bytes / row["walk_ms"] / 1e6, 1)
        row["tflops"] = round(N * 8.7e9 / row["walk_ms"] / 1e9, 2)
        if not args.no_torch:
            with torch.no_grad():
                ref = torch_tower(sd_dev, x, 12)
                row["rel_l2_vs_torch_fp32"] = CC.rel_l2(out.cpu(), ref.cpu().double())
                row["torch_fp32_ms"] = ev_ms(lambda: torch_tower(sd_dev, x, 12), args.iters)
                row["torch_fp32_call_ms"] = wall_ms(lambda: torch_tower(sd_dev, x, 12), args.iters)
                row["walk_over_torch"] = round(row["walk_ms"] / row["torch_fp32_ms"], 3)
        rows.append(row)
    line = json.dumps({"bench": "clip", "network": "ViT-B/32 image tower, 224^2, binary32, seeded weights", "weight_mb": round(weight_bytes / 1e6, 1),
                       "torch_baseline": "F.conv2d, F.layer_norm, F.linear, softmax attention by batched matmuls (tools/bench_clip.py torch_tower)",
                       "rows": rows})
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
