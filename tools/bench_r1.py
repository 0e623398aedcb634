#!/usr/bin/env python3
"""Timing of the R1 penalty (include/p3d_r1.h) at the trainer's size: img_resolution 512, 3 + 3 input channels,
channel_base 32768, channel_max 512; prints one JSON line and writes it to profiles/r1_bench.json.

  dreg      the Dreg phase's device work for one batch (default 4): forward on images that require grad, torch.autograd.grad(...,
            create_graph=True) inside ops.no_weight_gradients(), ops.r1_penalty, the backward of (penalty * gamma / 2).mean() into
            every parameter.  Next to it torch-ROCm fp32 double autograd of the same layers on the same GPU
            (tests/discriminator_cases.discriminator_f64 in binary32) and, for scale, the first-order step of
            tools/bench_discriminator.py.  Peak memory of each (torch.cuda.max_memory_allocated over one call).
  tangent   p3d_conv2d_mask_f32 on b512.conv0's shape against the two launches it fuses (p3d_conv2d_act_f32 with a linear epilogue,
            then p3d_bias_act_backward_f32).

dreg: medians of --iters calls between HIP events after a warm-up call (torch's comparator: --torch-iters).  tangent: medians of
--iters windows of 10 calls, the two candidates alternating.

    python tools/bench_r1.py [--iters 5] [--torch-iters 3] [--batch 4] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import discriminator_cases as DC  # noqa: E402

KW = dict(c_dim=25, img_resolution=512, img_channels=3, cond_mode="resnetcond_8", channel_base=32768, channel_max=512, conv_clamp=256,
          epilogue_kwargs={"mbstd_group_size": 4})
GAMMA = 10.0


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


def alternating_ms(fa, fb, windows, calls=10):
    """Medians of `windows` windows of `calls` calls each, the two candidates taking turns (both warmed first): (ms per call of fa, of fb)."""
    fa(), fb()
    torch.cuda.synchronize()
    out = ([], [])
    for _ in range(windows):
        for fn, dst in ((fa, out[0]), (fb, out[1])):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                fn()
            b.record()
            torch.cuda.synchronize()
            dst.append(a.elapsed_time(b) / calls)
    return statistics.median(out[0]), statistics.median(out[1])


def peak_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--torch-iters", type=int, default=3)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r1_bench.json"))
    args = ap.parse_args()
    import panic3d_amd as P
    P._lib.lib()
    torch.manual_seed(0)
    N = args.batch
    D = P.DualDiscriminator(**KW).cuda()
    D.set_r1_grad(True)
    pd = {n: q.detach().clone().requires_grad_(True) for n, q in D.named_parameters()}
    image0, raw0 = torch.randn(N, 3, 512, 512, device="cuda"), torch.randn(N, 3, 128, 128, device="cuda")
    c, feats = torch.randn(N, 25, device="cuda"), torch.randn(N, 16, device="cuda")

    def ours_dreg():
        image, raw = image0.clone().requires_grad_(True), raw0.clone().requires_grad_(True)
        logits = D({"image": image, "image_raw": raw}, c, {"resnet_feats": feats})
        with P.ops.no_weight_gradients():
            g = torch.autograd.grad([logits.sum()], [image, raw], create_graph=True, only_inputs=True)
        (P.ops.r1_penalty(*g) * (GAMMA / 2)).mean().backward()
        D.zero_grad(set_to_none=True)

    def torch_dreg():
        image, raw = image0.clone().requires_grad_(True), raw0.clone().requires_grad_(True)
        logits = DC.discriminator_f64(pd, image, raw, c, feats, KW)
        gi, gr = torch.autograd.grad([logits.sum()], [image, raw], create_graph=True, only_inputs=True)
        ((gi.square().sum([1, 2, 3]) + gr.square().sum([1, 2, 3])) * (GAMMA / 2)).mean().backward()
        for q in pd.values():
            q.grad = None

    def ours_step():
        image, raw = image0.clone().requires_grad_(True), raw0.clone().requires_grad_(True)
        F.softplus(-D({"image": image, "image_raw": raw}, c, {"resnet_feats": feats})).mean().backward()
        D.zero_grad(set_to_none=True)

    dreg = {"N": N, "dreg_ms": round(ev_ms(ours_dreg, args.iters), 3), "torch_fp32_dreg_ms": round(ev_ms(torch_dreg, args.torch_iters), 3),
            "first_order_step_ms": round(ev_ms(ours_step, args.iters), 3)}
    dreg["dreg_over_torch"] = round(dreg["dreg_ms"] / dreg["torch_fp32_dreg_ms"], 3)
    dreg.update(dreg_peak_mib=peak_mib(ours_dreg), torch_fp32_dreg_peak_mib=peak_mib(torch_dreg), first_order_step_peak_mib=peak_mib(ours_step))

    # the tangent layer on b512.conv0's shape: [N,64,512,512] -> [N,64,512,512], 3x3, lrelu, clamp 256
    conv0 = D.b512.conv0
    Ci, Co = conv0.in_channels, conv0.out_channels
    h = torch.randn(N, Ci, 512, 512, device="cuda")
    pre = torch.randn(N, Co, 512, 512, device="cuda") * 100
    with torch.no_grad():
        wk = conv0._wk()
    meta = ("lrelu", conv0.act_gain, float(conv0.conv_clamp))

    def fused():
        P.ops._conv2d_mask_impl(h, wk, pre, *meta, 1, 1)

    def two_launches():
        z = P.ops._conv2d_act_impl(h, wk, None, "linear", 1.0, None, 1, 1, None)
        P.ops._bias_act_backward_meta(pre, z, meta)
    assert torch.equal(P.ops._conv2d_mask_impl(h, wk, pre, *meta, 1, 1),
                       P.ops._bias_act_backward_meta(pre, P.ops._conv2d_act_impl(h, wk, None, "linear", 1.0, None, 1, 1, None), meta)[0])
    t_fused, t_two = alternating_ms(fused, two_launches, args.iters)
    tangent = {"shape": [N, Ci, Co, 512, 512], "fused_ms": round(t_fused, 3), "two_launches_ms": round(t_two, 3)}
    tangent["fused_over_two"] = round(tangent["fused_ms"] / tangent["two_launches_ms"], 3)
    line = json.dumps({"bench": "r1", "network": "512^2, 3+3 channels, channel_base 32768, channel_max 512", "iters": args.iters, "torch_iters": args.torch_iters, "dreg": dreg,
                       "tangent_b512_conv0": tangent})
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
