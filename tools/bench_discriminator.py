#!/usr/bin/env python3
"""Timing of the dual discriminator (include/p3d_discriminator.h) at the trainer's size: img_resolution 512, 3 + 3
input channels, channel_base 32768, channel_max 512; prints one JSON line and writes it to profiles/discriminator_bench.json.

Per batch size (4 and 1): the no-grad forward and forward + backward (softplus(-logits).mean() -> the images and every parameter),
each the median of --iters runs timed with HIP events after a warm-up; next to them torch-ROCm fp32 autograd of the same layers on
the same GPU (tests/discriminator_cases.discriminator_f64 in binary32: F.conv2d and torch stand-ins of upfirdn2d and bias_act).
`layers` gives forward + backward of each block on its own for the first batch size, ours and torch's, so that a block that loses
is named.

    python tools/bench_discriminator.py [--iters 5] [--batches 4,1] [--out FILE]
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


def torch_block(p, b, x):
    """One resnet block of discriminator_f64 (without fromrgb), binary32."""
    f = torch.tensor([1.0, 3.0, 3.0, 1.0], device=x.device)
    f = f.ger(f) / 64

    def conv(name, x, act, down=1, gain=1.0, clamp=256.0):
        w = p[f"{b}.{name}.weight"]
        k = w.shape[-1]
        w = w * (1 / (w.shape[1] * k * k) ** 0.5)
        stride, pad = 1, k // 2
        if down == 2:
            x = DC.upfirdn2d_torch(x, f, down=2 if k == 1 else 1, padding=pad + 1)
            stride, pad = (1 if k == 1 else 2), 0
        return DC.bias_act_any(F.conv2d(x, w, stride=stride, padding=pad), p.get(f"{b}.{name}.bias"), act,
                               (DC.SQRT2 if act == "lrelu" else 1.0) * gain, None if clamp is None else clamp * gain)
    y = conv("skip", x, "linear", 2, DC.SQRT_HALF, None)
    return y + conv("conv1", conv("conv0", x, "lrelu"), "lrelu", 2, DC.SQRT_HALF)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--batches", default="4,1")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "discriminator_bench.json"))
    args = ap.parse_args()
    import panic3d_amd as P
    P._lib.lib()
    torch.manual_seed(0)
    D = P.DualDiscriminator(**KW).cuda()
    pd = {n: q.detach().clone().requires_grad_(True) for n, q in D.named_parameters()}
    rows, layers = [], []
    batches = [int(b) for b in args.batches.split(",")]
    for N in batches:
        image = torch.randn(N, 3, 512, 512, device="cuda", requires_grad=True)
        raw = torch.randn(N, 3, 128, 128, device="cuda", requires_grad=True)
        c, feats = torch.randn(N, 25, device="cuda"), torch.randn(N, 16, device="cuda")

        def ours_fwd():
            with torch.no_grad():
                D({"image": image, "image_raw": raw}, c, {"resnet_feats": feats})

        def ours_step():
            F.softplus(-D({"image": image, "image_raw": raw}, c, {"resnet_feats": feats})).mean().backward()
            D.zero_grad(set_to_none=True)

        def torch_fwd():
            with torch.no_grad():
                DC.discriminator_f64(pd, image, raw, c, feats, KW)

        def torch_step():
            F.softplus(-DC.discriminator_f64(pd, image, raw, c, feats, KW)).mean().backward()
        rows.append({"N": N, "fwd_ms": round(ev_ms(ours_fwd, args.iters), 3), "fwd_bwd_ms": round(ev_ms(ours_step, args.iters), 3),
                     "torch_fp32_fwd_ms": round(ev_ms(torch_fwd, args.iters), 3), "torch_fp32_fwd_bwd_ms": round(ev_ms(torch_step, args.iters), 3)})
    N = batches[0]
    for res in D.block_resolutions:
        blk = getattr(D, f"b{res}")
        Ci = blk.conv0.in_channels
        x = torch.randn(N, Ci, res, res, device="cuda", requires_grad=True)

        def ours():  # (the block's three layers as DiscriminatorBlock.forward calls them; fromrgb left out on both sides)
            y = blk.skip(x, gain=DC.SQRT_HALF)
            blk.conv1(blk.conv0(x), gain=DC.SQRT_HALF, res=y).sum().backward()

        def theirs():
            torch_block(pd, f"b{res}", x).sum().backward()
        layers.append({"block": f"b{res}", "channels": [Ci, blk.conv1.out_channels], "fwd_bwd_ms": round(ev_ms(ours, args.iters), 3),
                       "torch_fp32_fwd_bwd_ms": round(ev_ms(theirs, args.iters), 3)})
    line = json.dumps({"bench": "discriminator", "network": "512^2, 3+3 channels, channel_base 32768, channel_max 512", "rows": rows,
                       "layers_N": N, "layers": layers})
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
