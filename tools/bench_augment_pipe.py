#!/usr/bin/env python3
"""Timing of the augmentation pipe (panic3d_amd/augment.py, include/p3d_augment_tail.h) at the trainer's size, batch
4 x 6 x 512^2; prints one JSON line and writes it to profiles/augment_pipe_bench.json.

  tail   ops.augment_tail with 43 taps, noise and cutout: forward, and forward + adjoint under autograd, against a torch composition of
         the same steps on the same GPU (tests/augment_pipe_cases.torch_tail: F.pad reflect, the two grouped F.conv2d, add, multiply)
         with torch's autograd.  Medians over --repeats windows of --calls back-to-back calls between HIP events after a warm-up,
         alternating with the comparator.  `hbm_bound_frac`: the compulsory traffic (image in, noise in, image out; cotangent in and
         out for the adjoint) at 8 TB/s over the measured time.
  pipe   one whole AugmentPipe call, wall time with a synchronisation after each call (the draws on the host are part of it), for the
         trainer's twelve transforms (BGC) and for all fifteen, against a torch composition that draws its parameters on the device with
         the reference's sequence of torch calls and reads its margins back as the reference does (one device-to-host copy per call),
         then runs tests/augment_cases.torch_operator and torch_tail.  `fresh_draws`: every call draws anew, so the margins and with
         them the comparator's convolution shapes change from call to call, and torch's convolution back end chooses an algorithm for
         every new shape; `repeated_draw`: both sides reseed before every call, so the shapes repeat and that choice is cached.
Where ours/torch > 1 the package is slower than torch's composition: the ratio is recorded as measured.

    python tools/bench_augment_pipe.py [--repeats 7] [--calls 10] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import augment_cases as AC  # noqa: E402
import augment_pipe_cases as PC  # noqa: E402
from bench_augment import compare  # noqa: E402

SHAPE = (4, 6, 512, 512)
HBM_BYTES_PER_S = 8e12
ALL15 = dict(**AC.BGC, imgfilter=1, noise=1, cutout=1)


def wall_ms(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def compare_wall(ours, theirs, repeats, calls):
    for fn in (ours, theirs):
        for _ in range(2):
            fn()
    t = {"ours": [], "torch": []}
    for _ in range(repeats):
        t["ours"].append(wall_ms(ours, calls))
        t["torch"].append(wall_ms(theirs, calls))
    med = {k: statistics.median(v) for k, v in t.items()}
    return {"ours_ms": round(med["ours"], 4), "torch_ms": round(med["torch"], 4), "ours_over_torch": round(med["ours"] / med["torch"], 3),
            "ours_min_max_ms": [round(min(t["ours"]), 4), round(max(t["ours"]), 4)],
            "torch_min_max_ms": [round(min(t["torch"]), 4), round(max(t["torch"]), 4)]}


def device_pipe(pipe, hz):
    """The comparator of the whole call: the pipe's transforms from torch's operators, the parameters drawn on the device in the
    reference's sequence, the margins (and the matrices the stand-in composes on the host) read back in one copy."""
    op = AC.torch_operator(hz)
    fbank = pipe.Hz_fbank
    eye3, eye4 = torch.eye(3, device=fbank.device), torch.eye(4, device=fbank.device)
    v = torch.tensor([1, 1, 1, 0], device=fbank.device) / np.sqrt(3)
    vv = v.ger(v)

    def mat(*rows):
        ref = [e for r in rows for e in r if isinstance(e, torch.Tensor)][0]
        return torch.stack([e if isinstance(e, torch.Tensor) else torch.full_like(ref, float(e)) for r in rows for e in r], dim=-1).reshape(ref.shape + (len(rows), -1))

    def rot(t):
        return mat([torch.cos(t), torch.sin(-t), 0], [torch.sin(t), torch.cos(t), 0], [0, 0, 1])

    def fn(x):
        N, ch, H, W = x.shape
        dev, p = x.device, pipe.p
        rand, randn = (lambda *s: torch.rand(s, device=dev)), (lambda *s: torch.randn(s, device=dev))
        pick = lambda strength, shape, a, b: torch.where(rand(*shape) < strength * p, a, b)
        i = pick(pipe.xflip, (N,), torch.floor(rand(N) * 2), torch.zeros(N, device=dev))
        G = eye3 @ mat([1 / (1 - 2 * i), 0, 0], [0, 1, 0], [0, 0, 1])
        i = pick(pipe.rotate90, (N,), torch.floor(rand(N) * 4), torch.zeros(N, device=dev))
        G = G @ rot(np.pi / 2 * i)
        t = pick(pipe.xint, (N, 1), (rand(N, 2) * 2 - 1) * pipe.xint_max, torch.zeros(N, 2, device=dev))
        G = G @ mat([1, 0, -torch.round(t[:, 0] * W)], [0, 1, -torch.round(t[:, 1] * H)], [0, 0, 1])
        s = pick(pipe.scale, (N,), torch.exp2(randn(N) * pipe.scale_std), torch.ones(N, device=dev))
        G = G @ mat([1 / s, 0, 0], [0, 1 / s, 0], [0, 0, 1])
        p_rot = 1 - torch.sqrt((1 - pipe.rotate * p).clamp(0, 1))
        th = torch.where(rand(N) < p_rot, (rand(N) * 2 - 1) * np.pi * pipe.rotate_max, torch.zeros(N, device=dev))
        G = G @ rot(th)
        s = pick(pipe.aniso, (N,), torch.exp2(randn(N) * pipe.aniso_std), torch.ones(N, device=dev))
        G = G @ mat([1 / s, 0, 0], [0, s, 0], [0, 0, 1])
        th = torch.where(rand(N) < p_rot, (rand(N) * 2 - 1) * np.pi * pipe.rotate_max, torch.zeros(N, device=dev))
        G = G @ rot(th)
        t = pick(pipe.xfrac, (N, 1), randn(N, 2) * pipe.xfrac_std, torch.zeros(N, 2, device=dev))
        G = G @ mat([1, 0, -t[:, 0] * W], [0, 1, -t[:, 1] * H], [0, 0, 1])
        cx, cy = (W - 1) / 2, (H - 1) / 2
        cp = G @ torch.tensor([[-cx, -cy, 1], [cx, -cy, 1], [cx, cy, 1], [-cx, cy, 1]], device=dev).t()
        m = cp[:, :2, :].permute(1, 0, 2).flatten(1)
        m = torch.cat([-m, m]).max(dim=1).values + torch.tensor([6 - cx, 6 - cy] * 2, device=dev)
        m = m.max(torch.zeros(4, device=dev)).min(torch.tensor([W - 1, H - 1] * 2, device=dev)).ceil()
        back = torch.cat([G.reshape(-1), m]).cpu().numpy()  # the read-back: the reference's `margin.ceil().to(torch.int32)` unpacking
        G_host, margins = back[:-4].reshape(N, 3, 3), tuple(int(k) for k in back[-4:])
        b = pick(pipe.brightness, (N,), randn(N) * pipe.brightness_std, torch.zeros(N, device=dev))
        C = mat([1, 0, 0, b], [0, 1, 0, b], [0, 0, 1, b], [0, 0, 0, 1]) @ eye4
        c = pick(pipe.contrast, (N,), torch.exp2(randn(N) * pipe.contrast_std), torch.ones(N, device=dev))
        C = mat([c, 0, 0, 0], [0, c, 0, 0], [0, 0, c, 0], [0, 0, 0, 1]) @ C
        i = pick(pipe.lumaflip, (N, 1, 1), torch.floor(rand(N, 1, 1) * 2), torch.zeros(N, 1, 1, device=dev))
        C = (eye4 - 2 * vv * i) @ C
        th = pick(pipe.hue, (N,), (rand(N) * 2 - 1) * np.pi * pipe.hue_max, torch.zeros(N, device=dev))
        sn, cs = torch.sin(th), torch.cos(th)
        cc, a = 1 - cs, 1 / np.sqrt(3)
        C = mat([a * a * cc + cs, a * a * cc - a * sn, a * a * cc + a * sn, 0], [a * a * cc + a * sn, a * a * cc + cs, a * a * cc - a * sn, 0],
                [a * a * cc - a * sn, a * a * cc + a * sn, a * a * cc + cs, 0], [0, 0, 0, 1]) @ C
        s = pick(pipe.saturation, (N, 1, 1), torch.exp2(randn(N, 1, 1) * pipe.saturation_std), torch.ones(N, 1, 1, device=dev))
        C = (vv + (eye4 - vv) * s) @ C
        x = op(x, G_host, margins, C)
        if pipe.imgfilter > 0:
            power = torch.tensor([10, 1, 1, 1], device=dev) / 13
            g = torch.ones(N, 4, device=dev)
            for k, strength in enumerate(pipe.imgfilter_bands):
                t_k = pick(pipe.imgfilter * strength, (N,), torch.exp2(randn(N) * pipe.imgfilter_std), torch.ones(N, device=dev))
                t = torch.ones(N, 4, device=dev)
                t[:, k] = t_k
                g = g * (t / (power * t.square()).sum(dim=-1, keepdim=True).sqrt())
            x = PC.torch_tail(x, g @ fbank)
        if pipe.noise > 0:
            sigma = pick(pipe.noise, (N, 1, 1, 1), randn(N, 1, 1, 1).abs() * pipe.noise_std, torch.zeros(N, 1, 1, 1, device=dev))
            x = x + torch.randn(x.shape, device=dev) * sigma
        if pipe.cutout > 0:
            size = pick(pipe.cutout, (N, 1, 1, 1, 1), torch.full((N, 2, 1, 1, 1), pipe.cutout_size, device=dev), torch.zeros(N, 2, 1, 1, 1, device=dev))
            center = rand(N, 2, 1, 1, 1)
            mx = ((torch.arange(W, device=dev).reshape(1, 1, 1, -1) + 0.5) / W - center[:, 0]).abs() >= size[:, 0] / 2
            my = ((torch.arange(H, device=dev).reshape(1, 1, -1, 1) + 0.5) / H - center[:, 1]).abs() >= size[:, 1] / 2
            x = x * torch.logical_or(mx, my).to(torch.float32)
        return x
    return fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment_pipe_bench.json"))
    args = ap.parse_args()
    import panic3d_amd as P
    dev = torch.device("cuda")
    N, C, H, W = SHAPE
    hz = P.ops.augment_filter_tables()[0]
    x, g = torch.randn(SHAPE, device=dev), torch.randn(SHAPE, device=dev)
    batch_bytes = 4 * N * C * H * W
    result = {"shape": list(SHAPE), "device": torch.cuda.get_device_name(0), "repeats": args.repeats, "calls": args.calls,
              "source_hash": P._build.source_hash(), "tail_plan_43_taps": list(P.ops.augment_tail_plan(43))}
    # the tail
    d = P.AugmentPipe(imgfilter=1, noise=1, cutout=1).draw(*SHAPE, debug_percentile=0.8)
    taps, sigma, rect = (torch.from_numpy(a).to(dev) for a in (d.taps, d.sigma, d.rect))
    z = torch.randn(SHAPE, device=dev)
    tail = P.ops.AugmentTail(taps, z, sigma, rect)

    def ours_fwd():
        with torch.no_grad():
            return P.ops.augment_tail(x, tail)

    def ours_both():
        xt = x.detach().requires_grad_(True)
        return torch.autograd.grad(P.ops.augment_tail(xt, tail), xt, g)

    def torch_fwd():
        with torch.no_grad():
            return PC.torch_tail(x, taps, z, sigma, rect)

    def torch_both():
        xt = x.detach().requires_grad_(True)
        return torch.autograd.grad(PC.torch_tail(xt, taps, z, sigma, rect), xt, g)
    fwd, both = compare(ours_fwd, torch_fwd, args.repeats, args.calls), compare(ours_both, torch_both, args.repeats, args.calls)
    fwd["hbm_bound_frac"] = round(3 * batch_bytes / HBM_BYTES_PER_S / (fwd["ours_ms"] * 1e-3), 4)
    both["hbm_bound_frac"] = round(5 * batch_bytes / HBM_BYTES_PER_S / (both["ours_ms"] * 1e-3), 4)
    result["tail"] = {"comparator": "torch composition of the same steps on the same GPU (F.pad reflect, two grouped F.conv2d, add, multiply)",
                      "forward": fwd, "forward_adjoint": both}
    # the whole call
    result["pipe"] = {"comparator": "torch composition, parameters drawn on the device, margins read back once per call; wall time, synchronised per call"}
    for name, kwargs in (("bgc", AC.BGC), ("all15", ALL15)):
        pipe = P.AugmentPipe(**kwargs).to(dev)
        pipe.set_p(0.6)
        theirs = device_pipe(pipe, hz)

        def ours_call():
            with torch.no_grad():
                return pipe(x)

        def torch_call():
            with torch.no_grad():
                return theirs(x)

        def reseeded(fn):
            def call():
                torch.manual_seed(0)  # the host's and the device's generators: every call draws the same parameters
                return fn()
            return call
        result["pipe"][name] = {"fresh_draws": compare_wall(ours_call, torch_call, args.repeats, args.calls),
                                "repeated_draw": compare_wall(reseeded(ours_call), reseeded(torch_call), args.repeats, args.calls)}
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
