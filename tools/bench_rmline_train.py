#!/usr/bin/env python3
"""Timing of one training batch of the illustration-to-render module (panic3d_amd/rmline_train.py, include/p3d_rmline_grad.h, DESIGN.md
§4.19): `RMLineModel.fit_step` — the generator's step on B patches, then the discriminator's on 2 B — at B = 64, 256 and 1024 pairs of
21 x 21 patches (the reference fixes no batch size: `prep.bs` is the user's).  Prints one JSON line and writes it to
profiles/rmline_train_bench.json.  Per B:

  fit_step_ms            the whole batch between two HIP events; forward_ms / backward_ms / optim_ms its three phases (both steps
                         together), each between HIP events of their own: training_step, loss.backward(), optimizer.step();
  launches               the library's kernels of one fit_step (ops.RMLINE_LAUNCHES; the optimisers' two and torch's small ops —
                         slicing, the 16-value mean, the BCE — come on top);
  kernels                the three convolution kernels on the generator's 32 -> 32 layer at the discriminator step's size (2 B patches,
                         29 x 29 -> 27 x 27): forward (per-tap sums, as training runs it), data gradient, weight gradient, with 2 * 9 * Ci * Co * Ho * Wo * N FLOP over each time;
  torch_fp32_*           torch-ROCm's own fp32 autograd of the same step on the same GPU: the same modules, F.pad, torch.lerp,
                         torch.optim.Adam (tests/rmline_train_cases.RefModel);
  fit_step_over_torch    this project's time over torch's.
Medians of --iters runs after a warm-up.

    python tools/bench_rmline_train.py [--iters 10] [--batches 64,256,1024] [--no-torch] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import rmline_train_cases as TC  # noqa: E402


def phased_fit_step(model, batch, opts):
    """fit_step's own sequence (RMLineModel.fit_step / RefModel.fit_step) with an event at every phase boundary."""
    nets, marks = (model.generator, model.discriminator), []

    def mark():
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        marks.append(e)
    mark()
    for idx, opt in enumerate(opts):
        for p in nets[1 - idx].parameters():
            p.requires_grad_(False)
        loss = model.training_step(batch, 0, idx)
        mark()
        opt.zero_grad()
        loss.backward()
        mark()
        opt.step()
        mark()
        for p in nets[1 - idx].parameters():
            p.requires_grad_(True)
    return marks


def time_fit(model, batch, opts, iters, warm=3):
    for _ in range(warm):
        phased_fit_step(model, batch, opts)
    torch.cuda.synchronize()
    rows = []
    for _ in range(iters):
        m = phased_fit_step(model, batch, opts)
        torch.cuda.synchronize()
        d = [m[i].elapsed_time(m[i + 1]) for i in range(6)]
        rows.append((m[0].elapsed_time(m[6]), d[0] + d[3], d[1] + d[4], d[2] + d[5]))
    med = [round(statistics.median(r[i] for r in rows), 4) for i in range(4)]
    return dict(zip(("fit_step_ms", "forward_ms", "backward_ms", "optim_ms"), med))


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
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--batches", default="64,256,1024")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rmline_train_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rmline_train needs an MI355X: the HIP path has no CPU fallback")
    import panic3d_amd as P
    P._lib.lib()
    ops, cfg, rows = P.ops, TC.CONFIGS["real"], []
    for B in [int(b) for b in args.batches.split(",")]:
        model = P.RMLineModel(**cfg).cuda().train()
        batch = TC.make_batch(cfg, B, device="cuda")
        opts = model.configure_optimizers()[0]
        row = {"B": B, "patches": [B, 2 * B]}
        row.update(time_fit(model, batch, opts, args.iters))
        before = ops.RMLINE_LAUNCHES[0]
        model.fit_step(batch, opts)
        row["launches"] = ops.RMLINE_LAUNCHES[0] - before
        N, Ci, Co, Hin = 2 * B, cfg["gen_width"], cfg["gen_width"], cfg["size"] + 2 * cfg["gen_depth"] - 2
        x, dz = torch.randn((N, Hin, Hin, Ci), device="cuda"), torch.randn((N, Hin - 2, Hin - 2, Co), device="cuda")
        wk, bias = torch.randn((9, Ci, Co), device="cuda") * 0.1, torch.zeros(Co, device="cuda")
        flop = 2 * 9 * Ci * Co * (Hin - 2) ** 2 * N
        kern = {"forward": lambda: ops.rmline_conv(x, wk, bias, "leaky", 0.01, per_tap=True), "dgrad": lambda: ops.rmline_conv_dgrad(dz, wk, a=x, slope=0.01),
                "wgrad": lambda: ops.rmline_conv_wgrad(x, dz)}
        row["kernels"] = {}
        for name, fn in kern.items():
            ms = ev_ms(fn, max(args.iters // 2, 3))
            row["kernels"][name] = {"ms": round(ms, 4), "tflops": round(flop / ms / 1e9, 2)}
        row["kernels"]["slices"] = ops.rmline_wgrad_plan(N, Ci, Co)["slices"]
        del x, dz
        if not args.no_torch:
            ref = TC.ref_like(model, dtype=torch.float32, device="cuda")
            ropts = [torch.optim.Adam(ref.generator.parameters(), lr=ref.lr_gen), torch.optim.Adam(ref.discriminator.parameters(), lr=ref.lr_dis)]
            t = time_fit(ref, batch, ropts, args.iters)
            row.update({"torch_fp32_" + k: v for k, v in t.items()})
            row["fit_step_over_torch"] = round(row["fit_step_ms"] / t["fit_step_ms"], 3)
        rows.append(row)
        del model, batch
        torch.cuda.empty_cache()
    line = json.dumps({"bench": "rmline_train", "network": "generator 6 x conv3x3 (4-32-32-32-32-32-3), discriminator 4 x conv3x3 (4-16-16-16-16), "
                       "21 x 21 patches, patch_size 9, binary32", "rows": rows})
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
