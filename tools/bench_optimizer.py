#!/usr/bin/env python3
"""Timing of the optimiser step (panic3d_amd/optim.py, include/p3d_optim.h) at the trainer's size: the full-width
generator (tests/p3d_testing.FULL_KW with the seeded parameters of fill_generator_params: 30 M parameters) and the trainer's
DualDiscriminator; prints one JSON line and writes it to profiles/optimizer_bench.json.

Compared, in one process, alternating window by window, after a warm-up, with HIP events around --calls back-to-back calls and the
median over --repeats windows:

  torch   the reference's composition (training_loop_v0.py:364-375, :387-390): torch.cat of the gradients, nan_to_num, split, the
          gradients re-pointed into the flat vector, torch.optim.Adam (its default, the foreach form) .step(), and for the G step
          with EMA the loop p_ema.copy_(p.lerp(p_ema, beta)) over the parameters and b_ema.copy_(b) over the buffers;
  kernel_only   p3d_optim_step_f32 alone on the uploaded tables: the device time, without the host's per-tensor work;
  ours    optim.phase_step: one launch; with EMA the lerp of the parameters rides in that launch and the buffers take one more
          (EMA-only, weight 0); `ours_two_launches` is the drop-in form phase_step() + update_ema().

Per row: the times, ours / torch, the launch counts of one call (device kernels and copies as torch.profiler sees them; "not measured"
where the profiler gives nothing), and the algorithmic bytes from the shapes (4 B x numel x streams: g, v, p read and m, v, p written
with beta1 = 0; + e read and written with the EMA) over the time, beside the 6.29 TB/s measured streaming rate and the 8 TB/s peak of
the MI355X.  No ratio is asserted: `fused_is_faster` records the condition (ours < torch for the G step with EMA and for the D step).

    python tools/bench_optimizer.py [--repeats 7] [--calls 10] [--out FILE] [--small]
"""
import argparse
import copy
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

BETA, LR, BETAS, EPS = 0.99778, 0.002 * 16 / 17, (0.0, 0.99 ** (16 / 17)), 1e-8
STREAM_TBS, PEAK_TBS = 6.29, 8.0


def window_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def compare(fns, repeats, calls):
    for fn in fns.values():  # warm-up: code objects, the allocator, the optimiser's state and table
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(repeats):  # alternating, so that a disturbance from outside meets every form
        for k, fn in fns.items():
            t[k].append(window_ms(fn, calls))
    return {k: {"ms": round(statistics.median(v), 4), "min_max_ms": [round(min(v), 4), round(max(v), 4)]} for k, v in t.items()}


def launches(fn):
    """Device kernels and device copies of one call, or 'not measured'."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
        return n if n > 0 else "not measured"
    except Exception as e:  # the profiler is an aid, not the subject
        return f"not measured ({type(e).__name__})"


def kernel_only(P, table, mode):
    """The launch alone, from the table and the per-step entries an optimiser left on the device: the device time of a step."""
    import ctypes as C
    L = P._lib.lib()
    a = P._lib.OptimArgs(tensors=table.tensors.data_ptr(), steps=table.steps.data_ptr(), chunks=table.chunks.data_ptr(), n_chunks=table.n_chunks,
                         n_tensors=table.n, mode=mode, sanitize=1, grad_scale=1.0, nan_v=0.0, posinf_v=1e5, neginf_v=-1e5, eps=EPS,
                         beta1=BETAS[0], beta2=BETAS[1])
    return lambda: P._lib.check(L.p3d_optim_step_f32(C.byref(a), P.ops._stream()), "p3d_optim_step_f32")


def torch_phase(params, opt):
    flat = torch.cat([p.grad.flatten() for p in params])
    torch.nan_to_num(flat, nan=0, posinf=1e5, neginf=-1e5, out=flat)
    for p, g in zip(params, flat.split([p.numel() for p in params])):
        p.grad = g.reshape(p.shape)
    opt.step()


def torch_ema(G_ema, G, beta):
    with torch.no_grad():
        for p_ema, p in zip(G_ema.parameters(), G.parameters()):
            p_ema.copy_(p.lerp(p_ema, beta))
        for b_ema, b in zip(G_ema.buffers(), G.buffers()):
            b_ema.copy_(b)


def seed_grads(module, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    for p in module.parameters():
        p.grad = torch.randn(p.shape, device="cuda", generator=g) * 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--small", action="store_true", help="the small test networks instead of the trainer's (a dry run of the tool)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optimizer_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_optimizer.py needs a GPU"
    import panic3d_amd as P
    import p3d_shared_cases as MC
    import p3d_testing as T
    from panic3d_amd.generator import TriPlaneGenerator
    P._lib.lib()
    optim, ops = P.optim, P.ops
    if a.small:
        G = MC.memo_generator("cuda")
        D = P.DualDiscriminator(c_dim=25, img_resolution=32, img_channels=3, cond_mode="resnetcond_8", channel_base=1024, channel_max=48).cuda()
    else:
        G = TriPlaneGenerator(**T.FULL_KW).cuda()
        D = P.DualDiscriminator(c_dim=25, img_resolution=512, img_channels=3, cond_mode="resnetcond_8", channel_base=32768, channel_max=512,
                                conv_clamp=256, epilogue_kwargs={"mbstd_group_size": 4}).cuda()
    T.fill_generator_params(G, 3)
    res = {"device": torch.cuda.get_device_name(0), "repeats": a.repeats, "calls_per_window": a.calls, "size": "small" if a.small else "trainer",
           "lr": LR, "betas": BETAS, "ema_beta": BETA, "stream_TBps_measured": STREAM_TBS, "peak_TBps": PEAK_TBS}

    def row(times, numel, streams, counts):
        out = dict(times)
        for k, v in times.items():
            gb = 4.0 * numel * streams / 1e9
            v.update(algorithmic_GB=round(gb, 4), TBps=round(gb / v["ms"], 3), of_stream_rate=round(gb / v["ms"] / STREAM_TBS, 3),
                     launches=counts.get(k))
        for k in times:
            if k != "torch":
                out[k + "_over_torch"] = round(times[k]["ms"] / times["torch"]["ms"], 3)
        return out

    # ---- G: the phase alone, and the phase with the EMA --------------------------------------------------------------------------------
    Gt, Ge, Gte = copy.deepcopy(G), copy.deepcopy(G), copy.deepcopy(G)  # torch's copy, our G_ema, torch's G_ema
    seed_grads(G, 1)
    seed_grads(Gt, 1)
    n_g = sum(p.numel() for p in G.parameters())
    n_b = sum(b.numel() for b in G.buffers())
    res["G"] = {"parameters": n_g, "tensors": len(list(G.parameters())), "buffer_elements": n_b, "buffers": len(list(G.buffers()))}
    ours = optim.Adam(G.parameters(), lr=LR, betas=BETAS, eps=EPS)
    theirs = torch.optim.Adam(Gt.parameters(), lr=LR, betas=BETAS, eps=EPS)
    pt = [p for p in Gt.parameters() if p.numel() > 0]
    fb = [(b, e) for b, e in zip(G.buffers(), Ge.buffers()) if b.dtype == torch.float32 and b.numel() > 0]
    other = [(b, e) for b, e in zip(G.buffers(), Ge.buffers()) if not (b.dtype == torch.float32 and b.numel() > 0)]
    tab = {}

    def ours_fused():
        optim.phase_step(G, ours, ema=(list(Ge.parameters()), BETA))
        if fb:
            tab["b"] = ops.adam_ema_step([b for b, _ in fb], ema_params=[e for _, e in fb], ema_weights=[0.0] * len(fb), table=tab.get("b"))
        for b, e in other:
            e.copy_(b)

    def ours_two():
        optim.phase_step(G, ours)
        optim.update_ema(Ge, G, BETA)

    def torch_with_ema():
        torch_phase(pt, theirs)
        torch_ema(Gte, Gt, BETA)
    optim.phase_step(G, ours)
    fns = {"ours": lambda: optim.phase_step(G, ours), "kernel_only": kernel_only(P, ours._tables[(0, False)], P._lib.P3D_OPTIM_ADAM),
           "torch": lambda: torch_phase(pt, theirs)}
    res["G_step"] = row(compare(fns, a.repeats, a.calls), n_g, 6, {k: launches(f) for k, f in fns.items()})
    ours_fused()
    fns = {"ours": ours_fused, "ours_two_launches": ours_two, "kernel_only": kernel_only(P, ours._tables[(0, True)], P._lib.P3D_OPTIM_ADAM_EMA),
           "torch": torch_with_ema}
    res["G_step_with_ema"] = row(compare(fns, a.repeats, a.calls), n_g, 8, {k: launches(f) for k, f in fns.items()})
    fns = {"ours": lambda: optim.update_ema(Ge, G, BETA), "torch": lambda: torch_ema(Gte, Gt, BETA)}
    res["update_ema"] = row(compare(fns, a.repeats, a.calls), n_g + n_b, 3, {k: launches(f) for k, f in fns.items()})
    del Gt, Ge, Gte, ours, theirs, pt, fb, other
    G.zero_grad(set_to_none=True)

    # ---- D ------------------------------------------------------------------------------------------------------------------------------
    Dt = copy.deepcopy(D)
    seed_grads(D, 2)
    seed_grads(Dt, 2)
    n_d = sum(p.numel() for p in D.parameters())
    res["D"] = {"parameters": n_d, "tensors": len(list(D.parameters()))}
    ours = optim.Adam(D.parameters(), lr=LR, betas=BETAS, eps=EPS)
    theirs = torch.optim.Adam(Dt.parameters(), lr=LR, betas=BETAS, eps=EPS)
    pt = [p for p in Dt.parameters() if p.numel() > 0]
    optim.phase_step(D, ours)
    fns = {"ours": lambda: optim.phase_step(D, ours), "kernel_only": kernel_only(P, ours._tables[(0, False)], P._lib.P3D_OPTIM_ADAM),
           "torch": lambda: torch_phase(pt, theirs)}
    res["D_step"] = row(compare(fns, a.repeats, a.calls), n_d, 6, {k: launches(f) for k, f in fns.items()})

    res["fused_is_faster"] = bool(res["G_step_with_ema"]["ours"]["ms"] < res["G_step_with_ema"]["torch"]["ms"]
                                  and res["D_step"]["ours"]["ms"] < res["D_step"]["torch"]["ms"])
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
