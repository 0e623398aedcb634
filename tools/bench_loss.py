#!/usr/bin/env python3
"""Timing of the training loss's operators (include/p3d_loss.h) at the trainer's size: batch 4, 512^2 images, render
resolution 128, blur sigma 10 (61 taps); prints one JSON line and writes it to profiles/loss_bench.json.

Per operator: the median (and the spread) over --repeats windows of --calls back-to-back calls, timed with HIP events after a warm-up,
ours and the torch-ROCm composition of the same arithmetic on the same GPU, the two alternating window by window:

  blur            ops.blur on the image [4,3,512,512] and on the raw image [4,3,128,128], forward alone and forward + adjoint under
                  autograd; torch: the reference's depthwise F.conv2d pair (tests/loss_cases.blur_torch);
  view_terms      ops.view_terms, forward + backward to weights and xyz; torch: the reference's sequence of launches
                  (tests/loss_cases.view_terms_impl_torch) with autograd;
  l1_mean         ops.l1_mean forward + backward on [4,3,512,512]; torch: (a - b).abs().mean();
  Gcond, Dmain    one accumulate_gradients call of panic3d_amd.loss.StyleGAN2LossOrthoCondA with a stand-in G that returns leaf tensors
                  of the trainer's sizes (the generator's own time is bench.py's subject) and the trainer's DualDiscriminator; torch: the
                  same class with the three operators replaced by the torch compositions above (D stays the HIP one in both).

Where ours/torch > 1 the operator is slower than torch's composition: the ratio is recorded as measured.

    python tools/bench_loss.py [--repeats 7] [--calls 20] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import loss_cases as LC  # noqa: E402

N, S, R, SIGMA = 4, 512, 128, 10.0


def window_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def compare(ours, theirs, repeats, calls):
    for fn in (ours, theirs):  # warm-up: code objects, torch's algorithm choice, the allocator
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = {"ours": [], "torch": []}
    for _ in range(repeats):  # alternating, so that a disturbance from outside meets both
        t["ours"].append(window_ms(ours, calls))
        t["torch"].append(window_ms(theirs, calls))
    med = {k: statistics.median(v) for k, v in t.items()}
    return {"ours_ms": round(med["ours"], 4), "torch_ms": round(med["torch"], 4), "ours_over_torch": round(med["ours"] / med["torch"], 3),
            "ours_min_max_ms": [round(min(t["ours"]), 4), round(max(t["ours"]), 4)],
            "torch_min_max_ms": [round(min(t["torch"]), 4), round(max(t["torch"]), 4)]}


class LeafG(torch.nn.Module):
    """f() returns leaf tensors of the trainer's sizes; mapping returns a constant."""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(1)
        P = torch.nn.Parameter
        self.image, self.image_raw = P(torch.randn(N, 3, S, S, generator=g) * 0.5), P(torch.randn(N, 3, R, R, generator=g) * 0.5)
        self.image_weights, self.image_xyz = P(torch.rand(N, 1, R, R, generator=g)), P(torch.rand(N, 3, R, R, generator=g) - 0.5)
        self.rendering_kwargs, self.cond_mode = dict(box_warp=1.0, density_reg=0.0), "ortho_front.leaf"

    def mapping(self, z, c, cond, **kw):
        return z[:, None, :].repeat(1, 14, 1)

    def f(self, x):
        return {"image": self.image * 1, "image_raw": self.image_raw * 1, "image_weights": self.image_weights * 1, "image_xyz": self.image_xyz * 1}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_loss.py needs a GPU"
    import panic3d_amd as P
    P._lib.lib()
    ops = P.ops
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev)
    res = {"size": {"batch": N, "image": S, "render": R, "sigma": SIGMA, "taps": 61}, "repeats": a.repeats, "calls_per_window": a.calls,
           "device": torch.cuda.get_device_name(0)}
    f = ops.gaussian_filter(SIGMA, dev)

    for name, shape in (("blur_image", (N, 3, S, S)), ("blur_raw", (N, 3, R, R))):
        x, gy = rnd(*shape), rnd(*shape)
        with torch.no_grad():
            err = LC.rel_l2(ops.blur(x, SIGMA), LC.blur_torch(x, f))
            res[name + "_forward"] = dict(compare(lambda: ops.blur(x, SIGMA), lambda: LC.blur_torch(x, f), a.repeats, a.calls), rel_l2_vs_torch=err)
        xg = x.clone().requires_grad_(True)

        def both(fn):
            xg.grad = None
            fn(xg).backward(gy)
        res[name + "_forward_adjoint"] = compare(lambda: both(lambda t: ops.blur(t, SIGMA)), lambda: both(lambda t: LC.blur_torch(t, f)), a.repeats, a.calls)

    gt_alpha, gt_xyz = LC.blob_alpha(N, S, 5).to(dev), rnd(N, 3, S, S) * 0.3
    w, xyz = torch.rand(N, 1, R, R, generator=g).to(dev).requires_grad_(True), (rnd(N, 3, R, R) * 0.3).requires_grad_(True)

    def vt(impl):
        w.grad = xyz.grad = None
        t = impl()
        (t[0] + t[1]).backward()

    def vt_torch():  # (forward and both gradients inside: torch.autograd.grad on its own graph)
        return LC.view_terms_impl_torch(w, xyz, gt_alpha, gt_xyz, "norm", None, True)
    res["view_terms_norm_forward_backward"] = compare(lambda: vt(lambda: ops.view_terms(w, xyz, gt_alpha, gt_xyz, "norm")),
                                                      vt_torch, a.repeats, a.calls)
    x, y = rnd(N, 3, S, S).requires_grad_(True), rnd(N, 3, S, S)

    def l1(fn):
        x.grad = None
        fn().backward()
    res["l1_mean_forward_backward"] = compare(lambda: l1(lambda: ops.l1_mean(x, y)), lambda: l1(lambda: (x - y).abs().mean()), a.repeats, a.calls)

    # the phases: a leaf G, the trainer's discriminator
    D = P.DualDiscriminator(c_dim=25, img_resolution=512, img_channels=3, cond_mode="resnetcond_8", channel_base=32768, channel_max=512,
                            conv_clamp=256, epilogue_kwargs={"mbstd_group_size": 4}).to(dev)
    G = LeafG().to(dev)
    cond = {"resnet_feats": rnd(N, 16), "image_camera": rnd(N, 25)}
    for key in ("image_ortho_front", "image"):
        cond[key], cond[key + "_alpha"], cond[key + "_xyz"] = torch.rand(N, 3, S, S, generator=g).to(dev), LC.blob_alpha(N, S, 7).to(dev), rnd(N, 3, S, S) * 0.3
    cond["image_ortho_front_camera"] = rnd(N, 25)
    inp = dict(real_img=rnd(N, 3, S, S), real_c=rnd(N, 25), real_cond=cond, gen_z=rnd(N, 512), gen_c=rnd(N, 25))
    kw = dict(LC.LAMBDAS, r1_gamma=0, blur_init_sigma=SIGMA, blur_fade_kimg=200, neural_rendering_resolution_initial=R, dual_discrimination=True)
    loss = P.StyleGAN2LossOrthoCondA(device=dev, G=G, D=D, augment_pipe=None, lpips_model=LC.lpips_stand_in, **kw)
    hip = {k: getattr(ops, k) for k in ("_blur_impl", "_l1_impl", "_view_terms_impl")}
    stand = dict(_blur_impl=LC.blur_impl_torch, _l1_impl=LC.l1_impl_torch, _view_terms_impl=LC.view_terms_impl_torch)

    def phase(name, impls):
        for k, v in impls.items():
            setattr(ops, k, v)
        try:
            G.zero_grad(set_to_none=True)
            D.zero_grad(set_to_none=True)
            loss.accumulate_gradients(phase=name, gain=1.0, cur_nimg=0, **inp)
        finally:
            for k, v in hip.items():
                setattr(ops, k, v)
    for name in ("Gcond", "Dmain"):
        res["phase_" + name] = compare(lambda: phase(name, hip), lambda: phase(name, stand), a.repeats, max(a.calls // 4, 2))
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
