#!/usr/bin/env python3
"""Golden gradients of the StyleGAN2 synthesis network, produced by the REFERENCE ITSELF on CPU (fp32 autograd; the reference
imported unmodified, as make_golden_synthesis.py does; only runs in the build container).  Output: tests/golden/syn_grad_*.npz.

The generators are the ones of syn_generator_none.npz / syn_generator_cond.npz (weights, ws and conditioning images are read from
those fixtures).  Per case: latent injections (da_0, db_1); the unconditioned case with stop_level = 2, the conditioned one
through every level (every edit of the conditioning glue reaches the loss); constant noise; the loss is
sum(out * g_out) with a seeded cotangent g_out.  Recorded: g_out, the injections, and the gradient of ws, of every synthesis
parameter and of the conditioning tensors that enter the synthesis network.

    python tests/golden/make_golden_synthesis_grad.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_synthesis as MG  # noqa: E402  (sets up the reference's import path)

import numpy as np  # noqa: E402
import torch  # noqa: E402

CASES = (("none", 2), ("cond", None))
COND_GRAD = ("image_ortho_front", "resnet_chonk")  # the conditioning tensors the synthesis network reads


def thin(t):
    """Every THIN-th element of the flattened gradient for tensors of more than 4096 elements (the whole tensor otherwise): the test
    compares the same elements."""
    a = t.detach().reshape(-1).numpy()
    return a[::THIN].copy() if a.size > 4096 else t.detach().numpy()


THIN = 3


def grad_case(tag, stop_level):
    torch.set_grad_enabled(True)
    cond_mode = dict(MG.COND_MODES)[tag]
    g = dict(np.load(os.path.join(HERE, f"syn_generator_{tag}.npz")))
    G = MG.ns.Generator(cond_mode=cond_mode, **MG.GEN_KW).eval()
    G.load_state_dict({k[3:].replace("__", "."): torch.from_numpy(v) for k, v in g.items() if k.startswith("sd_")}, strict=True)
    cond = {k[5:]: torch.from_numpy(v).clone() for k, v in g.items() if k.startswith("cond_") and k != "cond_mode"}
    for k in COND_GRAD:
        cond[k].requires_grad_(True)
    ws = torch.from_numpy(g["ws"]).clone().requires_grad_(True)
    gg = torch.Generator().manual_seed(93)
    with torch.no_grad():
        _, loc = G.synthesis(ws, cond, noise_mode="const", return_more=True)
    inj = {}
    for lvl, (x, img) in enumerate(loc["ximgs"]):
        if lvl == 0:
            inj[f"da_{lvl}"] = (torch.randn(x.shape, generator=gg) * 0.3).requires_grad_(True)
        if lvl == 1:
            inj[f"db_{lvl}"] = (torch.randn(img.shape, generator=gg) * 0.3).requires_grad_(True)
    out = G.synthesis(ws, cond, latent_injection=inj, stop_level=stop_level, noise_mode="const")
    g_out = torch.randn(out.shape, generator=gg)
    (out * g_out).sum().backward()
    rec = {"g_ws": ws.grad.numpy(), "stop_level": np.array(-1 if stop_level is None else stop_level),
           "draw_checksum": np.array([float(g_out.double().sum() + sum(v.detach().double().sum() for v in inj.values()))]),
           "out_sub": out.detach()[:, ::8, ::4, ::4].contiguous().numpy()}
    for k, v in inj.items():
        if v.grad is not None:  # (an injection after the stop level does not reach the output)
            rec["g_inj_" + k] = v.grad.numpy()
    for k in COND_GRAD:
        if cond[k].grad is not None:
            rec["g_cond_" + k] = cond[k].grad.numpy()
    for n, p in G.synthesis.named_parameters():
        if p.grad is not None:  # (the blocks after a stop level do not reach the output)
            rec["g_" + n.replace(".", "__")] = thin(p.grad)
    MG.save(f"syn_grad_{tag}.npz", **rec)


if __name__ == "__main__":
    torch.set_num_threads(8)
    for tag, sl in CASES:
        grad_case(tag, sl)
