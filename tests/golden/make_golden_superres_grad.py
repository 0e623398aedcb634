#!/usr/bin/env python3
"""Golden gradients of the 512^2 super-resolution (SuperresolutionHybrid8XDC, 256 hidden channels), produced by the REFERENCE ITSELF
on CPU (fp32 autograd; the reference imported unmodified, as make_golden_synthesis.py does; only runs in the build container).
Output: tests/golden/sr_grad.npz.

The case is tests/superres_grad_cases.py's: sr_num_fp16_res = 4 (the clamp 256 is live; ToRGB biases of +-255 make it clip on both
sides), deterministic parameters, seeded rgb / feature image / ws, constant noise, loss sum(image * g_out) with a seeded cotangent.
Recorded: the gradients of rgb, the feature image, ws and every parameter (thinned: superres_grad_cases.thin), a sub-sample
of the image and the draws' checksum.

    python tests/golden/make_golden_superres_grad.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]
import make_golden_synthesis as MG  # noqa: E402  (sets up the reference's import path)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import superres_grad_cases as SRC  # noqa: E402
from training.superresolution import SuperresolutionHybrid8XDC  # noqa: E402


def main():
    torch.set_grad_enabled(True)
    sr = SRC.fill(SuperresolutionHybrid8XDC(**SRC.SR_KW).eval())
    rgb, x, ws, g_out, chk = SRC.draws()
    for t in (rgb, x, ws):
        t.requires_grad_(True)
    out = sr(rgb, x, ws, noise_mode="const")
    clipped = float((out.detach().abs() >= 255.0).double().mean())
    print(f"image {tuple(out.shape)}, fraction beyond the clamp region: {clipped:.3f}")
    (out * g_out).sum().backward()
    rec = {"g_rgb": SRC.thin(rgb.grad.numpy()), "g_x": SRC.thin(x.grad.numpy()), "g_ws": ws.grad.numpy(),
           "draw_checksum": np.array([chk]), "out_sub": out.detach()[:, :, ::8, ::8].contiguous().numpy()}
    for n, p in sr.named_parameters():
        rec["g_" + n.replace(".", "__")] = SRC.thin(p.grad.numpy())
    MG.save("sr_grad.npz", **rec)


if __name__ == "__main__":
    torch.set_num_threads(16)
    main()
