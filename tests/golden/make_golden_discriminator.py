#!/usr/bin/env python3
"""Golden vectors for the dual discriminator, produced by the REFERENCE ITSELF on CPU (its source tree imported unmodified from the
directory P3D_REFERENCE_DIR names).  Writes only arrays and names: tests/golden/discriminator.npz.

    P3D_REFERENCE_DIR=<checkout of the reference> python tests/golden/make_golden_discriminator.py

The reference's DualDiscriminator (training/dual_discriminator.py) on the small network of tests/discriminator_cases.py (D_KW: 32^2,
3 + 3 image channels, at most 48 channels, c_dim 25, cond_mode resnetcond_8, conv_clamp 256, mbstd group 2), batch 4 = two groups,
inputs scaled so that fromrgb's outputs reach the clamp.  Parameters, inputs and the cotangent are re-drawn by the tests from the same
seeds; the fixture stores the logits, the gradient of sum(logits * g) with respect to image, image_raw and every parameter (large
weights as every 2nd output and input channel, next to their full L2 norm), a checksum of what was re-drawn, and the reference's
state_dict names and shapes (also for freeze_layers = 2)."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("P3D_REFERENCE_DIR")
if not REF:
    sys.exit("set P3D_REFERENCE_DIR to a checkout of the reference")
os.environ.setdefault("PROJECT_DN", REF)
os.environ.setdefault("PROJECT_NAME", "x")
sys.path[:0] = [REF]
sys.path.append(os.path.join(REF, "_train", "eg3dc", "src"))
sys.path.append(os.path.dirname(HERE))  # tests/: the case definitions the tests share with this script

import numpy as np  # noqa: E402
import torch  # noqa: E402

import discriminator_cases as DC  # noqa: E402


def main():
    from training.dual_discriminator import DualDiscriminator
    D = DC.fill_discriminator(DualDiscriminator(**DC.D_KW))
    inp = DC.discriminator_inputs()
    image, raw = (inp[k].clone().requires_grad_(True) for k in ("image", "image_raw"))
    logits = D({"image": image, "image_raw": raw}, inp["c"], {"resnet_feats": inp["feats"]})
    (logits * inp["g"]).sum().backward()
    out = {"logits": logits.detach().numpy(), "g_image": image.grad.numpy(), "g_image_raw": raw.grad.numpy(),
           "checksum": np.float64(DC.checksum(D, inp))}
    for n, q in D.named_parameters():
        out["g_" + DC.key(n)] = DC.dsub(q.grad).numpy()
        out["n_" + DC.key(n)] = np.float64(q.grad.double().norm())
    sd = D.state_dict()
    out["state_names"] = np.array(list(sd.keys()))
    out["state_shapes"] = np.array([",".join(str(d) for d in v.shape) for v in sd.values()])
    Df = DualDiscriminator(**dict(DC.D_KW, block_kwargs={"freeze_layers": 2}))
    out["frozen2_parameters"] = np.array([n for n, _ in Df.named_parameters()])
    path = os.path.join(HERE, "discriminator.npz")
    np.savez_compressed(path, **out)
    print(f"discriminator.npz: {os.path.getsize(path) / 1024:.0f} KiB; logits {logits.detach().flatten().tolist()}")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
