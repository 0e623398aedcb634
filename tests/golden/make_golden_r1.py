#!/usr/bin/env python3
"""Golden vectors for the R1 penalty, produced by the REFERENCE ITSELF on CPU (its source tree imported unmodified from the directory
P3D_REFERENCE_DIR names).  Writes only arrays and names: tests/golden/r1.npz.

    P3D_REFERENCE_DIR=<checkout of the reference> python tests/golden/make_golden_r1.py

Network level: the reference's DualDiscriminator on the small network of tests/discriminator_cases.py (D_KW, DC's seeds) runs
loss_orthocondA.py:707-738's Dreg (tests/r1_cases.py: run_module) at the two image scales of r1_cases.SCALES, inside its own
conv2d_gradfix.no_weight_gradients().  Stored per scale: the penalty, both image gradients, the gradient of (penalty * GAMMA / 2).mean()
* GAIN for every parameter that received one (large weights as every 2nd output and input channel, next to their full L2 norm) and the
names of those parameters.  Loss level: the reference's StyleGAN2LossOrthoCondA on the stand-ins of tests/loss_cases.py for the cases
of r1_cases.PHASE_CASES: every reported value and every leaf gradient, as make_golden_loss.py stores the other phases."""
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("P3D_REFERENCE_DIR")
if not REF:
    sys.exit("set P3D_REFERENCE_DIR to a checkout of the reference")
os.environ.setdefault("PROJECT_DN", REF)
os.environ.setdefault("PROJECT_NAME", "x")
sys.path[:0] = [REF]
sys.path.append(os.path.join(REF, "_train", "eg3dc", "src"))
sys.path.append(os.path.dirname(HERE))  # tests/: the case definitions the tests share with this script
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))  # the package (loss.erosion / loss.dilation, as make_golden_loss.py)
sys.modules.setdefault("kornia", types.ModuleType("kornia"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import discriminator_cases as DC  # noqa: E402
import loss_cases as LC  # noqa: E402
import r1_cases as RC  # noqa: E402


def main():
    import kornia
    import panic3d_amd.loss as my_loss
    kornia.morphology = types.SimpleNamespace(erosion=lambda x, kernel: my_loss.erosion(x, kernel.shape[0]),
                                              dilation=lambda x, kernel: my_loss.dilation(x, kernel.shape[0]))
    from torch_utils import training_stats
    from torch_utils.ops import conv2d_gradfix
    from training import loss_orthocondA as ref
    from training.dual_discriminator import DualDiscriminator
    out = {}
    D = DC.fill_discriminator(DualDiscriminator(**DC.D_KW))
    for tag, scale in RC.SCALES.items():
        r = RC.run_module(D, RC.r1_inputs(scale), guard=conv2d_gradfix.no_weight_gradients())
        out[f"{tag}|penalty"], out[f"{tag}|g_image"], out[f"{tag}|g_raw"] = r["penalty"].numpy(), r["g_image"].numpy(), r["g_raw"].numpy()
        out[f"{tag}|names"] = np.array(sorted(r["grads"]))
        for n, g in r["grads"].items():
            out[f"{tag}|g|{n}"] = DC.dsub(g).numpy()
            out[f"{tag}|n|{n}"] = np.float64(g.double().norm())
        zero = [n for n, g in r["grads"].items() if not g.any()]
        missing = sorted(set(n for n, _ in D.named_parameters()) - set(r["grads"]))
        print(f"{tag}: penalty {r['penalty'].tolist()}; zero gradients {zero}; none {missing}")

    def capture(hook):
        training_stats.report = hook
    for name, case in RC.PHASE_CASES.items():
        reports, grads = LC.run_phase(ref.StyleGAN2LossOrthoCondA, case, capture)
        for k, v in reports.items():
            out[LC.fixture_key(name, "report", k)] = v.numpy()
        for k, v in grads.items():
            out[LC.fixture_key(name, "grad", k)] = v.numpy()
        print(f"{name}: reports {sorted(reports)}, gradients of {sorted(grads)}")
    path = os.path.join(HERE, "r1.npz")
    np.savez_compressed(path, **out)
    print(f"r1.npz: {os.path.getsize(path) / 1024:.0f} KiB, {len(out)} arrays")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    torch.set_num_threads(8)
    main()
