#!/usr/bin/env python3
"""Golden vectors for the training loss, produced by the REFERENCE ITSELF on CPU (its source tree imported unmodified from the
directory P3D_REFERENCE_DIR names).  Writes only arrays: tests/golden/loss_phases.npz.

    P3D_REFERENCE_DIR=<checkout of the reference> python tests/golden/make_golden_loss.py

The reference's StyleGAN2LossOrthoCondA runs every case of tests/loss_cases.py (PHASE_CASES) on the stand-in G, D and lpips_model
defined there; the fixture stores every value it reports through training_stats.report and the gradient of every stand-in leaf,
plus mask_view_orthofront's result on the cases' condition.

kornia is not installed where this runs: `kornia.morphology.erosion` / `dilation` are stood in by this package's loss.erosion /
loss.dilation (kornia 0.6.5 semantics), as make_golden_train_step.py stands in the Sobel filter, so loss_phases.npz pins the loss's
own arithmetic and phase rules, not kornia.
"""
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
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))  # the package (loss.erosion / loss.dilation)
sys.modules.setdefault("kornia", types.ModuleType("kornia"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import loss_cases as LC  # noqa: E402


def main():
    import kornia
    import panic3d_amd.loss as my_loss
    kornia.morphology = types.SimpleNamespace(erosion=lambda x, kernel: my_loss.erosion(x, kernel.shape[0]),
                                              dilation=lambda x, kernel: my_loss.dilation(x, kernel.shape[0]))
    from torch_utils import training_stats
    from training import loss_orthocondA as ref

    def capture(hook):
        training_stats.report = hook

    arrs = {}
    for name, case in LC.PHASE_CASES.items():
        reports, grads = LC.run_phase(ref.StyleGAN2LossOrthoCondA, case, capture)
        for k, v in reports.items():
            arrs[LC.fixture_key(name, "report", k)] = v.numpy()
        for k, v in grads.items():
            arrs[LC.fixture_key(name, "grad", k)] = v.numpy()
        print(f"{name}: {len(reports)} reports, gradients of {sorted(grads)}")
    cond = LC.loss_inputs()["real_cond"]
    lmask = ref.mask_view_orthofront(cond["image_ortho_front_xyz"], cond["image_ortho_front_alpha"], cond["image_xyz"], cond["image_alpha"],
                                     LC.BOX_WARP)
    print("lmask mean %.3f" % float(lmask.mean()))
    arrs["lmask"] = lmask.numpy()
    path = os.path.join(HERE, "loss_phases.npz")
    np.savez_compressed(path, **arrs)
    print(f"loss_phases.npz: {os.path.getsize(path) / 1024:.0f} KiB, {len(arrs)} arrays")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    torch.set_num_threads(8)
    main()
