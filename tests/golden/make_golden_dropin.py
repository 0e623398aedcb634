#!/usr/bin/env python3
"""tests/golden/dropin_reference.npz — what the REFERENCE's TriPlaneGenerator records and holds for the two small-width constructions
of tests/test_dropin_reference.py (KWS: unconditioned, conditioned), built from its own source on CPU under torch.manual_seed(0):
the init_args / init_kwargs its persistence decorator records, the name and shape of every parameter and buffer
(misc.named_params_and_buffers order) and the key list of its state_dict, as one JSON string per construction.  BUILD CONTAINER ONLY (imports the reference tree).

    python tests/golden/make_golden_dropin.py
"""
import json
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("P3D_REFERENCE", "/root/reference")
os.environ.setdefault("PROJECT_DN", REF)
os.environ.setdefault("PROJECT_NAME", "x")
sys.path[:0] = [REF, os.path.dirname(HERE)]
sys.path.append(os.path.join(REF, "_train", "eg3dc", "src"))
sys.modules.setdefault("kornia", types.ModuleType("kornia"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import training.triplane as ref_triplane  # noqa: E402
from torch_utils import misc  # noqa: E402
from test_dropin_reference import KWS  # noqa: E402

if __name__ == "__main__":
    out = {}
    for tag, kw in zip(("uncond", "cond"), KWS):
        torch.manual_seed(0)
        G = ref_triplane.TriPlaneGenerator(**kw).eval().requires_grad_(False)
        out[tag] = np.array(json.dumps({"init_args": list(G.init_args), "init_kwargs": G.init_kwargs,
                                        "params_and_buffers": [[n, list(t.shape)] for n, t in misc.named_params_and_buffers(G)],
                                        "state_dict": list(G.state_dict().keys())}))
    path = os.path.join(HERE, "dropin_reference.npz")
    np.savez_compressed(path, torch_version=np.array(torch.__version__), **out)
    print(f"dropin_reference.npz: {os.path.getsize(path) / 1024:.0f} KiB")
