#!/usr/bin/env python3
"""The bits of the forward modulated convolution, case by case: for comparing two builds of the library.

    python tools/modconv_bits.py > bits.txt

Runs every case of tests/modconv_cases.py through ops.modulated_conv2d — inputs from modconv_ref.make_inputs, under the case's
environment switches, the call of tests/test_hip_modconv_edges.py::_call — and prints one line per case: the case id and the
SHA-256 of the bytes of each output it returns (y, ActImage.data, ToRGB partials; "-" where the case has none).  Two builds that
compute the same print byte-identical files (profiles/r09_modconv_bits_*.txt)."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402
import panic3d_amd as P  # noqa: E402
import modconv_cases as MC  # noqa: E402
import modconv_ref as R  # noqa: E402
import test_hip_modconv_edges as E  # noqa: E402

# Private names this tool leans on (a rename fails loudly here, with an AttributeError / ImportError, not silently): the memoised shape
# queries of ops that an environment switch could change (the list of tests/test_hip_modconv_edges.py's `watched` fixture), ops._ACTS,
# and SWITCHES, DEV, _dev, _weights_f16, _call of that test module
SHAPE_MEMOS = ("_WSB", "_WLAYOUT", "_TAKES_IMAGE", "_FUSES_TORGB")


def sha(t):
    return "-" if t is None else hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def main():
    ops = P.ops
    P._lib.lib()
    lrelu = ops._ACTS["lrelu"]
    for c in MC.CASES:
        for k in E.SWITCHES:
            os.environ.pop(k, None)
        for k, v in c.sw.items():
            os.environ[k] = str(v)
        for name in SHAPE_MEMOS:
            getattr(ops, name).clear()
        ops._ACTS["lrelu"] = (lrelu[0], c.alpha, lrelu[2]) if c.act == "lrelu" else lrelu
        d = E._dev(R.make_inputs(c))
        flag = ops.conv_domain_flag(torch.device(E.DEV))
        lib = ops.conv_weight_layout(c.I, c.O, c.W, c.up) if (c.mma == "x2" and c.ks == 3) else 0
        with torch.no_grad():
            y, img, part = E._call(ops, c, d, E._weights_f16(ops, c, d, lib if c.layout == "lib" else 0), flag)
            torch.cuda.synchronize()
        print(c.id, sha(y), sha(None if img is None else img.data), sha(part), flush=True)
    ops._ACTS["lrelu"] = lrelu


if __name__ == "__main__":
    main()
