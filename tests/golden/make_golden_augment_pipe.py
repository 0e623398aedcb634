#!/usr/bin/env python3
"""Golden vectors for the augmentation pipe's module, produced by the REFERENCE ITSELF on CPU (its source tree imported unmodified from
the directory P3D_REFERENCE_DIR names).  Writes only arrays: tests/golden/augment_pipe_module.npz.

    P3D_REFERENCE_DIR=<checkout of the reference> python tests/golden/make_golden_augment_pipe.py

  * Hz_fbank, the reference's filter-bank buffer;
  * the tail family (tests/augment_pipe_cases.py: TAIL_PIPES, each on its TAIL_SHAPES entry, at TAIL_PERCENTILES): the output and the
    input gradient of a fixed cotangent, with what the reference itself computed for that run: the filter rows it hands to its first
    convolution, and for the pipe with geometry the theta it hands to F.affine_grid, the margins it hands to F.pad and its colour rows
    (make_golden_augment.colour_rows).  The calls are observed, not changed;
  * random mode: AugmentPipe(**RANDOM_PIPE) with p in RANDOM_P after torch.manual_seed(s), s in RANDOM_SEEDS, on RANDOM_SHAPES: the
    output, theta and margins.  This package's AugmentPipe.draw runs under the same seed and its margins are asserted equal.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("P3D_REFERENCE_DIR")
if not REF:
    sys.exit("set P3D_REFERENCE_DIR to a checkout of the reference")
sys.path.append(os.path.join(REF, "_train", "eg3dc", "src"))
sys.path.append(os.path.dirname(HERE))                   # tests/: the case definitions
sys.path.append(HERE)                                    # make_golden_augment.colour_rows
sys.path.append(os.path.dirname(os.path.dirname(HERE)))  # the package, for the margins' cross-check

import augment_cases as AC  # noqa: E402
import augment_pipe_cases as PC  # noqa: E402
from make_golden_augment import colour_rows  # noqa: E402
from training.augment import AugmentPipe  # noqa: E402


def observed(pipe, x, g, q):
    """One run with F.pad, F.affine_grid and F.conv2d observed: (output, input gradient or None, seen)."""
    F = torch.nn.functional
    pad, grid, conv, seen = F.pad, F.affine_grid, F.conv2d, {"pads": []}

    def see_pad(*a, **kw):
        if kw.get("mode") == "reflect":
            seen["pads"].append([int(v) for v in (kw["pad"] if "pad" in kw else a[1])])
        return pad(*a, **kw)

    def see_grid(*a, **kw):
        seen.setdefault("theta", (kw["theta"] if "theta" in kw else a[0]).detach().numpy().copy())
        return grid(*a, **kw)

    def see_conv(*a, **kw):
        w = kw["weight"] if "weight" in kw else a[1]
        if w.shape[2] == 1 and w.shape[3] == 43:  # the filter's row pass: [N * C, 1, 1, taps]
            seen.setdefault("weight", w.detach().numpy().copy())
        return conv(*a, **kw)
    F.pad, F.affine_grid, F.conv2d = see_pad, see_grid, see_conv
    try:
        x = torch.from_numpy(x).requires_grad_(g is not None)
        y = pipe(x, debug_percentile=q)
        gx = torch.autograd.grad(y, x, torch.from_numpy(g))[0].numpy() if g is not None else None
    finally:
        F.pad, F.affine_grid, F.conv2d = pad, grid, conv
    if "theta" in seen:
        mx0, mx1, my0, my1 = seen["pads"][0]
        seen["margins"] = np.array([mx0, my0, mx1, my1], dtype=np.int32)
    return y.detach().numpy(), gx, seen


def main():
    import panic3d_amd
    out = {"Hz_fbank": AugmentPipe().Hz_fbank.numpy()}
    for pi, (kwargs, shape) in enumerate(zip(PC.TAIL_PIPES, PC.TAIL_SHAPES)):
        pipe = AugmentPipe(**kwargs)
        x, g = PC.tail_inputs(pi)
        for q in PC.TAIL_PERCENTILES:
            y, gx, seen = observed(pipe, x, g, q)
            out[PC.tail_key("out", pi, q)], out[PC.tail_key("grad", pi, q)] = y, gx
            out[PC.tail_key("taps", pi, q)] = seen["weight"][::shape[1], 0, 0, :]
            if "theta" in seen:
                out[PC.tail_key("theta", pi, q)], out[PC.tail_key("margins", pi, q)] = seen["theta"], seen["margins"]
                out[PC.tail_key("colour", pi, q)] = colour_rows(shape[1], q)
    ref, mine = AugmentPipe(**PC.RANDOM_PIPE), panic3d_amd.AugmentPipe(**PC.RANDOM_PIPE)
    for si, shape in enumerate(PC.RANDOM_SHAPES):
        x = PC.random_inputs(si)
        for p in PC.RANDOM_P:
            ref.p.copy_(torch.as_tensor(p))
            mine.p.copy_(torch.as_tensor(p))
            for seed in PC.RANDOM_SEEDS:
                torch.manual_seed(seed)
                y, _, seen = observed(ref, x, None, None)
                torch.manual_seed(seed)
                y2, _, _ = observed(ref, x, None, None)
                assert np.array_equal(y, y2), "the reference's seeded CPU run repeats to the bit"
                torch.manual_seed(seed)
                d = mine.draw(*shape)
                assert d.margins == tuple(int(v) for v in seen["margins"]), (si, p, seed, d.margins, seen["margins"])
                out[PC.random_key("out", si, p, seed)], out[PC.random_key("theta", si, p, seed)] = y, seen["theta"]
                out[PC.random_key("margins", si, p, seed)] = seen["margins"]
    np.savez_compressed(PC.GOLDEN, **out)
    print("wrote", PC.GOLDEN, os.path.getsize(PC.GOLDEN), "bytes,", len(out), "arrays")
    assert os.path.getsize(PC.GOLDEN) < (1 << 20)


if __name__ == "__main__":
    main()
