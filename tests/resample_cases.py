"""Cases, reference and gate shared by the tests of the generic resampler (k_upfirdn2d, csrc/p3d_fir.hip; ops.upfirdn2d / ops.fir and
their adjoint ops._upfirdn2d_adjoint): tests/test_resample_cases_cpu.py, tests/test_hip_resample_edges.py.  Not collected.

The reference is discriminator_cases.upfirdn2d_torch in float64 (a line-for-line restatement of upfirdn2d.py's _upfirdn2d_ref).  THE GATE
is the project's (tests/synthesis_grad_ref.py): K = fh * fw, absref = the same operator on |x| with |f| (and |gain|).

The filters are not symmetric, so that a missing or doubled flip, a flip in one axis, and swapped x / y padding all change the result:
"asym" = the normalised outer product of (1,2,4,8) and (1,3,5,11), "f3x5" = a normalised 3 x 5 filter without any symmetry; "sym" =
[1,3,3,1] is kept for the production calls."""
import collections

import torch

import discriminator_cases as DC

Case = collections.namedtuple("Case", "id shape filt up down padding flip gain")
CASES = [
    Case("01-pad-1221", (2, 3, 7, 5), "asym", 1, 1, [1, 2, 2, 1], False, 1),
    Case("02-pad-1221-flip", (2, 3, 7, 5), "asym", 1, 1, [1, 2, 2, 1], True, 1),
    Case("03-down2-pad1", (1, 2, 9, 7), "asym", 1, 2, 1, False, 1),
    Case("04-down2-pad-2112", (1, 2, 9, 7), "asym", 1, 2, [2, 1, 1, 2], False, 1),
    Case("05-up2-gain4", (2, 1, 5, 6), "asym", 2, 1, [2, 1, 2, 1], False, 4),
    Case("06-3x5-up2-down2", (1, 3, 6, 5), "f3x5", 2, 2, [3, 0, 1, 2], False, 1),
    Case("07-3x5-up3-down3", (1, 1, 4, 5), "f3x5", 3, 3, [2, 2, 1, 1], False, 1),
    Case("08-down2-crop", (1, 2, 10, 9), "asym", 1, 2, [-1, 0, 0, -1], False, 1),
    Case("09-down2-flip-resizing", (1, 2, 10, 9), "asym", 1, 2, 0, True, 1),
    Case("10-one-pixel-up2", (1, 1, 1, 1), "asym", 2, 1, [2, 1, 2, 1], False, 1),
    Case("11-one-output", (1, 1, 2, 2), "asym", 1, 1, 1, False, 1),
    Case("12-3x5-down3", (1, 1, 9, 8), "f3x5", 1, 3, [0, 1, 2, 0], False, 1),
    Case("13-up2-down3", (1, 2, 6, 7), "asym", 2, 3, [1, 2, 0, 3], False, 1),
    Case("14-up2-crop", (1, 1, 8, 8), "asym", 2, 1, [-1, 2, 2, -1], False, 1),
    Case("15-two-blocks", (3, 2, 11, 9), "f3x5", 1, 1, [1, 0, 2, 1], True, 2),   # 6 x 12 x 6 = 432 outputs: two blocks of 256, the second partial
    Case("16-sym-down2", (2, 3, 8, 8), "sym", 1, 2, 1, False, 1),                 # the discriminator's down-sampling call
    Case("17-sym-pad2", (2, 3, 8, 8), "sym", 1, 1, 2, False, 1),
]
CASE_IDS = [c.id for c in CASES]
BY_ID = {c.id: c for c in CASES}


def make_filter(name):
    if name == "sym":
        f = torch.tensor([1.0, 3.0, 3.0, 1.0]).ger(torch.tensor([1.0, 3.0, 3.0, 1.0]))
    elif name == "asym":
        f = torch.tensor([1.0, 2.0, 4.0, 8.0]).ger(torch.tensor([1.0, 3.0, 5.0, 11.0]))
    else:
        f = torch.tensor([[1.0, 4.0, 2.0, 7.0, 3.0], [5.0, 1.0, 9.0, 2.0, 6.0], [2.0, 8.0, 3.0, 1.0, 4.0]])
    return f / f.sum()


def make_inputs(c, _memo={}):
    """(x, f, g): the input, the filter and a cotangent of the output's shape, fp32, seeded by the case; shared, never modified."""
    if c.id not in _memo:
        gen = torch.Generator().manual_seed(1000 + CASES.index(c) if c in CASES else 999)
        x, f = torch.randn(*c.shape, generator=gen), make_filter(c.filt)
        oh, ow = out_hw(c)
        _memo[c.id] = (x, f, torch.randn(c.shape[0], c.shape[1], oh, ow, generator=gen))
    return _memo[c.id]


def out_hw(c):
    px0, px1, py0, py1 = DC._pad4(c.padding)
    fh, fw = make_filter(c.filt).shape
    return (c.shape[2] * c.up + py0 + py1 - fh) // c.down + 1, (c.shape[3] * c.up + px0 + px1 - fw) // c.down + 1


def kwargs(c):
    return dict(up=c.up, down=c.down, padding=c.padding, flip_filter=c.flip, gain=c.gain)


def case_ref(c, _memo={}):
    """dict(y, absref, gx, gx_absref, K): the float64 forward and, by float64 autograd, the gradient of sum(y * g) in x, each with the same
    operator on absolute values as the gate's scale (the adjoint of a non-negative operator on |g| is the sum of the |terms|)."""
    if c.id not in _memo:
        x, f, g = make_inputs(c)
        x64 = x.double().requires_grad_(True)
        y = DC.upfirdn2d_torch(x64, f.double(), **kwargs(c))
        gx, = torch.autograd.grad(y, x64, g.double())
        xa = x.double().abs().requires_grad_(True)
        ya = DC.upfirdn2d_torch(xa, f.double().abs(), **dict(kwargs(c), gain=abs(c.gain)))
        gxa, = torch.autograd.grad(ya, xa, g.double().abs())
        _memo[c.id] = dict(y=y.detach(), absref=ya.detach(), gx=gx, gx_absref=gxa, K=f.numel())
    return _memo[c.id]


# ---- seeded faults on the binary32 arithmetic (no kernel involved) -------------------------------------------------------------------------
FAULTS = ("no_flip", "flip_one_axis", "pad_xy_swapped", "adjoint_up_down_swapped", "tap_off_by_one", "gain_dropped")
FAULT_CASE = {"no_flip": "03-down2-pad1", "flip_one_axis": "06-3x5-up2-down2", "pad_xy_swapped": "04-down2-pad-2112",
              "adjoint_up_down_swapped": "13-up2-down3", "tap_off_by_one": "12-3x5-down3", "gain_dropped": "05-up2-gain4"}


def forward_f32(c, fault=None):
    """upfirdn2d_torch in binary32 with one seeded fault (or none).  Faults that change the output's shape are compared on the overlap."""
    x, f, _ = make_inputs(c)
    kw = kwargs(c)
    if fault == "no_flip":
        kw["flip_filter"] = not c.flip
    elif fault == "flip_one_axis":
        f, kw["flip_filter"] = f.flip([1]), c.flip
    elif fault == "pad_xy_swapped":
        px0, px1, py0, py1 = DC._pad4(c.padding)
        kw["padding"] = [py0, py1, px0, px1]
    elif fault == "tap_off_by_one":
        px0, px1, py0, py1 = DC._pad4(c.padding)
        kw["padding"] = [px0 + 1, px1 - 1, py0, py1]
    elif fault == "gain_dropped":
        kw["gain"] = 1
    return DC.upfirdn2d_torch(x, f, **kw)


def adjoint_f32(ops, c, fault=None):
    """ops._upfirdn2d_adjoint on binary32 CPU tensors (ops.upfirdn2d replaced by the stand-in), with one seeded fault or none."""
    x, f, g = make_inputs(c)
    up, down = (c.down, c.up) if fault == "adjoint_up_down_swapped" else (c.up, c.down)
    return ops._upfirdn2d_adjoint(g, f, up, down, c.padding, c.flip, c.gain, tuple(c.shape[2:]))


def overlap(a, b):
    """a cropped to b's extent where a fault changed the shape (and zero-filled where it is smaller)."""
    out = torch.zeros(b.shape, dtype=a.dtype)
    h, w = min(a.shape[2], b.shape[2]), min(a.shape[3], b.shape[3])
    out[:, :, :h, :w] = a[:, :, :h, :w]
    return out
