"""GPU (-m gpu): the generic resampler k_upfirdn2d (csrc/p3d_fir.hip; ops.upfirdn2d, ops.fir and its adjoint), k_upsample2x_add and
k_bias_act at the small ragged cases of tests/resample_cases.py — asymmetric and non-square filters, up and down together, unequal and
negative padding, flip_filter — against float64 under the project's gate (tests/test_resample_cases_cpu.py shows that binary32 torch
passes it and that six seeded faults fail).  ops.upsample2d_add bit for bit against the generic operator plus a binary32 addition, at
H != W, odd NC, an `add` at a 4-byte storage offset and an odd width; ops.bias_act exact against the binary32 restatement; an input
smaller than its filter is refused with P3D_E_RANGE, nothing written."""
import ctypes as C

import pytest
import torch

import p3d_torch_ops
import resample_cases as RC
from synthesis_grad_ref import gate

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P():
    import panic3d_amd
    panic3d_amd.build()
    panic3d_amd._lib.lib()
    return panic3d_amd


@pytest.mark.parametrize("ci", range(len(RC.CASES)), ids=RC.CASE_IDS)
def test_upfirdn2d_and_its_adjoint_vs_float64(P, ci):
    c = RC.CASES[ci]
    x, f, g = RC.make_inputs(c)
    ref = RC.case_ref(c)
    y = P.ops.upfirdn2d(x.cuda(), f, **RC.kwargs(c))
    assert tuple(y.shape) == tuple(ref["y"].shape)
    gate(f"{c.id} forward", y, ref["y"], ref["absref"], ref["K"])
    grads = []
    for _ in range(2):
        xg = x.cuda().requires_grad_(True)
        yg = P.ops.fir(xg, f, **RC.kwargs(c))
        assert torch.equal(yg.detach(), y)
        yg.backward(g.cuda())
        grads.append(xg.grad)
    assert tuple(grads[0].shape) == tuple(x.shape)
    gate(f"{c.id} adjoint", grads[0], ref["gx"], ref["gx_absref"], ref["K"])
    assert torch.equal(grads[0], grads[1])


@pytest.mark.parametrize("filt", ["sym", "asym"])
@pytest.mark.parametrize("shape", [(1, 3, 1, 2), (1, 5, 5, 6), (3, 1, 5, 10), (1, 3, 1, 10), (7, 1, 5, 2), (1, 3, 5, 3), (2, 2, 4, 7)],
                         ids=lambda s: "x".join(str(v) for v in s))
def test_upsample2d_add_is_the_generic_operator_bit_for_bit(P, shape, filt):
    """W in {2, 6, 10} x H in {1, 5} with an odd NC run k_upsample2x_add; the odd widths (2W % 4 != 0) and the `add` at a 4-byte storage
    offset take the generic operator inside the wrapper."""
    N, Cc, H, W = shape
    gen = torch.Generator().manual_seed(N * 1000 + Cc * 100 + H * 10 + W)
    x = torch.randn(*shape, generator=gen).cuda()
    add = torch.randn(N, Cc, 2 * H, 2 * W, generator=gen).cuda()
    f = RC.make_filter(filt).cuda()
    want = P.ops.upfirdn2d(x, f, up=2, padding=[2, 1, 2, 1], gain=4)
    assert tuple(want.shape) == (N, Cc, 2 * H, 2 * W)
    assert torch.equal(P.ops.upsample2d_add(x, f), want)
    assert torch.equal(P.ops.upsample2d_add(x, f, add), want + add)
    # a contiguous view one float into its storage: not 16-byte aligned
    store = torch.zeros(add.numel() + 1, device="cuda")
    off = store[1:].view_as(add)
    off.copy_(add)
    assert off.is_contiguous() and off.data_ptr() % 16 == 4
    assert torch.equal(P.ops.upsample2d_add(x, f, off), want + add)


def test_upsample2d_add_library_refuses_what_the_wrapper_reroutes(P):
    L = P._lib.lib()
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    x, f = torch.randn(1, 3, 5, 6).cuda(), torch.ones(4, 4, device="cuda")
    store = torch.full((3 * 10 * 12 + 1,), float("nan"), device="cuda")
    y = torch.full((3 * 10 * 12,), float("nan"), device="cuda")
    torch.cuda.synchronize()
    assert L.p3d_upsample2d_add_f32(p(x), 3, 5, 6, p(f), p(store[1:]), p(y), None) == -2  # a misaligned add
    assert L.p3d_upsample2d_add_f32(p(x), 3, 6, 5, p(f), None, p(y), None) == -2  # 2W % 4 != 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all())


@pytest.mark.parametrize("shape,dim,has_b,act,gain,clamp", [
    ((3, 5, 7, 3), 1, True, "lrelu", None, None),       # 315 values: a partial second block
    ((3, 5, 7, 3), 3, True, "linear", 2.0, 1.5),        # the last dimension, a clamp that clips
    ((4, 1, 9, 9), 1, True, "lrelu", None, 0.25),       # C = 1
    ((5, 67), 1, False, "lrelu", 0.5, 0.375),           # no bias
    ((2, 3, 11), 0, True, "linear", None, None),        # dim 0
])
def test_bias_act_is_the_binary32_restatement_exactly(P, shape, dim, has_b, act, gain, clamp):
    gen = torch.Generator().manual_seed(sum(shape) + dim)
    x = torch.randn(*shape, generator=gen)
    b = torch.randn(shape[dim], generator=gen) if has_b else None
    assert x.numel() % 256 != 0
    want = p3d_torch_ops.bias_act(x, b, dim=dim, act=act, gain=gain, clamp=clamp)
    if clamp is not None:
        assert 0.05 < float((want.abs() == clamp).float().mean()) < 0.95, "the clamp does not clip"
    got = P.ops.bias_act(x.cuda(), None if b is None else b.cuda(), dim=dim, act=act, gain=gain, clamp=clamp)
    assert torch.equal(got.cpu(), want)


# (H, W, fh, fw, down): H * up + pady0 + pady1 - fh = -1 in y, in x only, and -3 (refused before the fix too)
@pytest.mark.parametrize("H,W,fh,fw,down", [(3, 8, 4, 4, 2), (8, 3, 4, 4, 2), (8, 4, 3, 5, 3), (1, 8, 4, 4, 2)],
                         ids=["y-minus1", "x-minus1", "x-minus1-down3", "y-minus3"])
def test_input_smaller_than_the_filter_is_refused(P, H, W, fh, fw, down):
    """Truncating division gave such a call one output row (or column); the buffer is large enough for that shape, so a launch
    would show as written values, not as a fault."""
    L = P._lib.lib()
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    NC = 3
    x, f = torch.randn(NC, H, W).cuda(), torch.ones(fh, fw, device="cuda")
    y = torch.full((NC * (H + 2) * (W + 2) + 4096,), float("nan"), device="cuda")
    torch.cuda.synchronize()
    rc = L.p3d_upfirdn2d_f32(p(x), NC, H, W, p(f), fh, fw, 1, down, 0, 0, 0, 0, p(y), None)
    torch.cuda.synchronize()
    assert rc == -2, "P3D_E_RANGE: the operator has no output"
    assert bool(torch.isnan(y).all()), "a refused call wrote into y"
    with pytest.raises(RuntimeError, match="smaller than"):
        P.ops.upfirdn2d(x[None], f, down=down)
