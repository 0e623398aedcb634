"""GPU (-m gpu): every instantiation of the stand-alone ToRGB GEMM (k_torgb, csrc/p3d_torgb.hip; p3d_torgb_f32; ops.torgb) at the small
ragged shapes of tests/torgb_cases.py against its float64 reference, under the project's gate (tests/test_torgb_cases_cpu.py shows that
the reference is float64 torch, that binary32 torch passes the gate and that nine seeded faults fail it).  Per case: ops.torgb under the
gate; a direct C-ABI call into a NaN-filled buffer with NaN guards on both sides gives the same bits, writes every element and nothing
beside it; torgb_weights is the transposed, zero-padded matrix bit for bit.  The identities the kernel's comments promise, by batch
replication: one image at N = 1 runs PRE (I <= 512) or MS (I > 512); copied until 3 * KS tiles > 1024 it runs k_torgb<3,true>, and every
copy must have the N = 1 call's bits.  The calls the library must refuse, through the C ABI."""
import ctypes as C

import pytest
import torch

import torgb_cases as TC
from synthesis_grad_ref import gate

pytestmark = pytest.mark.gpu
GUARD = 4096  # floats on either side of y


@pytest.fixture(scope="module")
def P():
    import panic3d_amd
    panic3d_amd.build()
    panic3d_amd._lib.lib()
    return panic3d_amd


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _c_abi(P, x, wt, O, s, bias, clamp, skip, skipf, shape=None, null=()):
    """p3d_torgb_f32 called directly, y inside a NaN-filled buffer.  Returns (code, y [N,O,H,W] view, True if the guards are untouched)."""
    N, I, H, W = shape or x.shape
    n = max(N, 1) * O * H * W
    buf = torch.full((n + 2 * GUARD,), float("nan"), device="cuda")
    a = dict(x=x, wt=wt, styles=s, bias=bias, skip=skip, skipf=skipf, y=buf[GUARD:])
    for k in null:
        a[k] = None
    torch.cuda.synchronize()
    rc = P._lib.lib().p3d_torgb_f32(_ptr(a["x"]), N, I, H, W, _ptr(a["wt"]), O, _ptr(a["styles"]), _ptr(a["bias"]),
                                    float(clamp if clamp is not None else -1), _ptr(a["skip"]), _ptr(a["skipf"]), _ptr(a["y"]), None)
    torch.cuda.synchronize()
    guards = bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + n:]).all())
    return rc, buf[GUARD:GUARD + n], guards


@pytest.mark.parametrize("ci", range(len(TC.CASES)), ids=TC.CASE_IDS)
def test_torgb_kernel_vs_float64(P, ci):
    c = TC.CASES[ci]
    t, ref = TC.make_inputs(c), TC.case_ref(c)
    d = {k: (None if v is None else v.cuda()) for k, v in t.items()}
    wt = P.ops.torgb_weights(d["w"][:, :, None, None].contiguous())
    assert torch.equal(wt.cpu(), TC.weights_t(t["w"])), "torgb_weights: the transposed, zero-padded weights"
    y = P.ops.torgb(d["x"], wt, c.O, d["s"], d["bias"], c.clamp, d["skip"], d["f"])
    assert tuple(y.shape) == (c.N, c.O, c.H, c.W)
    gate(f"{c.id} {c.kernel}", y, ref["y"], ref["absref"], ref["K"])
    skipf = None if c.filt is None else P.ops.prepared_filter(d["f"], d["x"].device, 4.0, False)
    rc, y2, guards = _c_abi(P, d["x"], wt, c.O, d["s"], d["bias"], c.clamp, d["skip"], skipf)
    assert rc == 0 and guards, "the call wrote outside y"
    assert bool(torch.isfinite(y2).all()), "an element of y was not written"
    assert torch.equal(y2, y.reshape(-1)), "a second call gives other bits"


# Both I ranges: PRE (I <= 512) and MS (I > 512).  The map and the number of copies are fixed inside the test: O = 40, 22 x 44 = 31 KS
# tiles per image, so 3 * 31 = 93 <= 1024 at N = 1 and 3 * 12 * 31 = 1116 > 1024 at N = 12 (12 * 8 PX tiles: still the KS shape); the
# assert restates the dispatch rule of csrc/p3d_torgb_plan.hpp for those two launches
@pytest.mark.parametrize("I", [200, 512, 513, 1024])
def test_batch_replication_ties_pre_and_ms_to_the_loop_kernel(P, I):
    O, H, W, copies = 40, 22, 44, 12
    assert 3 * (-(-H * W // 32)) <= 1024 < 3 * copies * (-(-H * W // 32)) and copies * (-(-H * W // 128)) < 512
    c1 = TC.Case(f"replicated-i{I}", TC.PRE if I <= 512 else TC.MS, 1, I, O, H, W, True, TC.CLAMP, "asym")
    t, ref = TC.make_inputs(c1), TC.case_ref(c1)
    d = {k: (None if v is None else v.cuda()) for k, v in t.items()}
    wt = P.ops.torgb_weights(d["w"][:, :, None, None].contiguous())
    one = P.ops.torgb(d["x"], wt, O, d["s"], d["bias"], c1.clamp, d["skip"], d["f"])
    rep = lambda v: v.expand(copies, *v.shape[1:]).contiguous()
    many = P.ops.torgb(rep(d["x"]), wt, O, rep(d["s"]), d["bias"], c1.clamp, rep(d["skip"]), d["f"])
    # both sides under the float64 gate first: a failure here is a kernel's, a failure below the comment's
    gate(f"{c1.id} N = 1 ({c1.kernel})", one, ref["y"], ref["absref"], ref["K"])
    gate(f"{c1.id} N = {copies} ({TC.KS3})", many[copies - 1:], ref["y"], ref["absref"], ref["K"])
    for n in range(copies):
        assert torch.equal(many[n], one[0]), f"image {n} of the k_torgb<3,true> launch differs from the {c1.kernel} launch"


def _base(P, O=3, I=8, H=4, W=4, N=2):
    """Buffers of the refusals' base call, large enough for what each refused shape names."""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(max(N, 1), I, H, W, generator=g).cuda()
    w = torch.randn(min(O, 96), I, 1, 1, generator=g).cuda()
    wt = torch.zeros(I, 96, device="cuda")
    wt[:, :min(O, 96)] = w[:, :, 0, 0].t()
    skip = torch.randn(max(N, 1), O, (H + 1) // 2, (W + 1) // 2, generator=g).cuda()
    return dict(x=x, wt=wt if O > 32 else wt[:, :32].contiguous(), s=torch.ones(max(N, 1), I, device="cuda"), skip=skip,
                skipf=P.ops.prepared_filter(TC.setup_filter([1, 3, 3, 1]), x.device, 4.0, False))


@pytest.mark.parametrize("name,change,code", TC.REFUSALS, ids=[r[0] for r in TC.REFUSALS])
def test_torgb_refusals_write_nothing(P, name, change, code):
    shape = dict(N=2, I=8, O=3, H=4, W=4)
    shape.update({k: v for k, v in change.items() if k != "null"})
    b = _base(P, **shape)
    rc, y, guards = _c_abi(P, b["x"], b["wt"], shape["O"], b["s"], None, None, b["skip"], b["skipf"],
                           shape=(shape["N"], shape["I"], shape["H"], shape["W"]), null=change.get("null", ()))
    assert rc == code, name
    assert guards and bool(torch.isnan(y).all()), "a refused call wrote into y"


def test_torgb_weights_refuses_97_channels(P):
    w = torch.randn(97, 8, device="cuda")
    wt = torch.full((8 * 128,), float("nan"), device="cuda")
    torch.cuda.synchronize()
    assert P._lib.lib().p3d_torgb_weights_f32(_ptr(w), 97, 8, _ptr(wt), None) == -2
    assert P._lib.lib().p3d_torgb_weights_f32(None, 3, 8, _ptr(wt), None) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(wt).all())
    with pytest.raises(RuntimeError):
        P.ops.torgb_weights(w[:, :, None, None])
