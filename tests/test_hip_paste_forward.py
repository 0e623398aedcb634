"""GPU (-m gpu): the front-view paste's forward kernel (k_paste_front, csrc/p3d_paste.hip; p3d_paste_front_f32; ops.paste_front) at small
ragged shapes against the float64 restatement of tests/paste_cases.py, under its gate: the 0/1 masks equal on every decided pixel,
mask_occ / mask / paste / image within per-pixel allowances built from the restatement alone (tests/test_paste_forward_cpu.py shows
that the restatement is float64 torch, that a legitimate binary32 result passes and that eleven seeded faults fail).  Values exactly
on a threshold, one direct C-ABI call into NaN-filled, guarded buffers, and the wrapper's refusals."""
import ctypes as C

import pytest
import torch

import paste_cases as PC

pytestmark = pytest.mark.gpu
OUTPUTS = ("image", "paste", "mask", "mask_weights", "mask_edges", "mask_occ", "mask_dxyz")


@pytest.fixture(scope="module")
def P():
    import panic3d_amd
    panic3d_amd.build()
    panic3d_amd._lib.lib()
    return panic3d_amd


def _run(P, inputs, thresholds, norm):
    d = {k: v.cuda() for k, v in inputs.items()}
    return P.ops.paste_front(d["weights"], d["xyz"], d["occ"], d["rays_o"], d["rays_d"], d["front"], d["image"], *thresholds, PC.BW, norm)


@pytest.mark.parametrize("ci", range(len(PC.CASES)), ids=PC.CASE_IDS)
def test_paste_forward_kernel_vs_float64(P, ci):
    case = PC.CASES[ci]
    N, S = case[2], case[1]
    inputs, ref = PC.case_reference(case)
    out = _run(P, inputs, PC.case_thresholds(case), case[4])
    assert set(out) == set(OUTPUTS)
    for k in OUTPUTS:
        assert tuple(out[k].shape) == (N, 3 if k in ("image", "paste") else 1, S, S) and bool(torch.isfinite(out[k]).all()), k
    und, cap = PC.undecided(ref), PC.undecided_cap(case)
    rep = PC.gate(out, ref)
    print(f"{PC.CASE_IDS[ci]}: undecided " + ", ".join(f"{k} {v}" for k, v in und.items()) + f" (cap {cap}); differing decided pixels " +
          ", ".join(f"{k} {rep[k]}" for k in PC.BINARY) + "; worst ratio against the allowance " + ", ".join(f"{k} {rep[k]:.3g}" for k in PC.CONTINUOUS))
    assert all(v <= cap for v in und.values()), und
    assert not PC.gate_failures(rep), rep
    # the product of the kernel's own four masks, in the kernel's order, bit for bit
    assert torch.equal(out["mask"], ((out["mask_weights"] * out["mask_edges"]) * out["mask_occ"]) * out["mask_dxyz"])
    again = _run(P, inputs, PC.case_thresholds(case), case[4])  # no atomics: the same bits
    for k in OUTPUTS:
        assert torch.equal(out[k], again[k]), k


def test_paste_forward_ties_are_exact(P):
    """Weights equal to thresh_weight (strict >), occ equal to thresh_occ (strict <), a discrepancy of exactly 5/16 = thresh_dxyz
    (strict <), each next to values on the passing side: the masks written by hand in paste_cases.ties_case."""
    inputs, thresholds, expect = PC.ties_case()
    PC.check_ties(_run(P, inputs, thresholds, False), inputs, expect)


def test_paste_forward_c_abi_writes_every_element_and_nothing_else(P):
    """p3d_paste_front_f32 called directly at (r, S, N) = (5, 37, 2): every output buffer starts as NaN and is followed by a guard of
    0xFF bytes; afterwards every element is finite, the guards are untouched and the values are the wrapper's bits."""
    case = PC.CASES[1]
    r, S, N = case[:3]
    assert N * S * S % 256 != 0
    inputs, _ = PC.case_reference(case)
    thr = PC.case_thresholds(case)
    want = _run(P, inputs, thr, case[4])
    d = {k: v.cuda().contiguous() for k, v in inputs.items()}
    guard = 4096
    bufs = {}
    for k in OUTPUTS:
        n = N * (3 if k in ("image", "paste") else 1) * S * S
        b = torch.full((n * 4 + guard,), 0xFF, dtype=torch.uint8, device="cuda")
        b[:n * 4].view(torch.float32).fill_(float("nan"))
        bufs[k] = (b, n)
    a = P._lib.PasteArgs(*[d[k].data_ptr() for k in ("weights", "xyz", "occ", "rays_o", "rays_d", "front", "image")],
                         *[bufs[k][0].data_ptr() for k in OUTPUTS], N, r, S, 0, int(case[4]), *thr, PC.BW)
    assert [n for n, _ in P._lib.PasteArgs._fields_[7:14]] == ["out_" + k for k in OUTPUTS]
    torch.cuda.synchronize()
    rc = P._lib.lib().p3d_paste_front_f32(C.byref(a), None)
    torch.cuda.synchronize()
    assert rc == 0
    for k in OUTPUTS:
        b, n = bufs[k]
        got = b[:n * 4].view(torch.float32)
        assert bool(torch.isfinite(got).all()), k
        assert bool((b[n * 4:] == 0xFF).all()), k
        assert torch.equal(got, want[k].reshape(-1)), k


def test_paste_forward_wrapper_refusals(P):
    inputs, _ = PC.case_reference(PC.CASES[1])
    d = {k: v.cuda() for k, v in inputs.items()}
    thr = PC.case_thresholds(PC.CASES[1])

    def call(**kw):
        a = dict(d, **kw)
        return P.ops.paste_front(a["weights"], a["xyz"], a["occ"], a["rays_o"], a["rays_d"], a["front"], a["image"], *thr, PC.BW, True)
    call()
    for k in ("weights", "occ", "rays_o", "rays_d", "image"):
        with pytest.raises(RuntimeError):
            call(**{k: d[k][:1]})  # another batch
        with pytest.raises(RuntimeError):
            call(**{k: d[k][..., :-1].contiguous()})  # another width
    with pytest.raises(RuntimeError):
        call(front=torch.cat([d["front"], d["front"][:1]]))  # a batch that is neither 1 nor N
    with pytest.raises(RuntimeError):
        call(front=d["front"][..., :-1, :].contiguous())
    with pytest.raises(RuntimeError):
        call(xyz=d["xyz"][..., :-1].contiguous())  # not square
    with pytest.raises(RuntimeError):
        call(xyz=d["xyz"][:, :2].contiguous())  # two channels: the kernel would read a third
    with pytest.raises(RuntimeError):
        call(xyz=d["xyz"][0])
    with pytest.raises(RuntimeError):
        call(weights=inputs["weights"])  # a CPU tensor
