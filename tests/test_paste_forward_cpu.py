"""CPU (-m "not gpu"): the front-view paste's FORWARD without a device.  The float64 restatement the GPU test measures
k_paste_front against (tests/paste_cases.paste_forward_ref) is float64 torch's own composition; the gate's conditions (few undecided
pixels, balanced masks, fractional and clamped pixels) hold for the restatement alone on every case; a legitimate binary32 result
(the same torch composition in float32) passes the whole gate on every case; eleven seeded faults each fail it on a named case and
output; values exactly on a threshold; and p3d_paste_front_f32's argument errors, which come back before any launch."""
import ctypes as C

import pytest
import torch

import paste_cases as PC
import train_step_cases as TC


@pytest.fixture(scope="module")
def P():
    import panic3d_amd
    panic3d_amd.build()
    return panic3d_amd


def _torch(case, dtype, fault=None):
    return PC.paste_forward_torch(**PC.case_inputs(case), thresholds=PC.case_thresholds(case), box_warp=PC.BW, normalize_images=case[4],
                                  dtype=dtype, fault=fault)


@pytest.mark.parametrize("ci", [1, 2], ids=[PC.CASE_IDS[1], PC.CASE_IDS[2]])
def test_paste_forward_reference_is_float64_torch(P, ci):
    """coords='float64' IS float64 torch (F.interpolate bilinear and nearest, paste.sobel_magnitude, paste.xyz_discrepancy,
    paste.sample_orthofront, torch.lerp) at a ragged case and at a shared, normalised one: the continuous quantities, paste and image
    to rel-L2 1e-12, the masks equal."""
    case = PC.CASES[ci]
    _, ref = PC.case_reference(case, coords="float64")
    t64 = _torch(case, torch.float64)
    for k in ("weights", "edges", "occ", "dxyz"):
        assert TC.rel_l2(ref[k][0], t64["q"][k]) < 1e-12, k
    for k in ("paste", "image", "mask_occ", "mask"):
        assert TC.rel_l2(ref[k][0], t64[k]) < 1e-12, k
    for k in PC.BINARY:
        assert torch.equal(ref[k][0], t64[k]), k
    for k in PC.CONTINUOUS:  # every allowance is a positive number wherever the value can be rounded at all
        assert bool((ref[k][1] >= 0).all()) and bool(torch.isfinite(ref[k][1]).all()), k


def test_nearest_index_is_the_same_integers_in_binary32_and_float64():
    for case in PC.CASES:
        r, S = case[:2]
        assert torch.equal(PC.nearest_index(S, r, "binary32"), PC.nearest_index(S, r, "float64")), (r, S)


@pytest.mark.parametrize("ci", range(len(PC.CASES)), ids=PC.CASE_IDS)
def test_gate_conditions_hold_for_the_reference_alone(ci):
    """Conditions, not measurements: at most 0.5 % undecided pixels per mask (none in a case of fewer than 400 pixels), 10-90 % ones in
    each binary mask, fractional mask_occ pixels, clamped samples in the case built for them.  Three exemptions follow from the shapes
    themselves: at r = 1 and at S = 1 the up-sampled xyz is constant over the Sobel's window, so that mask is one value; one output
    pixel (S = 1) cannot be balanced; at r = 1 and at r = S every tap weight is 0 or 1, so mask_occ has no fractional pixel."""
    case = PC.CASES[ci]
    r, S, N = case[:3]
    _, ref = PC.case_reference(case)
    px = N * S * S
    und, cap = PC.undecided(ref), PC.undecided_cap(case)
    ones = {k: float(ref[k][0].mean()) for k in PC.BINARY}
    frac = float(((ref["mask_occ"][0] > 0) & (ref["mask_occ"][0] < 1)).double().mean())
    clamped = float(ref["clamped"].double().mean())
    print(f"{PC.CASE_IDS[ci]}: {px} pixels, undecided " + ", ".join(f"{k} {v} ({v / px:.3%})" for k, v in und.items()) + f" (cap {cap}); ones " +
          ", ".join(f"{k} {v:.1%}" for k, v in ones.items()) + f"; fractional mask_occ {frac:.1%}; clamped samples {clamped:.1%}")
    assert all(v <= cap for v in und.values()), und
    for k, v in ones.items():
        if S == 1 or (k == "mask_edges" and r == 1):
            continue
        assert 0.1 <= v <= 0.9, (k, v)
    if r == 1 or S == 1:
        q = ref["edges"][0]
        assert float((q - (3e-6) ** 0.5).abs().max()) < 1e-12 and case[6] > 10 * float(q.max())
    if r != 1 and r != S:
        assert frac > 0.05
    occ1 = float((ref["mask_occ"][0] > 0.5).double().mean())
    assert S == 1 or 0.1 <= occ1 <= 0.9
    if ci == PC.CLAMPED_CASE:
        assert 0.5 < clamped < 1.0
    assert int(ref["decided"].sum()) >= px - 3 * cap


@pytest.mark.parametrize("ci", range(len(PC.CASES)), ids=PC.CASE_IDS)
def test_legitimate_binary32_result_passes_the_gate(P, ci):
    """torch's float32 composition on CPU: other binary32 source coordinates than the kernel's (F.interpolate's and grid_sample's own),
    another order of the sums."""
    case = PC.CASES[ci]
    _, ref = PC.case_reference(case)
    rep = PC.gate(_torch(case, torch.float32), ref)
    print(f"{PC.CASE_IDS[ci]}: " + ", ".join(f"{k} {v:.3g}" for k, v in rep.items()))
    assert not PC.gate_failures(rep), rep


# fault -> (index into CASES, output) that must catch it
CAUGHT_BY = {
    "sobel_zero_pad": (5, "mask_edges"), "sobel_centre_1": (0, "mask_edges"), "nearest_rounded": (2, "mask_dxyz"), "occ_after": (1, "mask_occ"),
    "no_sign": (0, "mask_dxyz"), "rays_view0": (7, "mask_dxyz"), "front_view0": (7, "paste"), "swap_xy": (1, "paste"),
    "not_transposed": (2, "paste"), "zeros_padding": (8, "paste"), "align_corners": (9, "mask_weights"),
}


@pytest.mark.parametrize("fault", PC.FAULTS)
def test_seeded_fault_fails_the_gate(P, fault):
    ci, output = CAUGHT_BY[fault]
    case = PC.CASES[ci]
    _, ref = PC.case_reference(case)
    rep = PC.gate(_torch(case, torch.float32, fault=fault), ref)
    print(f"{fault}: caught at {PC.CASE_IDS[ci]} by {output} = {rep[output]:.3g}; all failing outputs {PC.gate_failures(rep)}")
    assert output in PC.gate_failures(rep), rep


def test_every_fault_is_named():
    assert set(CAUGHT_BY) == set(PC.FAULTS) and len(PC.FAULTS) == 11


def test_ties_expected_masks_in_binary32_torch(P):
    """The hand-written masks of the ties case are what torch's float32 composition gives (r = S: F.interpolate's taps have l = 0)."""
    inputs, thresholds, expect = PC.ties_case()
    PC.check_ties(PC.paste_forward_torch(**inputs, thresholds=thresholds, box_warp=PC.BW, normalize_images=False), inputs, expect)
    assert all(0 < int(expect[k].sum()) < 16 for k in ("mask_weights", "mask_occ", "mask_dxyz", "mask"))
    i0, i1, l = TC.up_taps(4, 4)
    assert torch.equal(i0, torch.arange(4)) and torch.count_nonzero(l) == 0


def test_paste_front_argument_errors_without_gpu(P):
    L = P._lib.lib()
    f = 256  # never dereferenced: the checks come first
    pointers = [n for n, t in P._lib.PasteArgs._fields_ if t is C.c_void_p]
    assert len(pointers) == 14
    base = dict({n: f for n in pointers}, N=1, r=16, S=64, front_shared=0, normalize_images=0, thresh_weight=0.5, thresh_edges=0.2,
                thresh_occ=0.5, thresh_dxyz=0.05, box_warp=0.7)

    def call(**kw):
        return L.p3d_paste_front_f32(C.byref(P._lib.PasteArgs(**dict(base, **kw))), None)
    assert L.p3d_paste_front_f32(None, None) == -1
    for n in pointers:
        assert call(**{n: None}) == -1, n
    assert call(N=0) == -1 and call(r=0) == -1 and call(S=0) == -1
    assert call(N=-1) == -1 and call(r=-3) == -1 and call(S=-4) == -1
    assert call(r=4097) == -2 and call(S=8193) == -2
