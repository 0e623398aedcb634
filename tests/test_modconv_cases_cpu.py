"""CPU: the designed matrix of the forward modulated convolution (tests/modconv_cases.py) and its reference and gate
(tests/modconv_ref.py), checked without a GPU.
(1) The list against the plan: every case passes the library's validation rules, reaches exactly the plan cell it names (the plan
    header compiled into tests/conv_plan_host.cpp's `q` request) and the list keeps its coverage conditions.
(2) The reference: float64 agreement with torch's own conv2d / conv_transpose2d formulation at every case, and the reference's
    recorded layer outputs (tests/golden/syn_layers.npz).
(3) The gate is neither vacuous nor too tight: float32 evaluations of every case in several summation orders, with the emulated
    one-term / two-term operand arithmetic of the f16 modes, stay within a quarter of GATE_C; each seeded defect — a transformation of
    that arithmetic, no kernel involved — fails the gate on a named case."""
import collections
import math
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import modconv_cases as MC
import modconv_ref as R
import p3d_testing as T
from host_build import compile_host

MMA = {"f32": 0, "f16": 1, "x2": 2}
SWITCHES = ("P3D_UP4", "P3D_UP4_RPW", "P3D_UP3_FUSED", "P3D_UP5", "P3D_FIR_IMG2")
KERNELS = ["k_modconv<0>", "k_modconv<1>", "k_modconv_h<0,false>", "k_modconv_h<0,true>", "k_modconv_h<1,false>", "k_modconv_h<1,true>",
           "k_modconv_w2<false>", "k_modconv_w2<true>", "k_modconv_w3<false>", "k_modconv_w3<true>", "k_modconv_up", "k_modconv_up_h<false>",
           "k_modconv_up_h<true>", "k_modconv_up3<false>", "k_modconv_up3<true>", "k_modconv_up5", "k_modconv_up4<8,2,3>", "k_modconv_up4<4,2,2>"]
REDUCES = ["-", "k_splitk_reduce", "k_splitk_reduce_img"]
TAILS = ["-", "k_act_to_image", "k_fir4x4_tiled", "k_fir4x4_img<false,4,2>", "k_fir4x4_img<true,2,3>", "k_fir4x4_img2<8>", "k_fir4x4_img2<32>"]
PIPELINED = ["k_modconv_w2<false>", "k_modconv_w2<true>", "k_modconv_w3<false>", "k_modconv_w3<true>", "k_modconv_up3<false>",
             "k_modconv_up3<true>", "k_modconv_up5", "k_modconv_up4<8,2,3>", "k_modconv_up4<4,2,2>"]
# the plan flags that can be true and false on a main kernel (csrc/p3d_conv_plan.hpp): a shallow split or none / a deep one; an fp32
# input or an image (the ToRGB ride takes images only); an image output wanted from the one-launch kernels or not
BOTH = {"fir_sums": ["k_modconv_up", "k_modconv_up_h<false>", "k_modconv_up_h<true>", "k_modconv_up3<false>", "k_modconv_up5"],
        "pre_image": ["k_modconv_w3<false>", "k_modconv_up3<false>", "k_modconv_up3<true>", "k_modconv_up5", "k_modconv_up4<8,2,3>", "k_modconv_up4<4,2,2>"],
        "main_img": ["k_modconv_w3<false>", "k_modconv_w3<true>", "k_modconv_up4<8,2,3>", "k_modconv_up4<4,2,2>"]}
FAMILY = {"k_modconv<0>": "modconv", "k_modconv<1>": "modconv", "k_modconv_w2<false>": "w2", "k_modconv_w2<true>": "w2", "k_modconv_w3<false>": "w3",
          "k_modconv_w3<true>": "w3", "k_modconv_up": "up", "k_modconv_up3<false>": "up3", "k_modconv_up3<true>": "up3", "k_modconv_up5": "up3",
          "k_modconv_up4<8,2,3>": "up4", "k_modconv_up4<4,2,2>": "up4"}
IDS = [c.id for c in MC.CASES]


# ---- (1) the list against the plan ------------------------------------------------------------------------------------------------
def _wide(W):
    return W >= 32


def _ksplit(N, I, O, GH, GW, tw):
    wgs, ks = ((GW + tw - 1) // tw) * ((GH + 7) // 8) * ((O + 63) // 64) * N, 1
    while ks < 64 and wgs * ks < 256 and I // (ks * 2) >= 8:
        ks *= 2
    return ks


def validation_error(c):
    """modconv_impl's and p3d_modconv2d_ex_f32's checks (p3d_synthesis.hip) and the plan header's conv_* rules, restated once: None
    for a call the library accepts."""
    ximg, yimg, rgb = c.xin == "img", c.out in ("img", "both", "rgb+img"), c.out.startswith("rgb")
    w3 = c.I % 16 == 0 and c.O % 64 == 0 and _wide(c.W)
    up3 = c.I % 16 == 0 and c.O % 32 == 0 and c.W >= 4
    if not ((c.ks == 3 and c.up in (1, 2)) or (c.ks == 1 and c.up == 1)):
        return "taps / up"
    if c.mma != "f32" and c.I % 16:
        return "f16 operands need I % 16 == 0"
    if c.layout not in ("oik", "lib"):
        return "a weight layout that conv_weight_layout does not name for the layer"
    if c.layout == "lib" and (c.mma != "x2" or c.ks != 3):
        return "image layouts are two-term 3x3 layouts"
    if ximg and (c.mma != "x2" or c.ks != 3 or c.I % 16 or c.demod is True or not (_wide(c.W) if c.up == 1 else up3)):
        return "image input"
    if yimg and (c.O % 8 or c.ks != 3):
        return "image output"
    if c.out == "img" and c.up != 2 or c.out == "both" and c.up != 1:
        return "up = 2 writes the image instead of y, up = 1 next to it"
    if rgb and not (c.up == 1 and c.ks == 3 and ximg and 1 <= c.R <= 4 and w3 and _ksplit(c.N, c.I, c.O, c.H, c.W, 32) == 1):
        return "ToRGB ride"
    if c.noise == "per" and c.N < 2:
        return "per-sample noise needs N > 1"
    return None


def test_every_case_passes_the_validation_rules():
    for c in MC.CASES:
        assert validation_error(c) is None, (c.id, validation_error(c))
    assert 80 <= len(MC.CASES) <= 120


def test_every_refused_call_fails_the_validation_rules():
    """The calls tests/test_hip_modconv_edges.py expects the library to refuse: each fails a rule, and only the rule it is there for."""
    rule = {"img-narrow": "image input", "img-o-not-32": "image input", "rgb-split": "ToRGB ride", "wrong-layout": "a weight layout"}
    assert sorted(r[0] for r in MC.REFUSALS) == sorted(rule)
    for rid in rule:
        c = MC.refusal_case(rid)
        assert (validation_error(c) or "").startswith(rule[rid]), (rid, validation_error(c))
        assert validation_error(c._replace(W=32, O=64, R=0, out="y", layout="oik")) is None, rid  # the shape next to it is accepted


def plan_lines(exe, cases):
    req = []
    for c in cases:
        sw = [c.sw.get(k, -1) for k in SWITCHES]
        req.append("q %d %d %d %d %d %d %d %d %d %d %d %d %g %d %d %d %d %d" % (
            c.N, c.I, c.O, c.H, c.W, c.ks, c.up, MMA[c.mma], c.xin == "img", c.out in ("img", "both", "rgb+img"), c.out.startswith("rgb"),
            c.act == "lrelu", c.alpha, *sw))
    res = subprocess.run([exe], input="\n".join(req) + "\n", capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    out = []
    for line in res.stdout.splitlines():
        _, main, ks, red, tail, fs, pi, mi = line.split()
        ks = int(ks)
        out.append((main, "1" if ks == 1 else "2-8" if ks <= 8 else ">8", red, tail, int(fs), int(pi), int(mi)))
    assert len(out) == len(cases)
    return out


def test_every_case_reaches_the_cell_it_names_and_the_list_covers_the_plan(tmp_path):
    exe = compile_host(tmp_path, "conv_plan_host.cpp")
    got = plan_lines(exe, MC.CASES)
    for c, cell in zip(MC.CASES, got):
        assert c.cell == cell, (c.id, c.cell, cell)
    assert MC.BY_ID["up3-refused-up4"].sw == {"P3D_UP4": 1} and MC.BY_ID["up3-refused-up4"].alpha == 2.0 \
        and not MC.BY_ID["up3-refused-up4"].cell[0].startswith("k_modconv_up4")
    by = collections.defaultdict(list)
    for c in MC.CASES:
        by[("main", c.cell[0])].append(c)
        by[("reduce", c.cell[2])].append(c)
        by[("tail", c.cell[3])].append(c)
    for kind, values in (("main", KERNELS), ("reduce", REDUCES), ("tail", TAILS)):
        assert {v for k, v in by if k == kind} == set(values)
        for v in values:
            cs = by[(kind, v)]
            assert len(cs) >= 2 and any(c.N == 1 for c in cs) and any(c.N == 3 for c in cs), (kind, v)
            assert any(c.H < c.W for c in cs) and any(c.H > c.W for c in cs), (kind, v)
    for j, flag in ((4, "fir_sums"), (5, "pre_image"), (6, "main_img")):
        for k in BOTH[flag]:
            assert {c.cell[j] for c in by[("main", k)]} == {0, 1}, (flag, k)
    for k in PIPELINED:  # per-sample noise with three samples on every pipelined kernel
        assert any(c.noise == "per" and c.N == 3 for c in by[("main", k)]), k
    fam = collections.defaultdict(list)
    for c in MC.CASES:
        fam[FAMILY.get(c.cell[0]) or ("up_h" if c.cell[0].startswith("k_modconv_up_h") else "h")].append(c)
    for name, cs in fam.items():  # every epilogue option in every family
        assert {c.noise for c in cs} == {None, "const", "per"}, name
        assert {c.demod for c in cs} == {True, False, "dcoef"} and {c.bias for c in cs} == {True, False}, name
        assert {c.act for c in cs} == {"linear", "lrelu"} and any(c.alpha != 0.2 for c in cs), name
        assert any(c.clamp is not None for c in cs) and len({c.gain for c in cs}) >= 3, name


# ---- (2) the reference ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def refs():
    """Inputs and float64 reference of every case, computed once and left unchanged."""
    out = {}
    for c in MC.CASES:
        t = R.make_inputs(c)
        out[c.id] = (t, R.case_ref(c, t))
    return out


def test_reference_agrees_with_torchs_own_convolutions(refs):
    for c in MC.CASES:
        t, ref = refs[c.id]
        d = lambda v: v.double() if v is not None else None
        x, w, s = d(t["x"]), d(t["w"]), d(t["s"])
        if c.mma == "f16":  # the operands the header documents: f16(s * x), f16(w); the demodulation from the fp32 weights
            dco = t["dcoef"].double() if t["dcoef"] is not None else R.demod_coefs(t["w"], t["s"]) if c.demod else torch.ones(c.N, c.O, dtype=torch.float64)
            x, w, s = R.f16_round(t["s"][:, :, None, None] * t["x"]), R.f16_round(t["w"]), torch.ones_like(s)
        else:
            dco = d(t["dcoef"])
        pre = R.torch_modconv_ref(x, w, s, d(t["noise"]), c.up, c.demod is True, d(t["bias"]), d(t["f"]), dcoef=dco)
        assert R.rel_l2(ref["pre"], pre) < 1e-13, c.id
        v = F.leaky_relu(pre, c.alpha) if c.act == "lrelu" else pre
        v = v * c.gain
        v = v.clamp(-c.clamp, c.clamp) if c.clamp is not None else v
        assert R.rel_l2(ref["y"], v) < 1e-13, c.id
        assert (ref["absref_pre"] >= ref["pre"].abs() * (1 - 1e-12)).all(), c.id


@pytest.mark.parametrize("tag", ["conv1", "conv0", "conv0b"])
def test_reference_reproduces_the_recorded_layer_outputs(tag):
    g = T.load_golden("syn_layers.npz")
    cin, cout, res, up = (int(v) for v in g[f"{tag}_cfg"])
    sd = {k[len(tag) + 4:]: torch.from_numpy(v) for k, v in g.items() if k.startswith(f"{tag}_sd_")}
    x, wl = torch.from_numpy(g[f"{tag}_x"]), torch.from_numpy(g[f"{tag}_w"])
    s = F.linear(wl, sd["affine__weight"] * (1.0 / math.sqrt(wl.shape[1])), sd["affine__bias"])  # FullyConnectedLayer, lr_multiplier 1
    noise = sd["noise_const"] * sd["noise_strength"]
    ref = R.modconv_ref(x, sd["weight"], s, up=up, noise=noise, bias=sd["bias"], f=R.setup_filter((1.0, 3.0, 3.0, 1.0)), act="lrelu", alpha=0.2,
                        gain=math.sqrt(2.0))
    err = float(np.abs(ref["y"].numpy() - g[f"{tag}_y"]).max() / max(1e-12, np.abs(g[f"{tag}_y"]).max()))
    assert err < 2e-6 * np.sqrt(cin * 9) + 1e-6, err  # test_synthesis_layer_vs_reference's tolerance


# ---- (3) float32 evaluations, summation orders, emulated operands, seeded defects ----------------------------------------------------
def _operand_terms(c, t, defect):
    """The products a kernel of this operand mode sums, as float32 tensors: [(a, b), ...] and the scale of the sum."""
    s = t["s"][:1].expand_as(t["s"]) if defect == "sample0_styles" else t["s"]
    xs = s[:, :, None, None] * t["x"]                      # fp32
    if c.mma == "f32":
        return [(xs, t["w"])], 1.0
    if c.mma == "f16":
        return [(R.flushed(xs.half()).float(), R.flushed(t["w"].half()).float())], 1.0
    A, B = xs * 16.0, t["w"] * 64.0
    Ah, Bh = A.half(), B.half()
    Al, Bl = (A - Ah.float()).half(), (B - Bh.float()).half()
    Ah, Al, Bh, Bl = (R.flushed(v).float() for v in (Ah, Al, Bh, Bl))
    return [(Ah, Bh), (Al, Bh), (Ah, Bl)], 1.0 / 1024.0


def _conv32(a, b, up, defect):
    if defect == "border_unpadded" and up == 1 and b.shape[-1] == 3:  # the border taps read the neighbouring value, not the padding
        H, W = a.shape[-2:]
        ap = F.pad(a, [1, 1, 1, 1], mode="replicate")
        return sum(torch.einsum("oi,nihw->nohw", b[:, :, ky, kx], ap[:, :, ky:ky + H, kx:kx + W]) for ky in range(3) for kx in range(3))
    return R.conv_taps(a, b, up)


def eval_f32(c, t, chunk, slices, defect=None):
    """One float32 evaluation: the K loop in chunks of `chunk` channels, the chunks dealt to `slices` split-K slices that are summed
    in slice order, then the FIR pass, the demodulation, noise, bias and the epilogue, every step rounded to float32.  `defect`: one
    of DEFECTS, a transformation of this arithmetic."""
    terms, scale = _operand_terms(c, t, defect)
    bounds = list(range(0, c.I, chunk)) + [c.I]
    chunks = list(zip(bounds[:-1], bounds[1:]))
    if defect == "last_chunk_dropped":
        chunks = chunks[:-1]
    per = -(-len(chunks) // slices)
    parts = []
    for j in range(0, len(chunks), per):
        acc = None
        for lo, hi in chunks[j:j + per]:
            for a, b in terms:
                v = _conv32(a[:, lo:hi], b[:, lo:hi], c.up, defect)
                acc = v if acc is None else acc + v
        parts.append(acc)
    if defect == "slice_dropped":
        parts = parts[:1] + parts[2:]
    if defect == "slice_twice":
        parts = parts + parts[:1]
    acc = parts[0]
    for p in parts[1:]:
        acc = acc + p
    acc = acc * scale
    if defect == "tile_tail_shifted":  # the last 16-column tile stores its columns one to the right
        c0 = (acc.shape[-1] - 1) // 16 * 16
        acc = torch.cat([acc[..., :c0], acc[..., c0 - 1:-1]], dim=-1)
    if defect == "tile_last_row_missing":
        acc = acc.clone()
        acc[..., 7, :] = 0.0
    if c.up == 2:
        if defect == "pitch_2w1":  # stored at a pitch of 2W + 4 with column ox at ox + 1, read at a pitch of 2W + 1
            N, O, TH, TW = acc.shape
            buf = acc.new_zeros((N, O, TH, TW + 3))
            buf[..., 1:TW + 1] = acc
            flat = F.pad(buf.reshape(N, O, -1), [0, 8])
            acc = torch.stack([flat[..., r * TW + 1:r * TW + 1 + TW] for r in range(TH)], dim=-2)
        F4 = R.fir4(t["f"], torch.float32, gain=1.0 if defect == "fir_gain_1" else 4.0, flip=defect != "fir_not_flipped")
        acc = R.fir_taps(acc, F4)
    OH, OW = acc.shape[-2:]
    if c.demod is not False:
        d = t["dcoef"] if t["dcoef"] is not None else R.demod_coefs(t["w"], t["s"], torch.float32)
        acc = acc * (d[:1] if defect == "sample0_dcoef" else d)[:, :, None, None]
    if t["noise"] is not None:
        nz = t["noise"].reshape(-1, 1, OH, OW)
        if defect == "sample0_noise":
            nz = nz[:1]
        if defect == "noise_hw_swapped":  # index x * OH + y in place of y * OW + x
            nz = nz.reshape(-1, 1, OW, OH).transpose(-1, -2)
        acc = acc + nz
    if t["bias"] is not None:
        acc = acc + t["bias"][None, :, None, None]
    if defect == "clamp_before_gain":
        v = torch.where(acc < 0, acc * c.alpha, acc) if c.act == "lrelu" else acc
        y = v.clamp(-c.clamp, c.clamp) * np.float32(c.gain)
    elif defect == "lrelu_wrong_side":
        y = R.epilogue(-acc, c.act, np.float32(c.alpha), np.float32(-c.gain), c.clamp)  # the slope on v > 0
    else:
        y = R.epilogue(acc, c.act, np.float32(c.alpha), np.float32(c.gain), c.clamp)
    out = {"y": y}
    if c.out in ("img", "both", "rgb+img"):
        ns = t["s"][:, torch.arange(c.O) % c.I] if defect == "image_producer_styles" else t["ns"]
        A = ns[:, :, None, None] * y * 16.0
        hi = A.half()
        lo = (A - hi.float()).half()
        out["img"] = (R.flushed(hi).float() + R.flushed(lo).float()) * (1.0 / 16.0)
    if c.R:
        G = c.O // 64
        m = (t["rgb_w"][None] * t["rgb_s"][:, None, :]).reshape(c.N, c.R, G, 64)
        yg = y.reshape(c.N, G, 64, OH, OW)
        if defect == "torgb_wrong_group":
            yg = yg.roll(1, dims=1)
        out["rgb"] = torch.einsum("nrgo,ngohw->gnrhw", m, yg)
    return out


def ratios(c, t, ref, got):
    r = {"y": R.gate_ratio(got["y"], ref["y"], ref["absref_y"], ref["K"])}
    if "img" in got:
        r["img"] = R.gate_ratio(got["img"], *R.image_ref(ref, t["ns"]), ref["K"])
    if "rgb" in got:
        part, ab, K = R.torgb_partial_ref(ref, t["rgb_w"], t["rgb_s"])
        r["rgb"] = R.gate_ratio(got["rgb"], part, ab, K)
        img, ab, K = R.torgb_ref(ref, t["rgb_w"], t["rgb_s"], t["rgb_b"])
        r["torgb"] = R.gate_ratio(got["rgb"].sum(dim=0) + t["rgb_b"][None, :, None, None], img, ab, K)
    return r


def test_float32_evaluations_stay_within_a_quarter_of_the_gate(refs):
    """Per-chunk (8-channel chunks for fp32 operands, 16 for f16 ones, one slice), per-split-slice (up to 8 slices summed in slice
    order) and the whole K loop in one sum, with the emulated operands of the f16 modes.  The worst ratio per operand mode is
    recorded in DESIGN.md §4.4."""
    worst = collections.defaultdict(float)
    for c in MC.CASES:
        t, ref = refs[c.id]
        ch = 8 if c.mma == "f32" else 16
        n = -(-c.I // ch)
        for chunk, slices in sorted({(ch, 1), (ch, min(n, 8)), (c.I, 1)}):
            for k, r in ratios(c, t, ref, eval_f32(c, t, chunk, slices)).items():
                worst[(c.mma, k)] = max(worst[(c.mma, k)], r)
                assert r <= R.GATE_C / 4, (c.id, chunk, slices, k, r)
    for k in sorted(worst):
        print("float32 evaluation, mode %s, output %s: worst ratio %.3f of c = %g" % (*k, worst[k], R.GATE_C))
    assert min(worst.values()) > 0.05  # not vacuous: fp32 round-off is a visible share of the gate in every mode and output


# each defect: the named case it must fail on, and the output that shows it
DEFECTS = {
    "last_chunk_dropped": ("m3-9x17", "y"), "slice_dropped": ("hx3-9x17", "y"), "slice_twice": ("up3-9x5", "y"),
    "border_unpadded": ("w2-9x33", "y"), "tile_tail_shifted": ("m3-9x17", "y"), "tile_last_row_missing": ("h3-9x17", "y"),
    "fir_not_flipped": ("up-8x16", "y"), "fir_gain_1": ("uph-9x17", "y"), "pitch_2w1": ("up3-9x5", "y"),
    "sample0_noise": ("up4s-n3", "y"), "sample0_dcoef": ("w3-9x33", "y"), "sample0_styles": ("m3-1xW", "y"),
    "noise_hw_swapped": ("up-1x17", "y"), "clamp_before_gain": ("m3-8x16", "y"), "lrelu_wrong_side": ("m3-7x15", "y"),
    "image_producer_styles": ("fused-7x29", "img"), "torgb_wrong_group": ("rgb-n3", "rgb"),
}


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_seeded_defect_fails_the_gate(refs, defect):
    cid, key = DEFECTS[defect]
    c = MC.BY_ID[cid]
    t, ref = refs[cid]
    ch = 8 if c.mma == "f32" else 16
    slices = min(-(-c.I // ch), 3)
    good = ratios(c, t, ref, eval_f32(c, t, ch, slices))
    bad = ratios(c, t, ref, eval_f32(c, t, ch, slices, defect))
    print(f"{defect} on {cid}: gate ratio {good[key]:.3f} -> {bad[key]:.3g}")
    assert good[key] <= R.GATE_C / 4 and bad[key] > R.GATE_C, (defect, good, bad)
