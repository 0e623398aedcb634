"""GPU (-m gpu): every plan of the FORWARD modulated convolution at small ragged shapes against float64 (csrc/p3d_conv_plan.hpp,
DESIGN.md §4.4).

One test per case of tests/modconv_cases.py (the plan cell each case reaches is checked on the CPU by
tests/test_modconv_cases_cpu.py): ops.modulated_conv2d under the case's environment switches, every output it returns — the fp32
result, the next layer's ActImage through .float(), the riding ToRGB's partial sums and their torgb_combine — against the float64
reference of tests/modconv_ref.py under the project's element-wise gate.  The workspace is WATCHED: ops._conv_scratch is replaced by
a stand-in that hands out exactly p3d_modconv2d_workspace_bytes bytes at the front of a larger buffer filled with 0xFF (NaN as f32
and as f16) just before the launches, so a read of a workspace value that no launch wrote poisons the output and a write past the
reported size shows in the guard bytes.  A second call gives the same bits (the forward has no atomics), the OIK and the image-layout
weight copies give the same bits, and the domain flag stays clear.  Last, the calls the validation refuses: the documented error,
nothing launched.

ops.modulated_conv2d takes the activation's slope from ops._ACTS (bias_act's defaults); a case with another alpha sets that entry for
the length of the test, so that the C ABI's `alpha` is exercised through the same wrapper."""
import pytest
import torch

import modconv_cases as MC
import modconv_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
# (tools/modconv_bits.py imports SWITCHES, DEV, _dev, _weights_f16 and _call from this module: keep the names, or change the tool too)
SWITCHES = ("P3D_UP4", "P3D_UP4_RPW", "P3D_UP3_FUSED", "P3D_UP5", "P3D_FIR_IMG2")
GUARD = 1 << 16  # watched bytes past the reported workspace size


@pytest.fixture(scope="module")
def P():
    import panic3d_amd
    panic3d_amd.build()
    panic3d_amd._lib.lib()
    return panic3d_amd


class WatchedScratch:
    """Stands in for ops._conv_scratch: the first `nbytes` bytes of a 256-byte aligned buffer that is GUARD bytes longer, every byte
    0xFF when the library gets it."""

    def __init__(self):
        self.buf, self.n, self.calls = None, 0, 0

    def __call__(self, device, nbytes):
        raw = torch.empty((int(nbytes) + GUARD + 256,), dtype=torch.uint8, device=device)
        off = (-raw.data_ptr()) % 256
        self.buf, self.n = raw[off:off + int(nbytes) + GUARD], int(nbytes)
        self.buf.fill_(0xFF)
        self.calls += 1
        return self.buf[:self.n]

    def guard_untouched(self):
        return bool((self.buf[self.n:] == 0xFF).all())

    def all_untouched(self):
        return self.buf is None or bool((self.buf == 0xFF).all())


@pytest.fixture
def watched(P, monkeypatch):
    ops = P.ops
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for name in ("_WSB", "_WLAYOUT", "_TAKES_IMAGE", "_FUSES_TORGB"):  # the memoised shape queries a switch could change
        monkeypatch.setattr(ops, name, {})
    w = WatchedScratch()
    monkeypatch.setattr(ops, "_conv_scratch", w)
    return w


def _dev(t):
    return {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in t.items()}


def _weights_f16(ops, c, d, layout):
    if c.mma == "f32":
        return None
    return ops.conv_weights_to_f16(d["w"], split=c.mma == "x2", layout=layout)


def _call(ops, c, d, wf, flag):
    """One ops.modulated_conv2d call of the case -> (y or None, ActImage or None, ToRGB partials or None)."""
    x = ops.act_to_image(d["x"], d["s"], saturated=flag) if c.xin == "img" else d["x"]
    kw = dict(noise=d["noise"], up=c.up, padding=c.ks // 2, resample_filter=d["f"] if c.up == 2 else None, demodulate=c.demod is not False,
              bias=d["bias"], act=c.act, gain=c.gain, clamp=c.clamp, weight_f16=wf, dcoef=d["dcoef"], saturated=flag)
    if c.out in ("img", "both", "rgb+img"):
        kw["next_styles"] = d["ns"]
    if c.R:
        kw.update(rgb_weight=d["rgb_w"], rgb_styles=d["rgb_s"], want_y=c.out != "rgb-noy")
    out = ops.modulated_conv2d(x, d["w"], None if c.xin == "img" else d["s"], **kw)
    if c.R:
        return out
    if c.out == "both":
        return out[0], out[1], None
    return (None, out, None) if c.out == "img" else (out, None, None)


def _bits(out):
    y, img, part = out
    return [None if y is None else y.clone(), None if img is None else img.data.clone(), None if part is None else part.clone()]


def _same_bits(a, b):
    return all((u is None and v is None) or (u is not None and v is not None and torch.equal(u, v)) for u, v in zip(a, b))


@pytest.mark.parametrize("cid", [c.id for c in MC.CASES])
def test_modconv_case_vs_float64(P, watched, monkeypatch, cid):
    ops = P.ops
    c = MC.BY_ID[cid]
    for k, v in c.sw.items():
        monkeypatch.setenv(k, str(v))
    if c.act == "lrelu" and c.alpha != ops._ACTS["lrelu"][1]:
        monkeypatch.setitem(ops._ACTS, "lrelu", (ops._ACTS["lrelu"][0], c.alpha, ops._ACTS["lrelu"][2]))
    t = R.make_inputs(c)
    ref = R.case_ref(c, t)
    d = _dev(t)
    flag = ops.conv_domain_flag(torch.device(DEV))
    lib = ops.conv_weight_layout(c.I, c.O, c.W, c.up) if (c.mma == "x2" and c.ks == 3) else 0
    if c.layout == "lib":
        assert lib != 0, "the case asks for an image layout the library does not name for this shape"
    with torch.no_grad():
        out = _call(ops, c, d, _weights_f16(ops, c, d, lib if c.layout == "lib" else 0), flag)
        torch.cuda.synchronize()
        assert watched.calls == 1 and watched.n == P._lib.lib().p3d_modconv2d_workspace_bytes(c.N, c.I, c.O, c.H, c.W, c.up)
        assert watched.guard_untouched(), "a launch wrote past p3d_modconv2d_workspace_bytes"
        first = _bits(out)
        again = _bits(_call(ops, c, d, _weights_f16(ops, c, d, lib if c.layout == "lib" else 0), flag))
        assert watched.guard_untouched()
        other = _bits(_call(ops, c, d, _weights_f16(ops, c, d, 0 if c.layout == "lib" else lib), flag)) if lib else None
        assert other is None or watched.guard_untouched()
        y, img, part = out
        assert (y is None) == (c.out in ("img", "rgb-noy")) and (img is None) == (c.out not in ("img", "both", "rgb+img")) and (part is None) == (not c.R)
        worst = []
        for v in (y, None if img is None else img.data, part):
            assert v is None or bool(torch.isfinite(v).all()), "an output holds a non-finite value (a workspace value no launch wrote?)"
        if y is not None:
            assert tuple(y.shape) == (c.N, c.O, c.H * c.up, c.W * c.up)
            worst.append(R.gate(f"{cid} y", y, ref["y"], ref["absref_y"], ref["K"]))
        if img is not None:
            assert img.shape == (c.N, c.O, c.H * c.up, c.W * c.up)
            worst.append(R.gate(f"{cid} image", img.float(), *R.image_ref(ref, t["ns"]), ref["K"]))
        if part is not None:
            assert tuple(part.shape) == (c.O // 64, c.N, c.R, c.H, c.W)
            worst.append(R.gate(f"{cid} torgb partials", part, *R.torgb_partial_ref(ref, t["rgb_w"], t["rgb_s"])))
            rgb = ops.torgb_combine(part, bias=d["rgb_b"])
            worst.append(R.gate(f"{cid} torgb", rgb, *R.torgb_ref(ref, t["rgb_w"], t["rgb_s"], t["rgb_b"])))
        print(f"gate {cid} [{c.cell[0]}]: worst {max(worst):.3f} (c = {R.GATE_C:g})")
        assert not ops.conv_domain_violated(flag), "the domain flag was raised at magnitudes of order one"
        assert _same_bits(first, again), "a second call gave other bits"
        assert other is None or _same_bits(first, other), "the OIK and the image-layout weight copies gave other bits"


# the documented error of each refused call: the wrapper's own message where it asks the library's rule first, else the C ABI's
# P3D_E_RANGE through _lib.check
REFUSED_WITH = {"img-narrow": "size out of supported range", "img-o-not-32": "does not stage this up-sampling layer",
                "rgb-split": "conv_fuses_torgb", "wrong-layout": "size out of supported range"}


@pytest.mark.parametrize("rid", [r[0] for r in MC.REFUSALS])
def test_refused_call_returns_the_documented_error_and_launches_nothing(P, watched, rid):
    ops = P.ops
    c = MC.refusal_case(rid)
    t = R.make_inputs(c)
    d = _dev(t)
    lay = c.layout if isinstance(c.layout, int) else 0
    if rid == "rgb-split":
        assert not ops.conv_fuses_torgb(c.N, c.I, c.O, c.H, c.W, c.R)
    if rid == "wrong-layout":
        assert ops.conv_weight_layout(c.I, c.O, c.W, c.up) != lay
    with torch.no_grad():
        wf = ops.conv_weights_to_f16(d["w"], split=True, layout=lay)
        with pytest.raises(RuntimeError, match=REFUSED_WITH[rid]):
            _call(ops, c, d, wf, None)
        torch.cuda.synchronize()
    assert watched.all_untouched(), "a refused call wrote to its workspace"
