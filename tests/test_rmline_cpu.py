"""CPU (-m "not gpu"): the illustration-to-render module without a device — the C ABI (include/p3d_rmline.h, _lib.RMLINE_SIGNATURES and
the library's exports; argument errors come back before any launch), the layer plan as a host program, the batch-norm fold against the
unfolded float64 Sequential, the state-dict names and a Lightning-style checkpoint round trip, the module's host logic on torch
stand-ins of the operators against the literal restatement (tests/rmline_cases.py), the properties of face_hull, and the gates that
tests/test_hip_rmline.py holds the kernels to: the binary32 stand-ins pass them, seeded faults fail them.  On the parent commit the
module, the table and the symbols do not exist."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import rmline_cases as RC
from host_build import compile_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = torch.nn.functional


@pytest.fixture(scope="module")
def P():
    import panic3d_amd
    panic3d_amd.build()
    return panic3d_amd


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_rmline_header_table_and_exports_agree(P):
    hdr = open(os.path.join(ROOT, "include", "p3d_rmline.h")).read()
    declared = set(re.findall(r"\b(p3d_rmline[a-z0-9_]+)\s*\(", hdr))
    lib = P._lib
    assert declared == set(lib.RMLINE_SIGNATURES) and len(declared) == 6
    others = set(lib.SIGNATURES) | set(lib.GRAD_SIGNATURES) | set(lib.SYN_GRAD_SIGNATURES) | set(lib.PASTE_GRAD_SIGNATURES) | set(lib.DISC_SIGNATURES) \
        | set(lib.LOSS_SIGNATURES) | set(lib.OPTIM_SIGNATURES) | set(lib.LPIPS_SIGNATURES) | set(lib.ENCODER_SIGNATURES) | set(lib.METRICS_SIGNATURES)
    assert not declared & others
    L = lib.lib()
    for name in declared:
        assert hasattr(L, name)
    B = P._build
    assert "p3d_rmline.hip" in B.SOURCES and os.path.join("..", "..", "include", "p3d_rmline.h") in B.HEADERS and "p3d_rmline_plan.hpp" in B.HEADERS
    for unit in (B.RENDER_UNIT, B.SYNTHESIS_UNIT):
        assert not any("p3d_rmline" in s for s in unit)
    for name in ("MAX_TAPS", "MAX_DILATE", "MAX_C", "ACT_NONE", "ACT_LEAKY", "ACT_TANH", "TILE_8", "TILE_4", "IN_STACK", "OUT_PLANAR", "OUT_LERP",
                 "IN_NO_MASK", "FWD_MASK_INPUT", "FWD_LERP"):
        assert int(re.search(rf"#define P3D_RMLINE_{name} (\d+)", hdr).group(1)) == getattr(lib, f"P3D_RMLINE_{name}")
    assert lib.P3D_ABI_VERSION == 9 and L.p3d_abi_version() == 9
    src = open(os.path.join(B.CSRC, "p3d_rmline.hip")).read()
    assert "mfma_f32_16x16x4f32" in src and "atomic" not in src.replace("with atomics", "")
    buf = (ctypes.c_size_t * 16)()
    assert L.p3d_rmline_struct_layout(0, buf, 16) == 8 and buf[0] == ctypes.sizeof(lib.RmlineDog) == 48
    assert L.p3d_rmline_struct_layout(1, buf, 16) == 9 and buf[0] == ctypes.sizeof(lib.RmlineLayer) == 40
    assert L.p3d_rmline_struct_layout(1, buf, 3) == -2 and L.p3d_rmline_struct_layout(2, buf, 16) == -2 and L.p3d_rmline_struct_layout(0, None, 16) == -1
    assert P.RMLineGenerator is P.rmline.RMLineGenerator and P.RMLineWrapper is P.rmline.RMLineWrapper and P.face_hull is P.rmline.face_hull


def _dog(P, **kw):
    p = dict(t=1.0, sigma=0.5, k=1.6, epsilon=0.01, kernel_factor=4.0, d=2, reserved=0)
    p.update(kw)
    return P._lib.RmlineDog(p["t"], p["sigma"], p["k"], p["epsilon"], p["kernel_factor"], p["d"], p["reserved"])


def test_rmline_argument_errors_without_gpu(P):
    L = P._lib.lib()
    p = 256  # never dereferenced: the checks come first
    out2 = (ctypes.c_int * 2)()
    assert L.p3d_rmline_dog_taps(_dog(P), out2) == 0 and list(out2) == [5, 7]
    assert L.p3d_rmline_dog_taps(_dog(P, sigma=1.0, t=2.0), out2) == 0 and list(out2) == [9, 13]
    assert L.p3d_rmline_dog_taps(_dog(P, sigma=0.1), out2) == 0 and list(out2) == [3, 3]
    assert L.p3d_rmline_dog_taps(_dog(P, sigma=2.5), out2) == 0 and list(out2) == [21, 33]  # the cap itself
    assert L.p3d_rmline_dog_taps(_dog(P, sigma=2.7), out2) == -2 and L.p3d_rmline_dog_taps(_dog(P, sigma=1e9), out2) == -2
    assert L.p3d_rmline_dog_taps(_dog(P, sigma=0.0), out2) == -1 and L.p3d_rmline_dog_taps(_dog(P, k=float("nan")), out2) == -1
    assert L.p3d_rmline_dog_taps(_dog(P, d=0), out2) == -2 and L.p3d_rmline_dog_taps(_dog(P, d=9), out2) == -2
    assert L.p3d_rmline_dog_taps(_dog(P, k=0.5, sigma=1.0), out2) == -2 and L.p3d_rmline_dog_taps(_dog(P, reserved=1), out2) == -2
    assert L.p3d_rmline_dog_taps(None, out2) == -1 and L.p3d_rmline_dog_taps(_dog(P), None) == -1
    for args in ((1.0, 0.5, 1.6, 0.01, 4), (2.0, 1.0, 1.6, 0.01, 4), (1.0, 0.7, 2.3, 0.0, 3), (1.0, 2.5, 1.6, 0.01, 4)):
        assert L.p3d_rmline_dog_taps(_dog(P, sigma=args[1], k=args[2], kernel_factor=float(args[4])), out2) == 0
        assert tuple(out2) == RC.taps(args[1], args[2], args[4]) == P.ops.rmline_dog_taps(args[1], args[2], args[4])

    def mask(img=p, N=1, C=3, H=8, W=8, hull=None, dog=_dog(P), m=p, image=None, resp=None):
        return L.p3d_rmline_mask_f32(img, N, C, H, W, hull, dog, m, image, resp, None)
    assert mask(img=None) == -1 and mask(m=None) == -1 and mask(dog=None) == -1 and mask(N=0) == -1 and mask(H=0) == -1
    assert mask(C=2) == -2 and mask(C=5) == -2 and mask(H=32769) == -2 and mask(N=65536) == -2 and mask(dog=_dog(P, sigma=3.0)) == -2
    assert mask(C=1, image=p) == -1

    def conv(x=p, image=None, m=None, hull=None, N=1, Hin=8, Win=8, pad=0, Ci=4, wk=p, bias=p, Co=8, act=1, slope=0.01, flags=0, plan=0, out=p):
        return L.p3d_rmline_conv_f32(x, image, m, hull, N, Hin, Win, pad, Ci, wk, bias, Co, act, slope, flags, plan, out, None)
    assert conv(x=None) == -1 and conv(wk=None) == -1 and conv(bias=None) == -1 and conv(out=None) == -1 and conv(N=0) == -1 and conv(Ci=0) == -1
    assert conv(Hin=2) == -2 and conv(Win=2) == -2 and conv(Ci=65) == -2 and conv(Co=65) == -2 and conv(act=3) == -2 and conv(flags=16) == -2
    assert conv(pad=1) == -2 and conv(plan=3) == -2 and conv(Ci=64, Co=64, plan=1) == -2 and conv(slope=float("inf")) == -2
    assert conv(flags=1) == -1 and conv(flags=1, image=p) == -2  # the stack wants an image; three channels without a hull
    assert conv(flags=1, image=p, Ci=3, pad=4) == -2 and conv(flags=1, image=p, hull=p, Ci=3) == -2  # nothing left of the image; a hull is a fourth channel
    assert conv(flags=4, Co=3, image=p, m=p) == -2 and conv(flags=6, Co=3, image=p) == -1 and conv(flags=6, Co=4, image=p, m=p) == -2  # the lerp's needs
    assert conv(flags=7, image=p, m=p, Ci=3, Co=3, pad=2, Hin=12, Win=12) == -2  # stack + lerp: the sizes agree only with pad 1


def test_forward_table_is_checked_before_any_launch(P):
    lib = P._lib
    L = lib.lib()
    p = 256

    def table(*recs):
        tab = (lib.RmlineLayer * len(recs))()
        for t, r in zip(tab, recs):
            for k, v in r.items():
                setattr(t, k, v)
        return tab
    l0 = dict(Ci=4, Co=8, act=1, plan=0, slope=0.01, w_off=0, b_off=288)
    l1 = dict(Ci=8, Co=3, act=2, plan=0, slope=0.0, w_off=296, b_off=512)
    count = ctypes.c_int(7)

    def run(recs=(l0, l1), img=p, N=1, C=4, H=8, W=8, hull=p, dog=_dog(P), weights=p, wf=515, pad=2, flags=3, image=p, mask=p, a0=p, a1=512,
            af=1 * 10 * 10 * 8, out=p):
        return L.p3d_rmline_forward_f32(img, N, C, H, W, hull, dog, table(*recs), len(recs), weights, wf, pad, flags, image, mask, a0, a1, af, out,
                                        ctypes.byref(count), None)
    # every one of these comes back before anything is launched (pointer 256 would fault the process if anything were)
    assert run(img=None) == -1 and run(weights=None) == -1 and run(out=None) == -1 and run(mask=None) == -1 and run(image=None) == -1
    assert run(a0=None) == -1 and run(a1=p) == -1 and run(hull=None) == -1 and run(N=0) == -1
    assert run(C=1) == -2 and run(dog=None) == -2 and run(flags=4) == -2 and run(pad=1) == -2 and run(pad=-1) == -2
    assert run(wf=514) == -2 and run(af=799) == -2 and run(recs=(l0, dict(l1, Ci=7))) == -2 and run(recs=(l0, dict(l1, reserved=1))) == -2
    assert run(recs=(l0, dict(l1, Co=4))) == -2 and run(recs=(l0, dict(l1, act=5))) == -2 and run(recs=(dict(l0, plan=9), l1)) == -2
    assert run(recs=(l0, dict(l1, w_off=-1))) == -2 and run(recs=(l0, dict(l1, b_off=513))) == -2 and run(dog=_dog(P, d=0)) == -2
    assert run(H=1, W=1, pad=0, flags=1) == -2  # nothing left after two unpadded layers
    assert count.value == 0


# ---- the plan -------------------------------------------------------------------------------------------------------------------------
def test_plan_rule_and_its_host_program(P, tmp_path):
    exe = compile_host(tmp_path, "rmline_plan_host.cpp")

    def run(ci, co, force):
        r = subprocess.run([exe, str(ci), str(co), str(force)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, (ci, co, force, r.stderr)  # the program itself checks what the kernel relies on
        return r.stdout.split()
    for ci in (1, 3, 4, 5, 31, 32, 33, 63, 64):
        for co in (1, 3, 7, 16, 17, 32, 33, 64):
            for force in (0, 1, 2):
                out = run(ci, co, force)
                ci4, cot = -(-ci // 4) * 4, 16 if co <= 16 else 32
                fits8 = 4 * (ci4 + 2) * (10 * 34 + 9 * cot) <= 160 * 1024
                if force == 1 and not fits8:
                    assert out == ["error", "-2"]
                    with pytest.raises(ValueError):
                        P.ops.rmline_conv_plan(ci, co, force)
                    continue
                rows = 8 if (force == 1 or (force == 0 and fits8)) else 4
                assert out[0] == "plan" and [int(v) for v in out[1:]] == [1 if rows == 8 else 2, rows, ci4, ci4 + 2, cot, -(-co // cot),
                                                                          4 * (ci4 + 2) * ((rows + 2) * 34 + 9 * cot)]
                pl = P.ops.rmline_conv_plan(ci, co, force)
                assert (pl["plan"], pl["rows"], pl["cot"], pl["lds_bytes"]) == (int(out[1]), rows, cot, int(out[7]))
    assert run(0, 8, 0) == ["error", "-1"] and run(65, 8, 0) == ["error", "-2"] and run(8, 65, 0) == ["error", "-2"] and run(8, 8, 3) == ["error", "-2"]
    assert P.ops.rmline_conv_plan(32, 32)["plan"] == 1 and P.ops.rmline_conv_plan(64, 64)["plan"] == 2  # the reference's layers take the 8-row tile


# ---- the fold and the names -----------------------------------------------------------------------------------------------------------
def test_fold_against_the_unfolded_sequential_in_float64(P):
    """fold_generator's operands are, bit for bit, the float64 fold rounded ONCE to binary32 (a fold done in binary32, or rounded twice,
    gives other bits), and that float64 fold is the unfolded Sequential to 1e-12.  One batch norm carries an eps of its own."""
    for arch in (RC.DEFAULT_ARCH, dict(RC.DEFAULT_ARCH, gen_depth=3, gen_width=5), RC.SMALL_ARCH):
        seq = RC.make_generator(seed=7, **arch)
        if arch["gen_batchnorm"]:
            seq[2].eps = 1e-3
        x = torch.randn(2, 3 + arch["gen_use_hull"], 15, 17, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
        folded = P.rmline.fold_generator(seq)
        assert len(folded) == arch["gen_depth"] and [f[2] for f in folded] == ["leaky"] * (arch["gen_depth"] - 1) + ["tanh"]
        assert all(f[3] == 0.01 for f in folded[:-1]) and all(f[0].dtype == f[1].dtype == torch.float32 for f in folded)
        with torch.no_grad():
            want = seq(x)
            # the fold restated here in float64 from the documented formula; each layer's operands against fold_generator's
            y, scale, shift, layer, differs = x, None, None, 0, False
            for m in seq:
                if isinstance(m, torch.nn.Conv2d):
                    w, b = m.weight, m.bias
                    if scale is not None:
                        b = b + (w * shift.view(1, -1, 1, 1)).sum(dim=(1, 2, 3))
                        w = w * scale.view(1, -1, 1, 1)
                        # what a binary32 fold would give: it must NOT be what fold_generator returns everywhere
                        w32 = m.weight.float() * scale.float().view(1, -1, 1, 1)
                        differs = differs or not torch.equal(RC.to_wk(w32), folded[layer][0])
                        scale = None
                    wk, bias = folded[layer][:2]
                    assert tuple(wk.shape) == (9, w.shape[1], w.shape[0])
                    assert torch.equal(wk, RC.to_wk(w).float()) and torch.equal(bias, b.float()), (arch, layer)
                    y = F.conv2d(y, w, b)
                    layer += 1
                elif isinstance(m, torch.nn.BatchNorm2d):
                    scale = m.weight / torch.sqrt(m.running_var + m.eps)
                    shift = m.bias - m.running_mean * scale
                else:
                    y = m(y)
        assert RC.rel_l2(y, want) <= 1e-12 and layer == arch["gen_depth"]
        assert differs == arch["gen_batchnorm"]  # (the comparison above can tell a binary32 fold from the float64 one)
    # the batch norm folded on the wrong side of the activation is another function
    seq = RC.make_generator(seed=7, **RC.DEFAULT_ARCH)
    x = torch.randn(2, 4, 15, 17, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        wrong = F.leaky_relu(F.batch_norm(F.conv2d(x, seq[0].weight, seq[0].bias), seq[2].running_mean, seq[2].running_var, seq[2].weight, seq[2].bias, False, 0.0, 1e-5))
        right = seq[2](seq[1](seq[0](x)))
    assert RC.rel_l2(wrong, right) > 1e-2
    with pytest.raises(ValueError, match="no convolution after"):
        P.rmline.fold_generator(torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3), torch.nn.LeakyReLU(), torch.nn.BatchNorm2d(4)))


def test_state_dict_names_and_a_lightning_checkpoint_round_trip(P, tmp_path):
    model = P.RMLineGenerator()
    sd = model.state_dict()
    want = RC.state_dict_of(RC.make_generator(**RC.DEFAULT_ARCH), discriminator=False)
    assert set(sd) == set(want) and len(sd) == 6 * 2 + 5 * 5
    assert [i for i, m in enumerate(model.generator) if isinstance(m, torch.nn.Conv2d)] == [0, 3, 6, 9, 12, 15]
    assert [i for i, m in enumerate(model.generator) if isinstance(m, torch.nn.BatchNorm2d)] == [2, 5, 8, 11, 14]
    assert tuple(sd["generator.0.weight"].shape) == (32, 4, 3, 3) and tuple(sd["generator.15.weight"].shape) == (3, 32, 3, 3)
    assert sd["generator.2.num_batches_tracked"].dtype == torch.long
    assert all(not p.requires_grad for p in model.parameters()) and not model.training
    assert torch.equal(P.RMLineGenerator().state_dict()["generator.6.weight"], sd["generator.6.weight"])  # seeded
    assert set(P.RMLineGenerator(**RC.SMALL_ARCH).state_dict()) == {"generator.0.weight", "generator.0.bias", "generator.2.weight", "generator.2.bias"}
    with pytest.raises(NotImplementedError, match="inference only"):
        model.train()
    assert model.eval() is model
    with pytest.raises(ValueError):
        P.RMLineGenerator(gen_width=65)
    # a Lightning-style checkpoint: {'state_dict' (generator.* and discriminator.*), 'hyper_parameters': {'model': {...}}}
    c = RC.module_case("default", (7, 5))
    path = str(tmp_path / "rmline.ckpt")
    torch.save({"state_dict": c["sd"], "hyper_parameters": {"model": dict(RC.DEFAULT_ARCH, dis_depth=4, lr_gen=0.001)}}, path)
    assert any(k.startswith("discriminator.") for k in c["sd"])
    a = P.RMLineGenerator.from_checkpoint(path)
    b = P.RMLineGenerator().load_checkpoint(path)
    for k, v in a.state_dict().items():
        assert torch.equal(v, c["sd"][k].to(v.dtype)) and torch.equal(v, b.state_dict()[k])
    assert isinstance(P.RMLineWrapper(path).model, P.RMLineGenerator)
    small = str(tmp_path / "small.ckpt")
    torch.save({"state_dict": RC.module_case("small", (7, 5))["sd"], "hyper_parameters": {"model": RC.SMALL_ARCH}}, small)
    assert P.RMLineGenerator.from_checkpoint(small).gen_depth == 2
    with pytest.raises(ValueError, match="gen_depth"):
        P.RMLineGenerator().load_checkpoint(small)
    with pytest.raises(RuntimeError):
        P.RMLineGenerator().load_state_dict({k: v for k, v in c["sd"].items() if k != "generator.5.running_var"})


# ---- the module's host logic on the stand-ins ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", sorted(RC.ARCHS))
def test_module_host_logic_on_stand_ins(P, monkeypatch, arch):
    RC.install_ops(monkeypatch, P.ops)
    for hw in RC.MODULE_SHAPES:
        c = RC.module_case(arch, hw)
        depth = c["arch"]["gen_depth"]
        assert not bool(RC.uncertain(c["img"]).any())
        model = RC.fill_model(P.RMLineGenerator(**c["arch"]), c["sd"])
        wrap = P.RMLineWrapper(model)
        fused, more = wrap(c["img"], face_hull=c["hull"], return_more=True)
        assert model.program().launches == depth + 1
        assert torch.equal(more["line_mask"].double(), c["mask"]) and torch.equal(fused[:, 3], c["img"][:, 3])
        assert RC.module_gate(c["name"] + " (stand-ins)", fused, c["f64"], c["f32"]) == []
        kept = (c["mask"] == 0).expand(-1, 3, -1, -1)
        assert torch.equal(fused[:, :3][kept], more["image"][kept])
        RC.TorchOps.calls.clear()
        layered = wrap(c["img"], face_hull=c["hull"], fused=False)
        assert RC.TorchOps.calls == ["mask"] + ["conv"] * depth and torch.equal(layered, fused)
        one = wrap(c["img"][0], face_hull=c["hull"][0])  # [C,H,W] in, [C,H,W] out
        assert tuple(one.shape) == tuple(c["img"][0].shape) and RC.rel_l2(one, fused[0]) <= 1e-6  # (torch's own convolution differs in the last bits between batch sizes)
        rgb = wrap(RC.composite(c["img"]), face_hull=c["hull"])  # three channels in, three out
        assert tuple(rgb.shape) == (2, 3) + hw and torch.equal(rgb, fused[:, :3])
        out = model(c["x"])
        assert model.program().launches == depth and set(out) == {"image", "line_mask", "face_hull"} and out["face_hull"] is c["x"]["face_hull"]
        assert RC.module_gate(c["name"] + " generator (stand-ins)", out["image"], c["g64"], c["g32"]) == []
        assert torch.equal(model(c["x"], fused=False)["image"], out["image"])
        if min(hw) > 2 * depth:
            assert tuple(model(c["x"], pad=False)["image"].shape) == (2, 3, hw[0] - 2 * depth, hw[1] - 2 * depth)
        else:
            with pytest.raises(ValueError, match="too small"):
                model(c["x"], pad=False)


def test_module_errors_and_the_fold_cache(P, monkeypatch):
    RC.install_ops(monkeypatch, P.ops)
    c = RC.module_case("default", (7, 5))
    model = RC.fill_model(P.RMLineGenerator(**c["arch"]), c["sd"])
    wrap = P.RMLineWrapper(model)
    with pytest.raises(NotImplementedError, match="inference only"):
        wrap(c["img"].clone().requires_grad_(True))
    with torch.no_grad():
        wrap(c["img"].clone().requires_grad_(True))  # nothing is recorded: allowed
    with pytest.raises(ValueError, match="image tensor"):
        wrap(c["img"][:, :2])
    with pytest.raises(RuntimeError, match="float32"):
        wrap(c["img"].double())
    with pytest.raises(ValueError, match="not both"):
        wrap(c["img"][:1], kpts=np.zeros((28, 2)), face_hull=c["hull"][:1])
    with pytest.raises(ValueError, match="one image"):
        wrap(c["img"], kpts=np.zeros((28, 2)))
    with pytest.raises(ValueError, match="face_hull"):
        wrap(c["img"], face_hull=c["hull"][:1])
    with pytest.raises(ValueError, match="face_hull"):
        model.run(RC.composite(c["img"]), c["mask"].float(), None)
    with pytest.raises(ValueError, match="line_mask"):
        model({"image": c["x"]["image"], "line_mask": c["x"]["line_mask"][:, :, :3], "face_hull": c["x"]["face_hull"]})
    with pytest.raises(ValueError, match="taps"):
        P.RMLineWrapper(model, dog=dict(sigma=5.0))
    assert torch.equal(wrap(c["img"]), wrap(c["img"], face_hull=torch.zeros_like(c["hull"])))  # no hull given: an empty one
    # the cached fold and program: reused while nothing changes, re-derived after an in-place write
    f1, p1 = model.folded(), model.program()
    assert model.folded() is f1 and model.program() is p1
    before = wrap(c["img"], face_hull=c["hull"])
    with torch.no_grad():
        model.generator[5].running_var.mul_(4.0)
    f2 = model.folded()
    assert f2 is not f1 and not torch.equal(f2[2][0], f1[2][0]) and torch.equal(f2[1][0], f1[1][0]) and model.program() is not p1
    assert not torch.equal(wrap(c["img"], face_hull=c["hull"]), before)
    model.load_state_dict(model.state_dict())  # copy_ bumps every version
    assert model.folded() is not f2
    prev = P.memo.set_enabled(False)
    try:
        assert model.folded() is not model.folded()
    finally:
        P.memo.set_enabled(prev)


def test_public_operators_refuse_host_tensors(P):
    ops = P.ops
    with pytest.raises(RuntimeError, match="CUDA/ROCm"):
        ops.rmline_mask(torch.zeros(1, 3, 8, 8))
    with pytest.raises(RuntimeError, match="CUDA/ROCm"):
        ops.rmline_conv(torch.zeros(1, 8, 8, 4), torch.zeros(9, 4, 8), torch.zeros(8))
    with pytest.raises(RuntimeError, match="CUDA/ROCm"):
        P.RMLineWrapper(P.RMLineGenerator(**RC.SMALL_ARCH))(torch.rand(1, 3, 8, 8))
    with pytest.raises(ValueError, match="unknown"):
        ops.rmline_dog_params(dict(sigmas=1.0))
    assert ops.rmline_dog_params(dict(d=3))["d"] == 3 and ops.rmline_dog_params()["sigma"] == 0.5


# ---- the face hull ----------------------------------------------------------------------------------------------------------------------
def _kpts(seed, size):
    g = np.random.RandomState(seed)
    k = np.zeros((28, 2))
    k[:11] = g.uniform(8, size - 8, (11, 2))                      # chin, eyelashes
    k[11:17] = np.array([20, 14]) + g.uniform(-5, 5, (6, 2))      # right eye
    k[17:23] = np.array([20, 44]) + g.uniform(-5, 5, (6, 2))      # left eye
    k[23] = (32, 30)                                              # nose
    k[24:28] = np.array([46, 30]) + g.uniform(-6, 6, (4, 2))      # mouth
    return k


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_face_hull_properties(P, seed, monkeypatch):
    size = 64
    k = _kpts(seed, size)
    G = P.rmline.KEYPOINT_GROUPS
    raw = P.face_hull(k, size, dilate=1)[0, 0].numpy() > 0
    full = P.face_hull(k, (size, size))
    assert tuple(full.shape) == (1, 1, size, size) and full.dtype == torch.float32 and set(full.unique().tolist()) == {0.0, 1.0}
    full = full[0, 0].numpy() > 0
    ik = k.astype(int)
    for grp in ("eye_right", "eye_left", "mouth", "nose", "eyelash_left", "eyelash_right"):  # every keypoint pixel that is drawn
        assert all(raw[r, c] for r, c in ik[G[grp]]), grp
    for grp in ("eye_right", "eye_left", "mouth"):  # convex before the dilation: the midpoint pixel of any two hull pixels is in it
        h = P.rmline.convex_hull_mask(ik[G[grp]], (size, size))
        pts = np.argwhere(h)
        assert len(pts) >= 1 and all(h[r, c] for r, c in ik[G[grp]])
        a, b = pts[:, None, :], pts[None, :, :]
        even = ((a + b) % 2 == 0).all(-1)
        mid = ((a + b) // 2)[even]
        assert h[mid[:, 0], mid[:, 1]].all(), grp
        # ... and it is the hull: no pixel outside the keypoints' bounding box
        assert pts.min(0).tolist() == ik[G[grp]].min(0).tolist() and pts.max(0).tolist() == ik[G[grp]].max(0).tolist()
    # degenerate hulls: one point, collinear points
    assert P.rmline.convex_hull_mask([(3, 4)], (8, 8)).sum() == 1 and P.rmline.convex_hull_mask([(1, 1), (3, 3), (5, 5)], (8, 8)).sum() == 5
    # the 5 x 5 dilation grows the bounding box by 2 on each side (the keypoints keep 8 pixels from the border)
    r, f = np.argwhere(raw), np.argwhere(full)
    assert (f.min(0) == r.min(0) - 2).all() and (f.max(0) == r.max(0) + 2).all()
    assert (full >= raw).all() and np.array_equal(full, F.max_pool2d(torch.from_numpy(raw).float()[None, None], 5, 1, 2)[0, 0].numpy() > 0)
    with pytest.raises(ValueError, match="outside"):
        P.face_hull(np.full((28, 2), 70.0), size)
    with pytest.raises(ValueError, match="28"):
        P.face_hull(np.zeros((5, 2)), size)
    # through the wrapper the mask is empty inside the hull
    RC.install_ops(monkeypatch, P.ops)
    wrap = P.RMLineWrapper(P.RMLineGenerator(gen_depth=2, gen_width=4))
    img = RC.smooth_image(1, 4, size, size, seed)
    out, more = wrap(img[0], kpts=k, return_more=True)
    assert tuple(out.shape) == (4, size, size) and float(more["line_mask"].sum()) > 0
    assert torch.equal(more["face_hull"][0, 0] > 0, torch.from_numpy(full)) and float((more["line_mask"] * more["face_hull"]).sum()) == 0


# ---- the gates: the project's operators on binary32 stand-ins of the kernels pass, seeded faults fail ------------------------------------
def test_reference_alone_leaves_out_under_one_percent(P):
    dog = P.ops.rmline_dog_params()  # the detector's defaults of the project ARE the wrapper's
    assert {k: dog[k] for k in RC.DOG_WRAPPER} == RC.DOG_WRAPPER and dog["d"] == 2 and P.RMLineWrapper.DOG == dog
    for hw in RC.MASK_SHAPES:
        for d in (1, 2, 3):
            for img in (RC.smooth_image(2, 3, hw[0], hw[1], 2), RC.smooth_image(2, 4, hw[0], hw[1], 2), RC.flat_image(2, 3, hw[0], hw[1]), RC.flat_image(2, 4, hw[0], hw[1])):
                assert float(RC.uncertain(img, RC.DOG_WRAPPER, d).double().mean()) <= 0.01
    flat = RC.flat_image(1, 3, 9, 33)
    resp = RC.batch_dog(flat.double(), **RC.DOG_WRAPPER)
    assert float((resp[..., :12] - 0.49).abs().max()) <= 1e-15 and float((resp[..., 21:] - 0.49).abs().max()) <= 1e-15  # flat: 0.5 - epsilon
    assert float(RC.line_mask(flat).sum()) > 0  # the edge is a line


@pytest.mark.parametrize("dog", sorted(RC.DOGS))
def test_response_and_mask_stand_ins_pass_and_faults_fail(P, monkeypatch, dog):
    RC.install_ops(monkeypatch, P.ops)
    p = RC.DOGS[dog]
    for hw in RC.RESPONSE_SHAPES:
        for C in (1, 3, 4):
            img = RC.smooth_image(2, C, hw[0], hw[1], 1)
            ref, bound = RC.batch_dog(img.double(), **p), RC.response_bound(img, **p)
            m, image, resp = P.ops.rmline_mask(img, None, dict(p, d=2), want_response=True)
            assert float(((resp.double() - ref).abs() / bound).max()) <= 1.0, (hw, C)
            assert tuple(m.shape) == (2, 1) + hw and (image is None) == (C == 1)
    img, hull = RC.smooth_image(2, 4, 33, 31, 2), RC.make_hull(2, 33, 31)
    assert RC.mask_gate("stand-in", P.ops.rmline_mask(img, hull, dict(p, d=2))[0], img, hull, p, 2, verbose=False) == []
    for fault in ("g0-g1", "zero_pad", "window_forward"):
        bad = RC.line_mask(img, hull, p, 2, fault=fault)
        assert RC.mask_gate(f"[{fault}]", bad, img, hull, p, 2, verbose=False) != [], fault
        if fault != "window_forward":
            r = RC.batch_dog(img.double(), fault=fault, **p)
            assert float(((r - RC.batch_dog(img.double(), **p)).abs() / RC.response_bound(img, **p)).max()) > 1.0, fault
    assert RC.mask_gate("[no hull]", P.ops.rmline_mask(img, None, dict(p, d=2))[0], img, hull, p, 2, verbose=False) != []


@pytest.mark.parametrize("chans", RC.CONV_CHANNELS)
def test_layer_stand_in_passes_and_faults_fail(P, monkeypatch, chans):
    RC.install_ops(monkeypatch, P.ops)
    for H, W in RC.CONV_SHAPES:
        c = RC.conv_case(chans[0], chans[1], H, W)
        run = lambda act, slope=c["slope"], w=c["w"]: P.ops.rmline_conv(RC.nhwc(c["x"]), RC.to_wk(w), c["b"], act, slope, planar=True)
        for act in sorted(RC.ACTS):
            assert RC.conv_gate(c["name"], run(act), c, act, verbose=False) == []
            assert torch.equal(RC.nchw(P.ops.rmline_conv(RC.nhwc(c["x"]), RC.to_wk(c["w"]), c["b"], act, c["slope"])), run(act))
        assert RC.conv_gate(c["name"] + " [slope 0.2]", run("leaky", slope=0.2), c, "leaky", verbose=False) != []
        assert RC.conv_gate(c["name"] + " [no act]", run("none"), c, "tanh", verbose=False) != []
        assert RC.conv_gate(c["name"] + " [taps transposed]", run("none", w=c["w"].transpose(2, 3)), c, "none", verbose=False) != []


def test_module_gate_catches_seeded_faults(P, monkeypatch):
    RC.install_ops(monkeypatch, P.ops)
    c = RC.module_case("default", (37, 41))
    arch, seq = c["arch"], c["seq"]
    model = RC.fill_model(P.RMLineGenerator(**arch), c["sd"])
    assert RC.module_gate("wrapper (stand-ins)", P.RMLineWrapper(model)(c["img"], face_hull=c["hull"]), c["f64"], c["f32"], verbose=False) == []
    assert RC.module_gate("generator (stand-ins)", model(c["x"])["image"], c["g64"], c["g32"], verbose=False) == []
    swapped, _ = RC.wrapper_forward(seq, c["img"], c["hull"], arch, dtype=torch.float32, fault="lerp_swapped")
    assert RC.module_gate("[lerp swapped]", swapped, c["f64"], c["f32"], verbose=False) != []
    x64 = {k: v.double() for k, v in c["x"].items()}
    with torch.no_grad():
        zero = RC.model_forward(seq, x64, arch, fault="zero_pad")["image"]
        seq[1].negative_slope = 0.2
        slope = RC.model_forward(seq, x64, arch)["image"]
        seq[1].negative_slope = 0.01
        # the batch norm folded on the wrong side of the activation: conv -> BN -> LeakyReLU for the first block
        mods = list(seq)
        mods[1], mods[2] = mods[2], mods[1]
        wrong = RC.model_forward(torch.nn.Sequential(*mods), x64, arch)["image"]
    for name, bad in (("zero padding", zero), ("slope 0.2", slope), ("batch norm before the activation", wrong)):
        assert RC.module_gate(f"[{name}]", bad, c["g64"], c["g32"], verbose=False) != [], name
    # a fault seeded under the project's own path: the stand-in of the layer kernel with slope 0.2
    monkeypatch.setattr(RC.TorchOps, "conv", staticmethod(lambda *a, _c=RC.TorchOps.conv: _c(*a, fault="slope")))
    assert RC.module_gate("[slope 0.2 in the operator]", model(c["x"])["image"], c["g64"], c["g32"], verbose=False) != []
