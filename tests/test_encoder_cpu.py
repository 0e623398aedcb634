"""CPU (-m "not gpu"): the conditioning encoder without a device — the C ABI (include/p3d_encoder.h, _lib.ENCODER_SIGNATURES and the
library's exports; argument errors come back before any launch), the host-side plan of every layer of the real network, the batch-norm
and PCA folds against the unfolded float64 forms, the state-dict names, the restatements and gates that tests/test_hip_encoder.py holds
the kernels to (the binary32 stand-ins pass them, seeded faults fail them), and the host logic of panic3d_amd/encoder.py on torch
stand-ins of the operators.  On the parent commit the module, the table and the symbols do not exist."""
import ctypes
import os
import re

import pytest
import torch

import encoder_cases as EC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = torch.nn.functional


@pytest.fixture(scope="module")
def P():
    import panic3d_amd
    panic3d_amd.build()
    return panic3d_amd


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_encoder_header_table_and_exports_agree(P):
    hdr = open(os.path.join(ROOT, "include", "p3d_encoder.h")).read()
    declared = set(re.findall(r"\b(p3d_enc[a-z0-9_]+)\s*\(", hdr)) - {"p3d_enc_layer"}
    lib = P._lib
    assert declared == set(lib.ENCODER_SIGNATURES) and len(declared) == 8
    others = set(lib.SIGNATURES) | set(lib.GRAD_SIGNATURES) | set(lib.SYN_GRAD_SIGNATURES) | set(lib.PASTE_GRAD_SIGNATURES) | set(lib.DISC_SIGNATURES) \
        | set(lib.LOSS_SIGNATURES) | set(lib.OPTIM_SIGNATURES) | set(lib.LPIPS_SIGNATURES)
    assert not declared & others
    L = lib.lib()
    for name in declared:
        assert hasattr(L, name)
    B = P._build
    assert "p3d_encoder.hip" in B.SOURCES and os.path.join("..", "..", "include", "p3d_encoder.h") in B.HEADERS and "p3d_encoder_plan.hpp" in B.HEADERS
    for unit in (B.RENDER_UNIT, B.SYNTHESIS_UNIT):
        assert not any("p3d_encoder" in s for s in unit)
    for name in ("KC", "CUS", "TILE_64", "TILE_32", "MAX_SPLIT", "RELU", "KIND_CONV", "KIND_MAXPOOL", "KIND_PREPARE"):
        assert int(re.search(rf"#define P3D_ENC_{name} (\d+)", hdr).group(1)) == getattr(lib, f"P3D_ENC_{name}")
    assert lib.P3D_ABI_VERSION == 9 and L.p3d_abi_version() == 9
    src = open(os.path.join(B.CSRC, "p3d_encoder.hip")).read()
    assert "mfma_f32_16x16x4f32" in src and "atomic" not in src.replace("with atomics", "")
    # the record's ctypes mirror against the compiled struct (lib() checks it on load; here: it bites)
    buf = (ctypes.c_size_t * 64)()
    n = L.p3d_enc_struct_layout(buf, 64)
    assert n == 19 and buf[0] == ctypes.sizeof(lib.EncLayer) == 80
    assert L.p3d_enc_struct_layout(buf, 3) == -2 and L.p3d_enc_struct_layout(None, 64) == -1
    assert P.ResNetEncoder is P.encoder.ResNetEncoder and P.ResnetFeatureExtractorPCA is P.encoder.ResnetFeatureExtractorPCA


def test_encoder_argument_errors_without_gpu(P):
    L = P._lib.lib()
    p = 256  # never dereferenced: the checks come first

    def conv(x=p, N=2, Ci=8, H=6, W=5, wk=p, k=3, stride=1, Co=8, bias=p, res=None, flags=1, out=p, plan=0, ws=p, nbytes=1 << 20):
        return L.p3d_enc_conv_f32(x, N, Ci, H, W, wk, k, stride, Co, bias, res, flags, out, plan, ws, nbytes, None)
    assert conv(x=None) == -1 and conv(wk=None) == -1 and conv(bias=None) == -1 and conv(out=None) == -1
    assert conv(N=0) == -1 and conv(Ci=0) == -1 and conv(Co=0) == -1 and conv(H=0) == -1
    assert conv(k=5) == -2 and conv(k=2) == -2 and conv(stride=3) == -2 and conv(stride=0) == -2 and conv(flags=2) == -2
    assert conv(plan=3 << 8 | 1) == -2 and conv(plan=1 << 8) == -2 and conv(plan=-1) == -2
    # a split needs its workspace: K = 72 is two chunks
    need = L.p3d_enc_conv_workspace_bytes(2, 8, 8, 6, 5, 3, 1, 1 << 8 | 2)
    assert need == 2 * 2 * 8 * 6 * 5 * 4 and L.p3d_enc_conv_workspace_bytes(2, 8, 8, 6, 5, 3, 1, 1 << 8 | 1) == 0
    assert conv(plan=1 << 8 | 2, nbytes=need - 1) == -3 and conv(plan=1 << 8 | 2, ws=None) == -1
    assert L.p3d_enc_conv_workspace_bytes(2, 8, 8, 6, 5, 5, 1, 0) == 0  # refused sizes

    pool = lambda x=p, planes=4, H=7, W=7, y=p: L.p3d_enc_maxpool_f32(x, planes, H, W, y, None)
    assert pool(x=None) == -1 and pool(y=None) == -1 and pool(planes=0) == -1 and pool(H=0) == -1 and pool(planes=1 << 40) == -2

    def prep(img=p, N=1, C=4, H=12, W=16, mean=p, std=p, h=8, w=10, out=p):
        return L.p3d_enc_prepare_f32(img, N, C, H, W, mean, std, h, w, out, None)
    assert prep(img=None) == -1 and prep(mean=None) == -1 and prep(std=None) == -1 and prep(out=None) == -1 and prep(N=0) == -1 and prep(h=0) == -1
    assert prep(C=2) == -2 and prep(H=1 << 22) == -2 and prep(w=1 << 22) == -2


def _table(P, recs):
    lib = P._lib
    tab = (lib.EncLayer * len(recs))()
    for t, r in zip(tab, recs):
        for k, v in r.items():
            setattr(t, k, v)
    return tab


def test_forward_table_is_checked_before_any_launch(P):
    lib = P._lib
    L = lib.lib()
    p = 256
    conv = dict(kind=0, N=2, Ci=8, H=6, W=5, Co=8, Ho=6, Wo=5, k=3, stride=1, in_=0, out=1, res=-1, flags=1, plan=0, w_off=0, b_off=576)
    pool = dict(kind=1, N=2, Ci=8, H=6, W=5, Co=8, Ho=3, Wo=3, in_=1, out=0, res=-1)
    off, ln = (ctypes.c_int64 * 2)(0, 512), (ctypes.c_int64 * 2)(480, 480)

    def run(recs, weights=p, wf=584, arena=p, af=992, off=off, ln=ln, nb=2, ws=p, nbytes=1 << 20):
        return L.p3d_encoder_forward_f32(_table(P, recs), len(recs), weights, wf, arena, af, off, ln, nb, ws, nbytes, None)
    ok = [conv, pool]
    assert run(ok, weights=None) == -1 and run(ok, arena=None) == -1 and run(ok, off=None) == -1 and run(ok, nb=0) == -1
    assert L.p3d_encoder_forward_f32(None, 2, p, 584, p, 992, off, ln, 2, p, 0, None) == -1
    # every one of these is the LAST record's fault, or a later one's: nothing may have been launched for the records before it
    # (pointer 256 would fault the process if anything were)
    bad = lambda **kw: [conv, dict(pool, **kw)]
    assert run(bad(kind=7)) == -2 and run(bad(in_=2)) == -2 and run(bad(out=-1)) == -2 and run(bad(in_=0, out=0)) == -2
    assert run(bad(Ho=4)) == -2 and run(bad(Co=9)) == -2 and run(bad(res=0)) == -2 and run(bad(reserved=1)) == -2
    assert run([conv, dict(conv, in_=1, out=0, Ho=5)]) == -2 and run([conv, dict(conv, in_=1, out=0, res=0)]) == -2  # res == out
    assert run([conv, dict(conv, in_=1, out=0, b_off=577)]) == -2 and run([conv, dict(conv, in_=1, out=0, w_off=-1)]) == -2
    assert run([conv, dict(conv, in_=1, out=0, k=5)]) == -2 and run([conv, dict(conv, in_=1, out=0, N=3)]) == -2  # N = 3: the buffer is too short
    assert run(ok, af=991) == -2 and run(ok, wf=583) == -2
    split = dict(conv, plan=1 << 8 | 2)
    need = L.p3d_encoder_workspace_bytes(_table(P, [conv, split]), 2)
    assert need == 2 * 480 * 4 and L.p3d_encoder_workspace_bytes(_table(P, [dict(conv, plan=1 << 8 | 1)]), 1) == 0
    assert run([pool, dict(split, in_=0, out=1)], nbytes=need - 1) == -3 and run([pool, dict(split, in_=0, out=1)], ws=None) == -1
    assert L.p3d_encoder_workspace_bytes(_table(P, [dict(conv, k=4)]), 1) == 0


def test_public_operators_check_before_any_launch(P):
    ops = P.ops
    with pytest.raises(RuntimeError, match="CUDA/ROCm"):
        ops.enc_maxpool(torch.zeros(1, 1, 7, 7))
    with pytest.raises(RuntimeError, match="CUDA/ROCm"):
        ops.enc_conv(torch.zeros(1, 2, 4, 4), torch.zeros(1, 2, 3), torch.zeros(3), 1)
    with pytest.raises(RuntimeError, match="CUDA/ROCm"):
        ops.enc_prepare(torch.zeros(1, 3, 8, 8), torch.zeros(3), torch.zeros(3), 4)
    with pytest.raises(RuntimeError, match="CUDA/ROCm"):  # the real impls refuse host tensors themselves: a host pointer never reaches a kernel
        P.ResNetEncoder(**EC.TINY)(torch.rand(1, 3, 32, 32), size=32)
    with pytest.raises(ValueError, match="k 5"):
        ops._enc_out_hw(8, 8, 5, 1)
    assert ops._enc_out_hw(9, 7, 1, 2) == (5, 4) and ops._enc_out_hw(20, 18, 7, 2) == (10, 9) and ops._enc_out_hw(8, 8, 3, 2) == (4, 4)
    assert ops.enc_resize_hw(512, 512, 256) == (256, 256) and ops.enc_resize_hw(40, 36, 32) == (35, 32) and ops.enc_resize_hw(5, 6, 8) == (8, 9)
    assert ops.enc_resize_hw(12, 16, 8) == EC.resize_hw(12, 16, 8) == (8, 10)


# ---- the plan -------------------------------------------------------------------------------------------------------------------------
def test_plan_fills_the_chip_for_every_layer_of_the_real_network(P):
    """ResNet-50 at batch 2 x 256^2: every convolution gets a plan; the documented fill condition holds — at least 256 workgroups
    wherever tile-32 tiles x chunks >= 256, else tile 32 with one chunk per split; the workspace is what the split asks for."""
    enc = P.ResNetEncoder()
    enc.set_pca(torch.zeros(512, 2048), torch.zeros(2048))
    recs, buf_len, outputs = enc.records((1, 3, 512, 512), 256, ("pca",))
    convs = [r for r in recs if r["kind"] == "conv"]
    assert len(convs) == 54 and len(recs) == 56  # 53 convolutions of the network + the PCA layer; the front end and the pool
    assert outputs["pca"][1] == (2, 512, 8, 8)
    kinds = set()
    for r in convs:
        (N, Ci, H, W), (_, Co, Ho, Wo), k, s = r["shape"], r["out_shape"], r["k"], r["stride"]
        pl = P.ops.enc_conv_plan(N, Ci, Co, Ho, Wo, k, s)
        chunks = -(-k * k * Ci // 64)
        pt = -(-N * Ho * Wo // 64)
        t32 = -(-Co // 32) * pt
        tm = 64 if pl["tile"] == 1 else 32
        assert pl["code"] == pl["tile"] << 8 | pl["split"] and pl["tile"] in (1, 2)
        assert pl["workgroups"] == -(-Co // tm) * pt * pl["split"]
        assert pl["split"] == -(-chunks // pl["cps"]) and (pl["split"] - 1) * pl["cps"] < chunks  # no empty split
        if t32 * chunks >= 256:
            assert pl["workgroups"] >= 256, (r["name"], pl)
        else:
            assert pl["tile"] == 2 and pl["cps"] == 1 and pl["split"] == chunks, (r["name"], pl)
        assert pl["workspace_bytes"] == (pl["split"] * N * Co * Ho * Wo * 4 if pl["split"] > 1 else 0)
        kinds.add((pl["tile"], pl["split"] > 1))
    assert kinds >= {(1, False), (2, False), (1, True)}, kinds  # the real network exercises rules 1, 2 and 3
    # a forced plan is clipped to the chunk count, and 255 splits is the most
    assert P.ops.enc_conv_plan(2, 64, 64, 4, 4, 1, 1, 2 << 8 | 255)["split"] == 1
    big = P.ops.enc_conv_plan(1, 4096, 64, 1, 1, 3, 1, 1 << 8 | 255)
    assert big["split"] <= 255 and big["cps"] == 3 and big["split"] == 192


# ---- the folds and the names ----------------------------------------------------------------------------------------------------------
def test_state_dict_names_and_counts(P):
    full = P.ResNetEncoder(num_classes=1000)
    sd = full.state_dict()
    assert len(sd) == 320 and sum(p.numel() for p in full.parameters()) == 25557032
    want = set(EC.make_weights(num_classes=1000, **EC.FULL))
    assert set(sd) == want
    assert tuple(sd["conv1.weight"].shape) == (64, 3, 7, 7) and tuple(sd["layer4.0.downsample.0.weight"].shape) == (2048, 1024, 1, 1)
    assert tuple(sd["layer2.0.conv2.weight"].shape) == (128, 128, 3, 3) and full.layer2[0].stride == 2 and full.layer2[1].stride == 1
    assert "layer1.0.downsample.0.weight" in sd and "layer1.1.downsample.0.weight" not in sd
    assert sd["bn1.num_batches_tracked"].dtype == torch.long and tuple(sd["fc.weight"].shape) == (1000, 2048)
    assert all(not p.requires_grad for p in full.parameters())
    assert "fc.weight" not in P.ResNetEncoder(**EC.TINY).state_dict()
    tiny = EC.fill_model(P.ResNetEncoder(**EC.TINY), EC.make_weights(pca_dim=16, **EC.TINY))
    assert tuple(tiny.pca_weights.shape) == (1, 16, 256) and tuple(tiny.pca_mean.shape) == (1, 256)
    assert {"pca_weights", "pca_mean"} <= set(tiny.state_dict())


def test_torchvision_agrees_when_present(P, monkeypatch):
    tv = pytest.importorskip("torchvision")
    EC.install_ops(monkeypatch, P.ops)
    ref = tv.models.resnet50(weights=None).eval()
    ours = P.ResNetEncoder(num_classes=1000)
    assert list(ours.state_dict()) == list(ref.state_dict()) or set(ours.state_dict()) == set(ref.state_dict())
    sd = EC.make_weights(num_classes=1000, **EC.FULL)
    ref.load_state_dict(sd)
    EC.fill_model(ours, sd)
    img = EC.make_image((1, 3, 64, 64), 3)
    x = EC.prepare(img, 64)
    with torch.no_grad():
        y = ref.layer4(ref.layer3(ref.layer2(ref.layer1(ref.maxpool(ref.relu(ref.bn1(ref.conv1(x))))))))
    assert EC.rel_l2(ours(img, size=64)["layer4"], y) <= 1e-4


def test_folds_against_the_unfolded_forms_in_float64(P):
    enc = P.encoder
    g = torch.Generator().manual_seed(3)
    for Ci, Co, k, stride in ((5, 7, 3, 2), (3, 4, 7, 2), (9, 6, 1, 1)):
        sd = EC.make_weights(**EC.TINY, seed=k)
        conv, bn = enc._Conv(Ci, Co, k).double(), enc._BN(Co).double()
        with torch.no_grad():
            conv.weight.copy_(torch.randn(Co, Ci, k, k, generator=g, dtype=torch.float64))
            bn.weight.copy_(sd["bn1.weight"][:Co]), bn.bias.copy_(sd["bn1.bias"][:Co])
            bn.running_mean.copy_(sd["bn1.running_mean"][:Co]), bn.running_var.copy_(sd["bn1.running_var"][:Co])
        x = torch.randn(2, Ci, 9, 8, generator=g, dtype=torch.float64)
        want = F.batch_norm(F.conv2d(x, conv.weight, stride=stride, padding=(k - 1) // 2), bn.running_mean, bn.running_var, bn.weight, bn.bias, False, 0.0, 1e-5)
        # the fold itself, before its one rounding: restated here in float64 from the documented formula
        s = bn.weight / torch.sqrt(bn.running_var + 1e-5)
        got64 = F.conv2d(x, conv.weight * s.view(-1, 1, 1, 1), bn.bias - bn.running_mean * s, stride=stride, padding=(k - 1) // 2)
        assert EC.rel_l2(got64, want) <= 1e-12
        # fold_bn: those numbers rounded once to binary32, in the wk layout
        wk, b = enc.fold_bn(conv.weight, bn)
        assert wk.dtype == b.dtype == torch.float32 and tuple(wk.shape) == (k * k, Ci, Co)
        assert torch.equal(wk, EC.to_wk((conv.weight * s.view(-1, 1, 1, 1))).float()) and torch.equal(b, (bn.bias - bn.running_mean * s).float())
    # the PCA: pw @ (feat - mean) as a 1 x 1 convolution with bias -pw mean
    pw, mean = torch.randn(6, 10, generator=g, dtype=torch.float64), torch.randn(10, generator=g, dtype=torch.float64)
    feat = torch.randn(2, 10, 3, 4, generator=g, dtype=torch.float64)
    want = (pw[None][:, None, None] @ (feat - mean[None][..., None, None]).permute(0, 2, 3, 1)[..., None]).squeeze(-1).permute(0, 3, 1, 2)
    got64 = F.conv2d(feat, pw.view(6, 10, 1, 1), -(pw @ mean))
    assert EC.rel_l2(got64, want) <= 1e-12
    wk, b = enc.fold_pca(pw, mean)
    assert tuple(wk.shape) == (1, 10, 6) and torch.equal(wk[0], pw.t().float()) and torch.equal(b, (-(pw @ mean)).float())


# ---- the gates: the binary32 stand-ins pass, seeded faults fail -------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(EC.CONV_CASES))
def test_conv_stand_in_passes_and_faults_fail(name):
    c = EC.conv_case(name)
    ref = EC.conv_ref(c)
    assert EC.conv_gate(EC.run_conv(EC.TorchOps, c, "cpu"), ref, c) == []
    faults = ["bias_per_split"] + (["no_res"] if c["res"] is not None else [])
    for fault in faults:
        bad = EC.conv_ref(c, torch.float32, fault=fault)["y"]
        assert EC.conv_gate(bad, ref, c, f" [{fault}]") != [], (name, fault)


@pytest.mark.parametrize("shape", EC.POOL_SHAPES)
def test_pool_zero_padding_fails_on_the_negative_input(shape):
    c = EC.pool_case(*shape)
    Ho, Wo = (shape[1] - 1) // 2 + 1, (shape[2] - 1) // 2 + 1
    for key in ("x", "neg"):
        y = EC.maxpool(c[key])
        assert tuple(y.shape) == (2, shape[0], Ho, Wo) and torch.isfinite(y).all()
    assert not torch.equal(EC.maxpool(c["neg"], fault="zero_pad"), EC.maxpool(c["neg"]))
    relu = F.relu(c["x"])  # what the network feeds the pool: zero padding cannot be seen there
    assert torch.equal(EC.maxpool(relu, fault="zero_pad"), EC.maxpool(relu))


@pytest.mark.parametrize("hw,size", EC.PREPARE_CASES)
def test_prepare_stand_in_passes_and_an_unmirrored_row_fails(hw, size):
    c = EC.prepare_case(hw, size)
    mean, std = (v.flatten() for v in EC.norm_consts(torch.float32))
    got = EC.TorchOps.enc_prepare(c["img"], mean, std, size)
    h, w = EC.resize_hw(hw[0], hw[1], size)
    assert tuple(got.shape) == (4, 3, h, w)
    assert EC.prepare_gate(f"prepare {hw}->{size}", got, c["img"], size) == []
    bad = torch.cat([got[:2], got[:2]])  # the mirror rows not mirrored
    assert EC.prepare_gate(f"[unmirrored] prepare {hw}->{size}", bad, c["img"], size) != []
    shifted = EC.TorchOps.enc_prepare(c["img"].roll(1, 1), mean, std, size)  # the fourth channel read as the first
    assert EC.prepare_gate(f"[channel] prepare {hw}->{size}", shifted, c["img"], size) != []


# ---- the module's host logic on the stand-ins -------------------------------------------------------------------------------------------
def test_network_host_logic_on_stand_ins(P, monkeypatch):
    EC.install_ops(monkeypatch, P.ops)
    c = EC.network_case("tiny")
    model = EC.fill_model(P.ResNetEncoder(**c["arch"]), c["sd"])
    feats = EC.STAGES + ("pca",)
    fused = model(c["img"], size=c["size"], features=feats)
    assert set(fused) == set(feats)
    assert tuple(fused["conv1"].shape) == (4, 8, 18, 16) and tuple(fused["layer4"].shape) == (4, 256, 2, 1) and tuple(fused["pca"].shape) == (4, 16, 2, 1)
    assert EC.network_gate("tiny (stand-ins)", fused, c) == []
    layered = model(c["img"], size=c["size"], features=feats, fused=False)
    assert all(torch.equal(fused[k], layered[k]) for k in feats)  # the table walk and the layer-by-layer calls: the same operands in the same order
    # rows N..2N-1 are the mirrored image's: the network of the flipped image gives them as its rows 0..N-1
    flipped = model(c["img"].flip(dims=(-1,)), size=c["size"], features=("layer2",))["layer2"]
    assert EC.rel_l2(flipped[:2], fused["layer2"][2:]) <= 1e-5 and EC.rel_l2(flipped[:2], fused["layer2"][:2]) > 1e-2
    # features= selects, and stops the walk after the last stage asked for
    only = model(c["img"], size=c["size"], features=("layer1", "conv1"))
    assert set(only) == {"layer1", "conv1"} and torch.equal(only["layer1"], fused["layer1"]) and torch.equal(only["conv1"], fused["conv1"])
    recs, _, _ = model.records(c["img"].shape, c["size"], ("layer1",))
    assert [r["name"] for r in recs][-1] == "layer1.0.conv3" and len(recs) == 2 + 1 + 4
    assert len(model.records(c["img"].shape, c["size"], ("conv1",))[0]) == 2
    # seeded fault of the whole network: a dropped residual fails the network gate
    monkeypatch.setattr(P.ops, "_enc_conv_impl", lambda x, wk, b, k, s, res, relu, plan: EC.TorchOps.enc_conv(x, wk, b, k, s, res, relu, fault="no_res"))
    broken = model(c["img"], size=c["size"], features=("layer4",), fused=False)
    assert EC.network_gate("[no_res] tiny", broken, c, verbose=False) != []


def test_network_errors_and_the_fold_cache(P, monkeypatch):
    EC.install_ops(monkeypatch, P.ops)
    c = EC.network_case("tiny")
    model = EC.fill_model(P.ResNetEncoder(**c["arch"]), c["sd"])
    with pytest.raises(NotImplementedError, match="inference only"):
        model(c["img"].clone().requires_grad_(True), size=32)
    with torch.no_grad():
        model(c["img"].clone().requires_grad_(True), size=32)  # nothing is recorded: allowed
    with pytest.raises(ValueError, match="features"):
        model(c["img"], size=32, features=("layer5",))
    with pytest.raises(ValueError, match="set_pca"):
        P.ResNetEncoder(**EC.TINY)(c["img"], size=32, features=("pca",))
    with pytest.raises(ValueError, match="image batch"):
        model(c["img"][:, :2], size=32)
    with pytest.raises(RuntimeError, match="float32"):
        model(c["img"].double(), size=32)
    with pytest.raises(ValueError, match="set_pca"):
        model.set_pca(torch.zeros(4, 7), torch.zeros(7))
    # the cached fold and programs: reused while nothing changes, re-derived after an in-place write
    f1 = model.folded()
    p1 = model.program(c["img"].shape, 32, ("layer4",))
    assert model.folded() is f1 and model.program(c["img"].shape, 32, ("layer4",)) is p1
    before = model(c["img"], size=32)["layer4"]
    with torch.no_grad():
        model.layer2[1].bn2.running_var.mul_(4.0)
    f2 = model.folded()
    assert f2 is not f1 and not torch.equal(f2["layer2.1.conv2"][0], f1["layer2.1.conv2"][0]) and torch.equal(f2["layer1.0.conv1"][0], f1["layer1.0.conv1"][0])
    assert model.program(c["img"].shape, 32, ("layer4",)) is not p1
    assert not torch.equal(model(c["img"], size=32)["layer4"], before)
    model.load_state_dict(model.state_dict())  # copy_ bumps every version
    assert model.folded() is not f2
    prev = P.memo.set_enabled(False)
    try:
        assert model.folded() is not model.folded()
    finally:
        P.memo.set_enabled(prev)


class _Image:
    """The reference's image class as far as katepca.py:20 uses it."""

    def __init__(self, t):
        self._t = t

    def bg(self, colour):
        assert colour == "k"
        return self

    def t(self):
        return self._t


def test_feature_extractor_host_logic(P, monkeypatch):
    EC.install_ops(monkeypatch, P.ops)
    c = EC.network_case("tiny")
    rfe = P.ResnetFeatureExtractorPCA(None, 16, size=c["size"], **c["arch"])
    assert rfe.fn_features is None and rfe.dim_out == 16 and isinstance(rfe.rfe, P.ResNetEncoder) and not rfe.rfe.training
    assert P.ResnetFeatureExtractorPCA(None, 512).size == 256
    with pytest.raises(ValueError, match="set_pca"):
        rfe(c["img"][0])
    # the tagger's checkpoint keeps the network under 'resnet.'; other entries are ignored, a missing one raises
    ck = {f"resnet.{k}": v for k, v in c["sd"].items() if not k.startswith("pca.")}
    ck["other.weight"] = torch.zeros(3)
    rfe.load_tagger(ck)
    with pytest.raises(KeyError, match="missing"):
        rfe.load_tagger({k: v for k, v in ck.items() if k != "resnet.layer3.0.bn2.running_var"})
    with pytest.raises(ValueError, match="at least 16"):
        rfe.set_pca(c["sd"]["pca.components"][:8], c["sd"]["pca.mean"])
    more = torch.cat([c["sd"]["pca.components"], torch.ones(3, 256)])
    rfe.set_pca(more.numpy(), c["sd"]["pca.mean"].numpy())  # arrays; the first dim_out components are kept
    assert tuple(rfe.rfe.pca_weights.shape) == (1, 16, 256) and tuple(rfe.rfe.pca_mean.shape) == (1, 256)
    want = {k: v[[0, 2]] for k, v in c["f64"].items()}  # the first image of the case's batch of two, and its mirror
    one = dict(c, f64={"pca": want["pca"]}, f32={"pca": c["f32"]["pca"][[0, 2]]})
    for img in (c["img"][0], c["img"][:1], _Image(c["img"][0])):
        out = rfe(img)
        assert tuple(out.shape) == (2, 16, 2, 1)
        assert EC.network_gate("extractor", {"pca": out}, one, verbose=False) == []
    with pytest.raises(ValueError, match="one image"):
        rfe(c["img"])
    with pytest.raises(NotImplementedError, match="inference only"):
        rfe(c["img"][0].clone().requires_grad_(True))
