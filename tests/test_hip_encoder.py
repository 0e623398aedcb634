"""GPU (-m gpu): the conditioning encoder on the HIP kernels (include/p3d_encoder.h, panic3d_amd/encoder.py).  Stage level: every kernel
on the binary32 inputs of the float64 restatement (tests/encoder_cases.py) under the project's gates — the convolution per value
8 sqrt(K) 2^-24 sum|terms| with K = Ci k^2 plus the bias and the residual, rel-L2 <= 1e-5, under EVERY plan (both tiles; no split, two,
as many as there are chunks) and two runs give the same bits; the pool bit-equal to F.max_pool2d, on an all-negative input too; the
front end per value 4 2^-24 sum|terms| against the float64 resize of the image and of its mirror.  Whole network: per feature
rel-L2(ours, f64) <= 4 rel-L2(torch binary32 of the same restatement on the CPU, f64); the one-call table walk gives the bits of the
layer-by-layer operators.  End to end: the extractor's output as `resnet_chonk` of G.f.  The gates' sensitivity to seeded faults is
shown on CPU in tests/test_encoder_cpu.py.  On the parent commit the module, the operators and the symbols do not exist."""
import pytest
import torch

import encoder_cases as EC

pytestmark = pytest.mark.gpu
F = torch.nn.functional


@pytest.fixture(scope="module")
def P():
    import panic3d_amd
    panic3d_amd.build()
    panic3d_amd._lib.lib()
    return panic3d_amd


@pytest.mark.parametrize("name", sorted(EC.CONV_CASES))
def test_conv_under_every_plan(P, name):
    c = EC.conv_case(name)
    ref = EC.conv_ref(c)
    bad, seen = [], set()
    N, Ci, H, W = c["x"].shape
    Ho, Wo = ref["y"].shape[2:]
    for plan in EC.PLANS:
        pl = P.ops.enc_conv_plan(N, Ci, c["w"].shape[0], Ho, Wo, c["k"], c["stride"], plan)
        seen.add((pl["tile"], pl["split"]))
        a, b = EC.run_conv(P.ops, c, "cuda", plan), EC.run_conv(P.ops, c, "cuda", plan)
        assert torch.equal(a, b), f"two runs differ under plan {plan:#x}"
        bad += EC.conv_gate(a.cpu(), ref, c, f" plan {plan:#x} (tile {pl['tile']}, split {pl['split']})")
    assert bad == []
    assert {t for t, _ in seen} == {1, 2}
    if Ci * c["k"] ** 2 > 64:
        assert max(s for _, s in seen) == -(-Ci * c["k"] ** 2 // 64) and (1, 1) in seen and (2, 1) in seen  # the splits were real ones


@pytest.mark.parametrize("shape", EC.POOL_SHAPES)
def test_maxpool_is_torchs_bit_for_bit(P, shape):
    c = EC.pool_case(*shape)
    for key in ("x", "neg"):  # 'neg': all negative, so that a padding cell counted as 0 would win
        y = P.ops.enc_maxpool(c[key].cuda())
        assert torch.equal(y.cpu(), F.max_pool2d(c[key], 3, 2, 1)), key
        assert torch.equal(P.ops.enc_maxpool(c[key].cuda()), y)


@pytest.mark.parametrize("hw,size", EC.PREPARE_CASES)
def test_prepare_against_the_float64_resize(P, hw, size):
    c = EC.prepare_case(hw, size)
    mean, std = (v.flatten().cuda() for v in EC.norm_consts(torch.float32))
    got = P.ops.enc_prepare(c["img"].cuda(), mean, std, size)
    assert tuple(got.shape) == (4, 3) + EC.resize_hw(hw[0], hw[1], size)
    assert EC.prepare_gate(f"prepare {hw}->{size}", got.cpu(), c["img"], size) == []
    assert torch.equal(P.ops.enc_prepare(c["img"].cuda(), mean, std, size), got), "two runs differ"


def test_public_operators_check_their_arguments(P):
    z = lambda *s: torch.zeros(*s, device="cuda")
    with pytest.raises(ValueError):
        P.ops.enc_conv(z(1, 3, 8, 8), z(25, 3, 8), z(8), 5)            # k
    with pytest.raises(ValueError):
        P.ops.enc_conv(z(1, 3, 8, 8), z(9, 4, 8), z(8), 3)             # wk's channels
    with pytest.raises(ValueError):
        P.ops.enc_conv(z(1, 3, 8, 8), z(9, 3, 8), z(7), 3)             # bias
    with pytest.raises(ValueError):
        P.ops.enc_conv(z(1, 3, 8, 8), z(9, 3, 8), z(8), 3, 2, z(1, 8, 8, 8))  # the residual has the OUTPUT's shape
    with pytest.raises(RuntimeError):
        P.ops.enc_conv(z(1, 3, 8, 8), z(9, 3, 8), z(8), 3, force_plan=3 << 8 | 1)
    with pytest.raises(ValueError):
        P.ops.enc_prepare(z(1, 2, 8, 8), z(3), z(3), 4)
    with pytest.raises(ValueError):
        P.ops.enc_maxpool(z(3, 8, 8))


@pytest.mark.parametrize("name", sorted(EC.NETWORK_CASES))
def test_whole_network(P, name):
    c = EC.network_case(name)
    model = EC.fill_model(P.ResNetEncoder(**c["arch"]), c["sd"]).cuda()
    feats = EC.STAGES + ("pca",)
    img = c["img"].cuda()
    fused = model(img, size=c["size"], features=feats)
    assert all(torch.isfinite(v).all() for v in fused.values())
    assert EC.network_gate(name, fused, c) == []
    layered = model(img, size=c["size"], features=feats, fused=False)
    assert all(torch.equal(fused[k], layered[k]) for k in feats), "the table walk and the layer-by-layer operators differ"
    again = model(img, size=c["size"], features=feats)
    assert all(torch.equal(fused[k], again[k]) for k in feats), "two runs differ"
    if name == "full-128":
        assert tuple(fused["layer4"].shape) == (2, 2048, 4, 4) and tuple(fused["pca"].shape) == (2, 512, 4, 4)
    only = model(img, size=c["size"], features=("layer2",))
    assert set(only) == {"layer2"} and torch.equal(only["layer2"], fused["layer2"])


def test_network_argument_errors(P):
    model = P.ResNetEncoder(**EC.TINY).cuda()
    x = torch.rand(1, 3, 40, 36, device="cuda")
    with pytest.raises(NotImplementedError, match="inference only"):
        model(x.clone().requires_grad_(True), size=32)
    with pytest.raises(RuntimeError, match="CUDA/ROCm|on cuda"):
        model(x.cpu(), size=32)
    with pytest.raises(ValueError, match="set_pca"):
        model(x, size=32, features=("pca",))


def test_extractor_output_conditions_the_generator(P):
    """ResnetFeatureExtractorPCA (small widths, PCA 16) on a 256^2 image -> [2,16,8,8]; G.f takes out[None, 0] as resnet_chonk and
    returns the same bits as for a clone of it."""
    import p3d_shared_cases as SC
    c = EC.network_case("tiny")
    rfe = P.ResnetFeatureExtractorPCA(None, 16, **c["arch"])
    EC.fill_model(rfe.rfe, c["sd"])
    rfe.cuda()
    img = EC.make_image((4, 256, 256), 8).cuda()
    out = rfe(img)
    assert tuple(out.shape) == (2, 16, 8, 8) and torch.isfinite(out).all() and float(out.std()) > 0
    assert torch.equal(rfe(img[None]), out)
    # p3d_shared_cases' small generator, with the cond_mode token that adds resnet_chonk to the 8 x 8 activations (reschonk_add_16)
    torch.manual_seed(5)
    kw = dict(SC.TRI_KW, rendering_kwargs={**SC.TRI_KW["rendering_kwargs"], "c_gen_conditioning_zero": True},
              cond_mode="ortho_front.add_shuffle2_4.inj_6b_4.reschonk_add_16", channel_base=2048, channel_max=64)
    G = P.generator.TriPlaneGenerator(**kw).cuda().eval()
    G.set_force_sigmoid(True)
    G.set_render_exact(True)
    cond = lambda chonk: {"image_ortho_front": img[None, :3, ::8, ::8].contiguous(), "resnet_chonk": chonk}
    a = SC.memo_call(G, cond(out[None, 0]), "cuda")
    b = SC.memo_call(G, cond(out[None, 0].clone()), "cuda")
    assert torch.isfinite(a).all() and torch.equal(a, b)
    assert not torch.equal(a, SC.memo_call(G, cond(out[None, 1]), "cuda"))  # the tensor is read: the mirror's features give another image
