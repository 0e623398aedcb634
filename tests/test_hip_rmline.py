"""GPU (-m gpu): the illustration-to-render module on the HIP kernels (include/p3d_rmline.h, panic3d_amd/rmline.py) against the float64
restatement of tests/rmline_cases.py.  The detector's response per value within 8 sqrt(K) 2^-24 sum|terms| (K = 3 + 2 (k0 + k1)); the
mask equal to float64's on every pixel whose decision that bound cannot flip (at most 1 % left out, asserted); one layer per value
within 8 sqrt(9 Ci + 1) 2^-24 sum|terms| and rel-L2 <= 1e-5 under both plans, every activation, the fused first-layer load and the fused
last-layer store bit-equal to the unfused composition; the whole module within 4 x torch's binary32 error, the input's bits where the
mask is 0, the one-call walk bit-equal to the layer-by-layer operators, both with the expected launch count; argument errors before any
launch; and one G.f call on the wrapper's output.  The gates' sensitivity to seeded faults is shown on CPU in tests/test_rmline_cpu.py.
On the parent commit the module, the operators and the symbols do not exist."""
import pytest
import torch

import rmline_cases as RC

pytestmark = pytest.mark.gpu
F = torch.nn.functional


@pytest.fixture(scope="module")
def P():
    import panic3d_amd
    panic3d_amd.build()
    panic3d_amd._lib.lib()
    return panic3d_amd


@pytest.mark.parametrize("dog", sorted(RC.DOGS))
@pytest.mark.parametrize("hw", RC.RESPONSE_SHAPES)
def test_response_against_float64(P, hw, dog):
    p = RC.DOGS[dog]
    bad = []
    for N, C in ((1, 1), (3, 3), (1, 4), (3, 4), (1, 3), (3, 1)):
        img = RC.smooth_image(N, C, hw[0], hw[1], 1)
        mask, image, resp = P.ops.rmline_mask(img.cuda(), None, dict(p, d=2), want_response=True)
        ref, bound = RC.batch_dog(img.double(), **p), RC.response_bound(img, **p)
        ratio = float(((resp.cpu().double() - ref).abs() / bound).max())
        print(f"response {dog} {hw} N={N} C={C}: worst {ratio:.3f} of the bound")
        if not ratio <= 1.0:
            bad.append((N, C, ratio))
        assert tuple(mask.shape) == (N, 1) + hw and tuple(resp.shape) == (N, 1) + hw
        if C == 4:  # the composite comes out too: one product and one sum per value
            assert float((image.cpu().double() - RC.composite(img.double())).abs().max()) <= 4 * RC.U
        else:
            assert image is None if C == 1 else image.data_ptr() == img.cuda().data_ptr() or torch.equal(image.cpu(), img)
        again = P.ops.rmline_mask(img.cuda(), None, dict(p, d=2), want_response=True)
        assert torch.equal(again[2], resp) and torch.equal(again[0], mask), "two runs differ"
    assert bad == []


@pytest.mark.parametrize("kind", ["smooth", "flat"])
@pytest.mark.parametrize("hw", RC.MASK_SHAPES)
def test_mask_equals_float64_where_the_response_decides(P, hw, kind):
    bad = []
    for C in (3, 4):
        img = RC.smooth_image(2, C, hw[0], hw[1], 2) if kind == "smooth" else RC.flat_image(2, C, hw[0], hw[1])
        for d in (1, 2, 3):
            for hull in (None, RC.make_hull(2, hw[0], hw[1])):
                p = dict(RC.DOG_WRAPPER, d=d)
                mask, _, _ = P.ops.rmline_mask(img.cuda(), hull.cuda() if hull is not None else None, p)
                assert set(mask.unique().tolist()) <= {0.0, 1.0}
                bad += RC.mask_gate(f"mask {kind} {hw} C={C} d={d} hull={hull is not None}", mask, img, hull, RC.DOG_WRAPPER, d)
                assert float(RC.uncertain(img, RC.DOG_WRAPPER, d).double().mean()) <= 0.01
                if hull is not None:
                    assert float((mask.cpu() * (hull != 0)).sum()) == 0
    if kind == "flat":  # on the flat regions the response is 0.5 - epsilon in float64: only the edge's neighbourhood can be a line
        resp = RC.batch_dog(RC.flat_image(1, 3, hw[0], hw[1]).double(), **RC.DOG_WRAPPER)
        far = torch.ones(hw[1], dtype=torch.bool)
        far[max(hw[1] // 2 - 4, 0):hw[1] // 2 + 4] = False
        assert float((resp[..., far] - 0.49).abs().max() if far.any() else 0.0) <= 1e-15
    assert bad == []


def _run_conv(P, c, act, plan, **kw):
    return P.ops.rmline_conv(RC.nhwc(c["x"]).cuda(), RC.to_wk(c["w"]).cuda(), c["b"].cuda(), act, c["slope"], plan=plan, **kw)


@pytest.mark.parametrize("chans", RC.CONV_CHANNELS)
def test_one_layer_under_every_plan(P, chans):
    Ci, Co = chans
    bad, plans = [], []
    for plan in (1, 2):
        try:
            plans.append(P.ops.rmline_conv_plan(Ci, Co, plan)["plan"])
        except ValueError:
            assert (Ci, Co, plan) == (64, 64, 1)  # the 8-row tile of the widest layer does not fit the LDS
    assert P.ops.rmline_conv_plan(Ci, Co)["plan"] == plans[0]
    for H, W in RC.CONV_SHAPES:
        c = RC.conv_case(Ci, Co, H, W)
        outs = []
        for plan in plans:
            for act in sorted(RC.ACTS):
                y = _run_conv(P, c, act, plan)
                assert tuple(y.shape) == (2, H - 2, W - 2, Co)
                assert torch.equal(_run_conv(P, c, act, plan), y), "two runs differ"
                bad += RC.conv_gate(f"{c['name']} plan {plan}", RC.nchw(y), c, act, c["slope"])
                planar = _run_conv(P, c, act, plan, planar=True)
                assert torch.equal(planar, RC.nchw(y)), "the planar store differs"
                outs.append((act, y))
        for (a0, y0), (a1, y1) in zip(outs[:3], outs[3:]):
            assert a0 == a1 and torch.equal(y0, y1), "the two plans differ"
    assert bad == []


@pytest.mark.parametrize("hw", [(1, 1), (5, 7), (RC.CONV_TILE[0] + 1, RC.CONV_TILE[1] + 1)])
def test_fused_ends_match_the_unfused_composition(P, hw):
    H, W = hw
    g = torch.Generator().manual_seed(H * 31 + W)
    image, mask = RC.smooth_image(2, 3, H, W, 4).cuda(), (torch.rand(2, 1, H, W, generator=g) > 0.5).float().cuda()
    hull = (RC.make_hull(2, H, W) != 0).float().cuda()
    for use_hull, use_mask, pad in ((True, True, 2), (False, True, 1), (True, False, 3), (False, False, 1)):
        Ci = 3 + use_hull
        w, b = torch.randn(8, Ci, 3, 3, generator=g), torch.randn(8, generator=g)
        wk, b = RC.to_wk(w).cuda(), b.cuda()
        stack = (image, mask if use_mask else None, hull if use_hull else None)
        fused = P.ops.rmline_conv(None, wk, b, "leaky", 0.01, stack=stack, pad=pad)
        xin = image * (1 - mask) if use_mask else image
        xin = torch.cat([xin, hull], dim=1) if use_hull else xin
        xin = F.pad(xin, (pad,) * 4, mode="replicate")
        plain = P.ops.rmline_conv(RC.nhwc(xin), wk, b, "leaky", 0.01)
        assert tuple(fused.shape) == (2, H + 2 * pad - 2, W + 2 * pad - 2, 8) and torch.equal(fused, plain), (use_hull, use_mask, pad)
    # the last layer's store: tanh, then torch.lerp against image and mask
    x = torch.randn(2, H + 2, W + 2, 5, generator=g).cuda()
    w, b = torch.randn(3, 5, 3, 3, generator=g) * 0.3, torch.randn(3, generator=g) * 0.1
    wk, b = RC.to_wk(w).cuda(), b.cuda()
    unfused = P.ops.rmline_conv(x, wk, b, "tanh", planar=True)
    assert torch.equal(P.ops.rmline_conv(x, wk, b, "tanh", planar=True, lerp=(image, mask)), torch.lerp(image, unfused, mask))
    # a soft weight takes torch.lerp's two branches (either side of 0.5); torch's own kernel may contract a + w (b - a) into one fma,
    # the store names every rounding: equal to within those roundings, not bit for bit
    soft = torch.rand(2, 1, H, W, generator=g).cuda()
    fused, plain = P.ops.rmline_conv(x, wk, b, "tanh", planar=True, lerp=(image, soft)), torch.lerp(image, unfused, soft)
    assert bool(((fused - plain).abs() <= 4 * RC.U * (image.abs() + unfused.abs())).all())
    kept = (mask == 0).expand(-1, 3, -1, -1)
    assert torch.equal(P.ops.rmline_conv(x, wk, b, "tanh", planar=True, lerp=(image, mask))[kept], image[kept])


@pytest.mark.parametrize("arch", sorted(RC.ARCHS))
@pytest.mark.parametrize("hw", RC.MODULE_SHAPES)
def test_whole_module(P, hw, arch, monkeypatch):
    c = RC.module_case(arch, hw)
    depth = c["arch"]["gen_depth"]
    model = RC.fill_model(P.RMLineGenerator(**c["arch"]), c["sd"]).cuda()
    wrap = P.RMLineWrapper(model)
    img, hull = c["img"].cuda(), c["hull"].cuda()
    fused, more = wrap(img, face_hull=hull, return_more=True)
    assert model.program().launches == depth + 1
    assert tuple(fused.shape) == tuple(img.shape) and torch.isfinite(fused).all()
    assert torch.equal(fused[:, 3], img[:, 3]), "the alpha is passed through"
    assert torch.equal(more["line_mask"].cpu().double(), c["mask"])  # (the case has no uncertain pixel)
    assert RC.module_gate(c["name"], fused, c["f64"], c["f32"]) == []
    kept = (more["line_mask"] == 0).expand(-1, 3, -1, -1)
    assert torch.equal(fused[:, :3][kept], more["image"][kept]), "where the mask is 0 the output carries the input's bits"
    calls = []
    for name in ("_rmline_mask_impl", "_rmline_conv_impl"):
        real = getattr(P.ops, name)
        monkeypatch.setattr(P.ops, name, lambda *a, _real=real, _name=name: (calls.append(_name), _real(*a))[1])
    layered = wrap(img, face_hull=hull, fused=False)
    assert len(calls) == depth + 1 and calls[0] == "_rmline_mask_impl"  # one launch per operator call
    assert torch.equal(layered, fused), "the one-call walk and the layer-by-layer operators differ"
    assert torch.equal(wrap(img, face_hull=hull), fused), "two runs differ"
    # the bare generator on a given mask (the reference model's forward): depth launches
    x = {k: v.cuda() for k, v in c["x"].items()}
    out = model(x)
    assert model.program().launches == depth and out["line_mask"] is x["line_mask"]
    assert RC.module_gate(c["name"] + " generator", out["image"], c["g64"], c["g32"]) == []
    assert torch.equal(model(x, fused=False)["image"], out["image"])
    if min(hw) > 2 * depth:
        crop = model(x, pad=False)["image"]
        assert tuple(crop.shape) == (2, 3, hw[0] - 2 * depth, hw[1] - 2 * depth)
        assert RC.rel_l2(crop, out["image"][:, :, depth:-depth, depth:-depth]) <= 1e-5


def test_argument_errors_come_before_any_launch(P):
    z = lambda *s: torch.zeros(*s, device="cuda")
    ops = P.ops
    with pytest.raises(ValueError):
        ops.rmline_mask(z(1, 2, 8, 8))                                   # channels
    with pytest.raises(ValueError):
        ops.rmline_mask(z(1, 3, 8, 8), z(1, 1, 8, 7))                    # the hull's shape
    with pytest.raises(ValueError, match="taps"):
        ops.rmline_mask(z(1, 3, 8, 8), None, dict(sigma=4.0))            # 2 int(4 * 1.6 * 4) + 1 = 51 taps
    with pytest.raises(ValueError):
        ops.rmline_mask(z(1, 3, 8, 8), None, dict(d=9))
    with pytest.raises(ValueError):
        ops.rmline_mask(z(1, 3, 8, 8), None, dict(k=0.5))
    with pytest.raises(RuntimeError, match="CUDA/ROCm"):
        ops.rmline_mask(torch.zeros(1, 3, 8, 8))
    with pytest.raises(ValueError):
        ops.rmline_conv(z(1, 8, 8, 4), z(9, 5, 8), z(8))                 # wk's channels
    with pytest.raises(ValueError):
        ops.rmline_conv(z(1, 8, 8, 4), z(9, 4, 8), z(7))                 # bias
    with pytest.raises(ValueError):
        ops.rmline_conv(z(1, 2, 8, 4), z(9, 4, 8), z(8))                 # smaller than the filter
    with pytest.raises(ValueError):
        ops.rmline_conv(z(1, 8, 8, 65), z(9, 65, 8), z(8))               # more than 64 channels
    with pytest.raises(ValueError):
        ops.rmline_conv(z(1, 8, 8, 4), z(9, 4, 8), z(8), "relu")
    with pytest.raises(ValueError):
        ops.rmline_conv(z(1, 8, 8, 64), z(9, 64, 64), z(64), plan=1)     # the forced tile does not fit
    with pytest.raises(ValueError):
        ops.rmline_conv(z(1, 8, 8, 4), z(9, 4, 3), z(3), lerp=(z(1, 3, 6, 6), z(1, 1, 6, 6)))  # lerp wants the planar store
    with pytest.raises(ValueError):
        ops.rmline_conv(None, z(9, 4, 8), z(8), stack=(z(1, 3, 6, 6), None, None), pad=1)      # four channels without a hull
    with pytest.raises(RuntimeError, match="CUDA/ROCm"):
        ops.rmline_conv(torch.zeros(1, 8, 8, 4), z(9, 4, 8), z(8))
    model = P.RMLineGenerator(gen_depth=2, gen_width=8).cuda()
    prog = model.program()
    with pytest.raises(ValueError):
        ops.rmline_forward(prog, z(1, 3, 8, 8), hull=None, dog={})       # the first layer wants a hull
    with pytest.raises(ValueError):
        ops.rmline_forward(prog, z(1, 4, 8, 8), hull=z(1, 1, 8, 8), mask=z(1, 1, 8, 8))  # RGBA without the detector
    with pytest.raises(ValueError):
        ops.rmline_forward(prog, z(1, 3, 3, 3), hull=z(1, 1, 3, 3), mask=z(1, 1, 3, 3), pad=0)  # nothing left
    with pytest.raises(ValueError):
        ops.rmline_forward(prog, z(1, 3, 8, 8), hull=z(1, 1, 8, 8), mask=z(1, 1, 8, 8), pad=1, lerp=True)
    with pytest.raises(RuntimeError, match="CUDA/ROCm"):
        ops.rmline_forward(prog, torch.zeros(1, 3, 8, 8), hull=z(1, 1, 8, 8), dog={})
    with pytest.raises(NotImplementedError, match="inference only"):
        P.RMLineWrapper(model)(z(1, 3, 8, 8).requires_grad_(True))
    with pytest.raises(NotImplementedError, match="inference only"):
        model.train()


def test_wrapper_output_conditions_the_generator(P):
    """One G.f call on the small test generator takes cond['image_ortho_front'] from RMLineWrapper."""
    import p3d_shared_cases as SC
    c = RC.module_case("default", (37, 41))
    wrap = P.RMLineWrapper(RC.fill_model(P.RMLineGenerator(**c["arch"]), c["sd"]).cuda())
    img = RC.smooth_image(1, 4, 64, 64, 6).cuda()
    kpts = torch.tensor([[20 + (i * 7) % 23, 18 + (i * 11) % 29] for i in range(28)], dtype=torch.float64).numpy()
    out = wrap(img[0], kpts=kpts)
    assert tuple(out.shape) == (4, 64, 64) and torch.isfinite(out).all() and not torch.equal(out, img[0])
    G = SC.memo_generator("cuda")
    feats = torch.randn(1, 16, generator=torch.Generator().manual_seed(2)).cuda()
    cond = lambda front: {"image_ortho_front": front[None, :3, ::2, ::2].contiguous(), "resnet_feats": feats}
    a = SC.memo_call(G, cond(out), "cuda")
    assert torch.isfinite(a).all() and tuple(a.shape) == (1, 3, 512, 512)
    assert torch.equal(a, SC.memo_call(G, cond(out.clone()), "cuda"))
    assert not torch.equal(a, SC.memo_call(G, cond(img[0]), "cuda"))  # the tensor is read: the raw illustration gives another image
