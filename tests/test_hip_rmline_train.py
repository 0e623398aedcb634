"""GPU (-m gpu): training the illustration-to-render module on the HIP operators (include/p3d_rmline_grad.h, panic3d_amd/rmline_train.py)
against the float64 closed forms and the float64 restatement of tests/rmline_train_cases.py.  Gates: a sum of K binary32 products may
miss float64 by 8 sqrt(K) 2^-24 sum|terms| per value; whole steps and five fit_steps must stay within 4 x the error torch's own binary32
autograd of the same modules makes on the same case (the margin of test_hip_lpips.py and test_hip_rmline.py).  Every case is a few
patches.  On the parent commit the module does not exist.

The running statistics equal torch's BatchNorm2d in this sense: on given binary32 inputs the update is within 2 ulp (of its larger
operand) of the exact float64 update, where torch's own sits too; in whole steps, where each network normalises its own binary32
activations, within 2 ulp plus 4 x torch's own error against float64.  The counter is exact.

Measured on one MI355X (148 tensors over the whole-step cases and the five fit_steps): this project's rel-L2 against float64 over
torch's binary32 rel-L2 has median 0.89 and maximum 3.52; five fit_steps: worst 1.78."""
import pytest
import torch

import rmline_train_cases as TC

pytestmark = pytest.mark.gpu
E = TC.EPS32
PAIRS = [(4, 32), (32, 32), (32, 3), (4, 16), (16, 16), (5, 7), (64, 64)]  # (Ci, Co)
MAPS = [(1, 1), (5, 7), (7, 15), (8, 16), (9, 17), (9, 31), (9, 33)]         # g / dz maps: across the 16-pixel block, the 32-column and 8-row tile


@pytest.fixture(scope="module")
def P():
    import panic3d_amd
    panic3d_amd.build()
    return panic3d_amd


def rnd(shape, seed, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).float()


# ---- statistics ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [3, 16, 32, 33])
def test_statistics(P, C):
    for N in (1, 3):
        for hw in ((1, 2), (7, 7), (9, 33)):
            for kind in ("normal", "offset"):
                x = rnd((N,) + hw + (C,), 11 * C + N) if kind == "normal" else 100.0 + rnd((N,) + hw + (C,), 13 * C + N, 0.01)
                x64 = x.double().reshape(-1, C)
                K = x64.shape[0]
                bn = torch.nn.BatchNorm2d(C)
                with torch.no_grad():
                    bn.running_mean.copy_(rnd((C,), 5)), bn.running_var.copy_(rnd((C,), 6).abs() + 0.5)
                rm, rv, cnt = bn.running_mean.clone().cuda(), bn.running_var.clone().cuda(), bn.num_batches_tracked.clone().cuda()
                rm0, rv0 = rm.double().cpu(), rv.double().cpu()
                mean, var = P.ops.rmline_bn_stats(x.cuda(), rm, rv, cnt, 0.1)
                m64, v64 = x64.mean(0), ((x64 - x64.mean(0)) ** 2).mean(0)
                mb, vb = TC.stats_bounds(x64)
                em, ev = (mean.double().cpu() - m64).abs(), (var.double().cpu() - v64).abs()
                print(f"C={C} N={N} hw={hw} {kind}: mean err/bound {float((em / mb).max()):.3f} var err/bound {float((ev / vb).max()):.3f}")
                assert (em <= mb).all() and (ev <= vb).all(), (N, hw, kind)
                bn.train()(x.permute(0, 3, 1, 2))
                # the running update against the EXACT float64 update of the same binary32 inputs, within 2 ulp of the larger operand
                # (torch's own binary32 update sits within 0.9 of that bound on these cases)
                xm, xv = 0.9 * rm0 + 0.1 * m64, 0.9 * rv0 + 0.1 * v64 * K / (K - 1)
                ulp_m = 2 * 2.0 ** -23 * torch.maximum(0.9 * rm0.abs(), 0.1 * m64.abs())
                ulp_v = 2 * 2.0 ** -23 * torch.maximum(0.9 * rv0.abs(), 0.1 * v64 * K / (K - 1))
                dm, dv = (rm.double().cpu() - xm).abs(), (rv.double().cpu() - xv).abs()
                print(f"  running update: mean {float((dm / ulp_m).max()):.3f}, var {float((dv / ulp_v).max()):.3f} of 2 ulp; "
                      f"torch's {float(((bn.running_mean.double() - xm).abs() / ulp_m).max()):.3f}, {float(((bn.running_var.double() - xv).abs() / ulp_v).max()):.3f}")
                assert (dm <= ulp_m).all() and (dv <= ulp_v).all(), (N, hw, kind)
                assert int(cnt) == int(bn.num_batches_tracked) == 1
                mean2, var2 = P.ops.rmline_bn_stats(x.cuda())  # no running statistics; the same bits
                assert torch.equal(mean2, mean) and torch.equal(var2, var)
    before = P.ops.RMLINE_LAUNCHES[0]
    with pytest.raises(ValueError):
        P.ops.rmline_bn_stats(torch.zeros((1, 1, 1, C), device="cuda"))  # one value per channel, as torch raises
    assert P.ops.RMLINE_LAUNCHES[0] == before


def test_statistics_many_workgroups(P):
    x = 3.0 + rnd((5, 31, 31, 32), 3)  # K = 4805: 19 workgroups merged in order
    x64 = x.double().reshape(-1, 32)
    mean, var = P.ops.rmline_bn_stats(x.cuda())
    mb, vb = TC.stats_bounds(x64)
    assert ((mean.double().cpu() - x64.mean(0)).abs() <= mb).all()
    assert ((var.double().cpu() - ((x64 - x64.mean(0)) ** 2).mean(0)).abs() <= vb).all()


# ---- the fold and the coefficients ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chans", [(4, 32), (32, 3), (5, 7), (64, 64)])
def test_fold_and_coefficients(P, chans):
    Ci, Co = chans
    w, b = rnd((Co, Ci, 3, 3), 1, 0.2), rnd((Co,), 2)
    gamma, beta, mean, var = rnd((Ci,), 3).abs() + 0.5, rnd((Ci,), 4), rnd((Ci,), 5), rnd((Ci,), 6).abs() + 0.1
    dev = [t.cuda() for t in (w, b, gamma, beta, mean, var)]
    wk, bf = P.ops.rmline_bn_fold(dev[0], dev[1], tuple(dev[2:]) + (1e-5,))
    wk64, bf64 = TC.bn_fold(w.double(), b.double(), (gamma.double(), beta.double(), mean.double(), var.double(), 1e-5))
    assert TC.rel_l2(wk, wk64) < 4 * E and float((bf.double().cpu() - bf64).abs().max()) < 8 * (9 * Ci) ** 0.5 * E * float((w.abs().sum((1, 2, 3)) * 3).max() + 1)
    wk0, bf0 = P.ops.rmline_bn_fold(dev[0], dev[1])
    assert torch.equal(wk0.cpu(), w.permute(2, 3, 1, 0).reshape(9, Ci, Co)) and torch.equal(bf0.cpu(), b)
    dwk, db = rnd((9, Ci, Co), 7), rnd((Co,), 8)
    got = P.ops.rmline_bn_coef(dwk.cuda(), db.cuda(), dev[0], dev[2], dev[3], dev[4], dev[5], 1e-5, 77)
    want = TC.bn_coef(dwk.double(), db.double(), w.double(), gamma.double(), beta.double(), mean.double(), var.double(), 1e-5, 77)
    for name, g, r in zip(("dgamma", "dbeta", "dw", "c0", "c1"), got, want):
        assert TC.rel_l2(g, r) < 2e-5, name
    none = P.ops.rmline_bn_coef(dwk.cuda(), db.cuda(), dev[0], dev[2], dev[3], dev[4], dev[5], 1e-5, 77, want_dw=False, want_affine=False)
    assert none[0] is None and none[1] is None and none[2] is None and torch.equal(none[3], got[3]) and torch.equal(none[4], got[4])


# ---- the forward with per-tap chains ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chans", [(4, 32), (32, 32), (32, 3), (5, 7), (64, 64)])
def test_forward_per_tap(P, chans):
    Ci, Co = chans
    for N, hw in ((1, (3, 3)), (3, (9, 17)), (2, (11, 35))):
        x, wk, b = rnd((N,) + hw + (Ci,), Ci + N), rnd((9, Ci, Co), Co, 0.3), rnd((Co,), 3)
        got = P.ops.rmline_conv(x.cuda(), wk.cuda(), b.cuda(), "leaky", 0.01, per_tap=True)
        ref = TC.conv(x.double(), wk.double(), b.double(), "leaky", 0.01)
        bound = 8 * (9 * Ci) ** 0.5 * E * (TC.conv(x.double().abs(), wk.double().abs(), b.double().abs()) )
        assert ((got.double().cpu() - ref).abs() <= bound).all(), (N, hw)
        one = P.ops.rmline_conv(x.cuda(), wk.cuda(), b.cuda(), "leaky", 0.01)  # the inference path's single chain: within both roundings
        assert ((got - one).abs().double().cpu() <= 2 * bound).all()
        assert torch.equal(got, P.ops.rmline_conv(x.cuda(), wk.cuda(), b.cuda(), "leaky", 0.01, per_tap=True))


# ---- the data gradient ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chans", PAIRS)
def test_data_gradient(P, chans):
    Ci, Co = chans
    worst = 0.0
    for N in (1, 3):
        for hw in MAPS:
            g, wk = rnd((N,) + hw + (Co,), 3 * Ci + N), rnd((9, Ci, Co), 5 * Co, 0.3)
            a = rnd((N, hw[0] + 2, hw[1] + 2, Ci), 7)
            a[:, ::2, ::3, :] = 0.0  # a = 0 takes the slope
            c0, c1 = rnd((Ci,), 8), rnd((Ci,), 9)
            gd, wd, ad = g.cuda(), wk.cuda(), a.cuda()
            plain = P.ops.rmline_conv_dgrad(gd, wd)
            ref = TC.conv_dgrad(g.double(), wk.double())
            bound = 8 * (9 * Co) ** 0.5 * E * TC.conv_dgrad(g.double().abs(), wk.double().abs())
            err = (plain.double().cpu() - ref).abs()
            worst = max(worst, float((err / bound.clamp_min(1e-30)).max()))
            assert (err <= bound).all() and TC.rel_l2(plain, ref) <= 1e-5, (N, hw)
            fused = P.ops.rmline_conv_dgrad(gd, wd, a=ad, c0=c0.cuda(), c1=c1.cuda(), slope=0.01)
            reff = TC.conv_dgrad(g.double(), wk.double(), a.double(), c0.double(), c1.double(), 0.01)
            fb = (bound + 4 * E * (ref.abs() + c0.double().abs() + (c1.double() * a.double()).abs())) * torch.where(a > 0, 1.0, 0.01).double()
            assert ((fused.double().cpu() - reff).abs() <= fb).all() and TC.rel_l2(fused, reff) <= 1e-5, (N, hw)
            only = P.ops.rmline_conv_dgrad(gd, wd, a=ad, slope=0.01)  # LeakyReLU's derivative alone
            assert torch.equal(only, torch.where(ad > 0, plain, plain * 0.01))
            planar = P.ops.rmline_conv_dgrad(gd, wd, a=ad, c0=c0.cuda(), c1=c1.cuda(), slope=0.01, planar=True)
            assert torch.equal(planar.permute(0, 2, 3, 1), fused)
            assert torch.equal(P.ops.rmline_conv_dgrad(gd, wd, a=ad, c0=c0.cuda(), c1=c1.cuda(), slope=0.01), fused)  # two runs, equal bits
    print(f"dgrad {chans}: worst err/bound {worst:.3f}")


# ---- the weight / bias gradient ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chans", PAIRS)
def test_weight_gradient(P, chans):
    Ci, Co = chans
    worst = 0.0
    for N in (1, 3, 8):
        for hw in MAPS:
            x, dz = rnd((N, hw[0] + 2, hw[1] + 2, Ci), 3 * Ci + N), rnd((N,) + hw + (Co,), 5 * Co + N)
            rw, rb = TC.conv_wgrad(x.double(), dz.double())
            aw, ab = TC.conv_wgrad(x.double().abs(), dz.double().abs())
            e = 8 * (N * hw[0] * hw[1]) ** 0.5 * E
            xd, dd = x.cuda(), dz.cuda()
            for force in sorted({0, 1, min(2, N), N}):
                dw, db = P.ops.rmline_conv_wgrad(xd, dd, force_slices=force)
                ew, eb = (dw.double().cpu() - rw).abs(), (db.double().cpu() - rb).abs()
                worst = max(worst, float((ew / (e * aw).clamp_min(1e-30)).max()), float((eb / (e * ab).clamp_min(1e-30)).max()))
                assert (ew <= e * aw).all() and (eb <= e * ab).all(), (N, hw, force)
                dw2, db2 = P.ops.rmline_conv_wgrad(xd, dd, force_slices=force)
                assert torch.equal(dw, dw2) and torch.equal(db, db2)  # bitwise reproducible under every slice count
                ow, _ = P.ops.rmline_conv_wgrad(xd, dd, force_slices=force, oihw=True)
                assert torch.equal(ow, dw.reshape(3, 3, Ci, Co).permute(3, 2, 0, 1))
    print(f"wgrad {chans}: worst err/bound {worst:.3f}")


@pytest.mark.parametrize("pad", [0, 2])
def test_first_layer_weight_gradient_builds_the_stack_in_the_load(P, pad):
    for N, S, Co in ((2, 9, 8), (3, 21, 32), (1, 10, 5)):
        image, mask = torch.rand((N, 3, S, S), generator=torch.Generator().manual_seed(S)), (rnd((N, 1, S, S), 2) > 0.3).float()
        hull = (rnd((N, 1, S, S), 3) > 0.5).float()
        dz = rnd((N, S + 2 * pad - 2, S + 2 * pad - 2, Co), 4).cuda()
        for m, h in ((mask, hull), (None, hull), (mask, None)):
            stored = TC.stack_input(image, m, h, pad)  # the same binary32 products as the load's
            a = P.ops.rmline_conv_wgrad(None, dz, stack=(image.cuda(), m.cuda() if m is not None else None, h.cuda() if h is not None else None), pad=pad)
            b = P.ops.rmline_conv_wgrad(stored.cuda(), dz)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (N, S, Co)


# ---- the head -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(2, 21, 6), (3, 10, 3), (1, 9, 2), (2, 7, 0)])
def test_head(P, case):
    N, S, crop = case
    gen = torch.Generator().manual_seed(S)
    t, image = torch.rand((N, 3, S, S), generator=gen) * 2 - 1, torch.rand((N, 3, S, S), generator=gen)
    mask = (torch.rand((N, 1, S, S), generator=gen) > 0.5).float()  # a line mask: 0 / 1
    t[:, :, 1, 1] = image[:, :, 1, 1]  # img = gt with mask != 0 too
    hull = (torch.rand((N, 1, S, S), generator=gen) > 0.5).float()
    img, l1, ci, ch = P.ops.rmline_head(t.cuda(), image.cuda(), mask.cuda(), hull.cuda(), crop)
    assert torch.equal(img.cpu(), torch.lerp(image, t, mask))  # torch.lerp's bits
    # a soft weight takes torch.lerp's two branches (either side of 0.5); torch's own kernel may contract a + w (b - a) into one fma, the
    # kernel names every rounding: equal to within those roundings, as tests/test_hip_rmline.py holds P3D_RMLINE_OUT_LERP
    soft = torch.rand((N, 1, S, S), generator=gen)
    simg = P.ops.rmline_head(t.cuda(), image.cuda(), soft.cuda())[0].cpu()
    assert ((simg - torch.lerp(image, t, soft)).abs() <= 4 * 2.0 ** -24 * (image.abs() + t.abs())).all()
    r64 = TC.head(t.double(), image.double(), mask.double(), hull.double(), crop)
    # img itself is binary32's; the L1 sum is held against float64 of the same binary32 img
    l64 = (img.double().cpu() - image.double()).abs().mean((1, 2, 3))
    assert ((l1.double().cpu() - l64).abs() <= 8 * (3 * S * S) ** 0.5 * E).all() and ((l1.double().cpu() - r64[1]).abs() <= 8 * (3 * S * S) ** 0.5 * E).all()
    if crop:
        assert torch.equal(ci, img[..., crop:-crop, crop:-crop]) and torch.equal(ch.cpu(), hull[..., crop:-crop, crop:-crop])
    else:
        assert ci is None and ch is None
    g = rnd((N,), 5)
    d = rnd((N, 3, S - 2 * crop, S - 2 * crop), 6)
    out = P.ops.rmline_head_grad(t.cuda(), img, image.cuda(), mask.cuda(), g.cuda(), d.cuda(), crop)
    ref = TC.head_grad(t.double(), img.double().cpu(), image.double(), mask.double(), g.double(), d.double(), crop)
    inner = TC.head_grad(None, img.double().cpu(), image.double(), mask.double(), g.double(), d.double(), crop)  # 1 - t^2 is absolute to 2^-24
    assert ((out.double().cpu() - ref).abs() <= 8 * E * (ref.abs() + inner.abs()) + 1e-30).all()
    assert (out.cpu().permute(0, 3, 1, 2)[(mask == 0).expand(-1, 3, -1, -1)] == 0).all()  # mask = 0: exactly 0
    # any strides of d: the channel-last view of the same values
    dcl = d.permute(0, 2, 3, 1).contiguous().cuda().permute(0, 3, 1, 2)
    assert torch.equal(P.ops.rmline_head_grad(t.cuda(), img, image.cuda(), mask.cuda(), g.cuda(), dcl, crop), out)
    # the two halves the autograd Functions launch compose to the same formula
    half = P.ops.rmline_head_grad(None, img, image.cuda(), mask.cuda(), g.cuda(), d.cuda(), crop, shape=(N, S, S))
    both = P.ops.rmline_head_grad(t.cuda(), None, None, None, None, half.permute(0, 3, 1, 2), 0)
    assert TC.rel_l2(both, ref) < 4 * E


# ---- whole steps -----------------------------------------------------------------------------------------------------------------------------
def expected_launches(Lg, Ld):
    """The library's launches of one fit_step (DESIGN.md §4.19's table)."""
    fwd = (4 * Lg - 2) + 1 + (4 * Ld - 2)
    gen_bwd = (4 * (Ld - 1) + 1) + 1 + (1 + 4 * (Lg - 1) + 2)
    dis_bwd = 4 * (Ld - 1) + 2
    return 2 * fwd + gen_bwd + dis_bwd


@pytest.mark.parametrize("name", ["real", "small", "ragged"])
@pytest.mark.parametrize("B", [1, 2])
def test_whole_steps(P, name, B):
    cfg = TC.CONFIGS[name]
    model = TC.perturb(P.RMLineModel(**cfg)).cuda().train()
    ref64, ref32 = TC.ref_like(model), TC.ref_like(model, dtype=torch.float32)
    batch = TC.make_batch(cfg, B)
    b64, bdev = {k: v.double() for k, v in batch.items()}, {k: v.cuda() for k, v in batch.items()}
    twin = TC.perturb(P.RMLineModel(**cfg)).cuda().train()  # a second run of the same steps: equal bits
    prev = {n: b.detach().clone() for n, b in ref64.named_buffers()}
    for idx in (0, 1):
        rl, rg, rb = TC.step_results(ref64, b64, idx)
        tl, tg, tb = TC.step_results(ref32, batch, idx)
        ml, mg, mb = TC.step_results(model, bdev, idx)
        wl, wg, wb = TC.step_results(twin, bdev, idx)
        for k in ("loss", "loss_l1", "loss_adv"):
            mine = float(model.logged[("train_gen_" if idx == 0 else "train_dis_") + k])
            assert abs(mine - float(ref64.last[k])) <= 1e-5, (k, mine, float(ref64.last[k]))
        other = "discriminator." if idx == 0 else "generator."
        for n in rg:
            if n.startswith(other):
                assert mg[n] is None and rg[n] is None, n
                continue
            mine, torchs = TC.rel_l2(mg[n], rg[n]), TC.rel_l2(tg[n], rg[n])
            print(f"{name} B={B} step {idx} {n}: {mine:.2e} (torch binary32 {torchs:.2e})")
            assert mine <= 4 * torchs, (n, mine, torchs)
            assert torch.equal(mg[n], wg[n]), n
        for n in rb:  # every batch norm of BOTH networks moved, in both steps
            if n.endswith("num_batches_tracked"):
                assert int(mb[n]) == int(rb[n]) == idx + 1, n
            else:
                # equal to torch's: the update's own arithmetic to 2 ulp of its larger operand; the activations the statistic is taken
                # from are each network's own binary32 forward, so their part is held, like the gradients, to 4 x torch's own error
                stat = (rb[n] - 0.9 * prev[n]) / 0.1  # the batch statistic float64 fed into this update
                ulp2 = 2 * 2.0 ** -23 * float(torch.maximum(0.9 * prev[n].abs(), 0.1 * stat.abs()).max())
                mine, torchs = float((mb[n].double().cpu() - rb[n]).abs().max()), float((tb[n].double() - rb[n]).abs().max())
                print(f"{name} B={B} step {idx} {n}: {mine:.2e} (torch binary32 {torchs:.2e}, 2 ulp {ulp2:.2e})")
                assert mine <= 4 * torchs + ulp2, (n, mine, torchs, ulp2)
            assert torch.equal(mb[n], wb[n]), n
        prev = rb
    opts = model.configure_optimizers()
    before = P.ops.RMLINE_LAUNCHES[0]
    model.fit_step(bdev, opts)
    assert P.ops.RMLINE_LAUNCHES[0] - before == expected_launches(cfg["gen_depth"], cfg["dis_depth"])
    with pytest.raises(NotImplementedError):
        model.forward({k: (v[:, 0].clone().requires_grad_(True) if k == "image" else v[:, 0]) for k, v in bdev.items()})


def test_one_value_per_channel_raises(P):
    cfg = dict(TC.CONFIGS["small"], patch_size=5, dis_depth=2)  # the discriminator's first map is 3 x 3: fine; pad=False on a 3 x 3 input is not
    model = P.RMLineModel(**cfg).cuda().train()
    x = {k: v[:1, 0, ..., :3, :3].contiguous().cuda() for k, v in TC.make_batch(cfg, 1).items() if k != "real_label"}
    with pytest.raises(ValueError):
        model.forward(x, pad=False)  # a 1 x 1 map from one patch: one value per channel, as torch raises


def test_five_fit_steps_and_the_hand_over(P):
    cfg = TC.CONFIGS["real"]
    model = P.RMLineModel(**cfg).cuda().train()
    ref64, ref32 = TC.ref_like(model), TC.ref_like(model, dtype=torch.float32)
    batch = TC.make_batch(cfg, 2)
    b64, bdev = {k: v.double() for k, v in batch.items()}, {k: v.cuda() for k, v in batch.items()}
    opts = model.configure_optimizers()
    assert all(isinstance(o, P.optim.Adam) for o in opts[0])
    o64 = [torch.optim.Adam(ref64.generator.parameters(), lr=1e-3), torch.optim.Adam(ref64.discriminator.parameters(), lr=1e-3)]
    o32 = [torch.optim.Adam(ref32.generator.parameters(), lr=1e-3), torch.optim.Adam(ref32.discriminator.parameters(), lr=1e-3)]
    for _ in range(5):
        model.fit_step(bdev, opts)
        ref64.fit_step(b64, o64)
        ref32.fit_step(batch, o32)
    p64, p32 = dict(ref64.named_parameters()), dict(ref32.named_parameters())
    for n, p in model.named_parameters():
        mine, torchs = TC.rel_l2(p, p64[n]), TC.rel_l2(p32[n], p64[n])
        print(f"five steps {n}: {mine:.2e} (torch binary32 {torchs:.2e})")
        assert mine <= 4 * torchs, (n, mine, torchs)
    # hand-over
    gen = P.RMLineGenerator()
    gen.load_state_dict(model.state_dict())  # the discriminator's keys are ignored
    gen = gen.cuda()
    x = {k: v[:, 0].contiguous() for k, v in bdev.items() if k != "real_label"}
    model.eval()
    assert torch.equal(model.forward(x)["image"], gen.forward(x)["image"])
    assert torch.equal(model.validation_step(bdev)["images"], torch.lerp(x["image"], gen.forward(x)["image"], x["line_mask"]))
    assert "_cache" not in "".join(model.state_dict())
    rgba = torch.rand((1, 4, 64, 64), generator=torch.Generator().manual_seed(1)).cuda()
    out = P.RMLineWrapper(model.to_generator())(rgba)
    assert out.shape == rgba.shape and torch.isfinite(out).all()
    model.train()
    with pytest.raises(NotImplementedError):
        P.RMLineGenerator().train(True)  # unchanged


# ---- argument errors -----------------------------------------------------------------------------------------------------------------------
def test_argument_errors_come_before_any_launch(P):
    ops, L = P.ops, P._lib.lib()
    before = ops.RMLINE_LAUNCHES[0]
    g, wk, a = torch.zeros((1, 5, 5, 8), device="cuda"), torch.zeros((9, 8, 8), device="cuda"), torch.zeros((1, 7, 7, 8), device="cuda")
    out = torch.full((1, 7, 7, 8), 7.0, device="cuda")
    for slope in (0.0, -0.01, float("nan")):
        with pytest.raises(ValueError):
            ops.rmline_conv_dgrad(g, wk, a=a, slope=slope)
        assert L.p3d_rmline_conv_dgrad_f32(g.data_ptr(), 1, 5, 5, 8, wk.data_ptr(), 8, a.data_ptr(), None, None, slope, 0, out.data_ptr(), None) == -1
    big = torch.zeros(4096, device="cuda")
    for gp, ap, op in ((4, 0, 0), (0, 4, 0), (0, 0, 4)):  # misaligned channel-last pointers
        assert L.p3d_rmline_conv_dgrad_f32(big.data_ptr() + gp, 1, 5, 5, 8, wk.data_ptr(), 8, big.data_ptr() + ap, None, None, 0.01, 0, out.data_ptr() + op, None) == -1
    assert L.p3d_rmline_conv_wgrad_f32(big.data_ptr() + 4, None, None, None, 1, 7, 7, 0, 8, g.data_ptr(), 8, 0, 0, out.data_ptr(), out.data_ptr(), big.data_ptr(), 4096, None) == -1
    with pytest.raises(ValueError):
        ops.rmline_conv_dgrad(torch.zeros((1, 5, 5, 65), device="cuda"), torch.zeros((9, 8, 65), device="cuda"))
    with pytest.raises(ValueError):
        ops.rmline_conv_wgrad(torch.zeros((1, 7, 7, 65), device="cuda"), torch.zeros((1, 5, 5, 8), device="cuda"))
    with pytest.raises(ValueError):
        ops.rmline_conv_wgrad(a, g, force_slices=2)  # more slices than patches
    with pytest.raises(ValueError):
        ops.rmline_conv(torch.zeros((1, 2, 2, 8), device="cuda"), wk, torch.zeros(8, device="cuda"))  # smaller than the filter
    with pytest.raises(ValueError):
        ops.rmline_bn_stats(torch.zeros((1, 1, 1, 8), device="cuda"))
    torch.cuda.synchronize()
    assert ops.RMLINE_LAUNCHES[0] == before and float(out.min()) == 7.0  # nothing ran, nothing was written
