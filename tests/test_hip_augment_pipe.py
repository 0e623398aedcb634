"""GPU (-m gpu): the augmentation pipe on the HIP kernels (include/p3d_augment_tail.h, panic3d_amd/augment.py).
Operator level: ops.augment_tail and its adjoint against the float64 restatement of tests/augment_pipe_cases.py under the gate
8 sqrt(K) 2^-24 sum|terms| (K the header's longest rounding chain), at the smallest sides the filter accepts, one pixel beyond the tile on
each axis, both tile heights, each stage alone and all together, an empty and a covering rectangle; bits run to run and across grad
modes; the adjoint identity; a double backward; argument errors.  Module level: AugmentPipe against the reference's recorded float32 runs
(at most 4 x as far from the restatement as the reference itself), at debug percentiles and in seeded random mode; the noise; the pipe
inside the loss's Dmain and Dreg on the real discriminator.  On the parent commit none of this exists."""
import numpy as np
import pytest
import torch

import augment_cases as AC
import augment_pipe_cases as PC
import discriminator_cases as DC
import loss_cases as LC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P():
    import panic3d_amd
    panic3d_amd.build()
    panic3d_amd._lib.lib()
    return panic3d_amd


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(PC.GOLDEN))


@pytest.fixture(scope="module")
def golden_op():
    return dict(np.load(AC.GOLDEN))


@pytest.fixture(scope="module")
def hz(P):
    return P.ops.augment_filter_tables()[0]


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- the operator ---------------------------------------------------------------------------------------------------------------------
ALL = dict(filt=True, noise=True, cutout=True)
# (shape, K, stages, rectangle).  65 x 65: one pixel beyond the 64 x 64 tile of K <= 51; 33 x 65 with 63 taps: beyond the 32-row tile.
TAIL_CASES = [
    ((2, 3, 22, 23), 43, ALL, "inner"), ((1, 1, 22, 22), 43, ALL, "inner"), ((2, 6, 24, 40), 43, ALL, "inner"), ((1, 2, 65, 65), 43, ALL, "inner"),
    ((2, 6, 24, 40), 7, ALL, "inner"), ((1, 2, 65, 65), 7, ALL, "inner"), ((2, 3, 22, 23), 1, ALL, "inner"), ((1, 2, 33, 65), 63, ALL, "inner"),
    ((2, 3, 22, 23), 43, dict(filt=True, noise=False, cutout=False), "inner"), ((2, 3, 22, 23), 43, dict(filt=False, noise=True, cutout=False), "inner"),
    ((2, 3, 22, 23), 43, dict(filt=False, noise=False, cutout=True), "inner"), ((2, 3, 22, 23), 43, ALL, "empty"), ((2, 3, 22, 23), 43, ALL, "all"),
    ((2, 2, 4, 6), 7, ALL, "inner"),
]


@pytest.mark.parametrize("shape,K,stages,rect_kind", TAIL_CASES)
def test_tail_against_float64(P, shape, K, stages, rect_kind):
    x, g, taps, z, sigma, rect = PC.explicit_tail(shape, K, 3, rect_kind=rect_kind, **stages)
    if taps is not None and K > 1:
        assert np.abs(taps - taps[:, ::-1]).max() > 0.01, "a non-symmetric filter"
    R = PC.TailRestated(shape, taps, z, sigma, rect)
    args = (dev(taps), dev(z), dev(sigma), dev(rect))
    xd, gd = dev(x), dev(g)
    y = P.ops.augment_tail(xd, *args)
    gx = P.ops.augment_tail_adjoint(gd, *args)
    torch.cuda.synchronize()
    r_f = AC.worst_ratio(np.abs(y.cpu().numpy() - R.forward(x)), R.bound(x))
    r_a = AC.worst_ratio(np.abs(gx.cpu().numpy() - R.adjoint(g)), R.adjoint_bound(g))
    print(f"{shape} K={K} {stages} {rect_kind}: forward {r_f:.3f} x the gate, adjoint {r_a:.3f} x the gate")
    assert r_f <= 1.0 and r_a <= 1.0
    # bits: run to run, and with autograd
    assert torch.equal(y, P.ops.augment_tail(xd, *args)) and torch.equal(gx, P.ops.augment_tail_adjoint(gd, *args))
    xr = xd.clone().requires_grad_(True)
    yr = P.ops.augment_tail(xr, *args)
    assert yr.requires_grad and torch.equal(yr.detach(), y)
    gr = gd.clone().requires_grad_(True)
    (gx1,) = torch.autograd.grad(yr, xr, gr, create_graph=True)
    assert torch.equal(gx1.detach(), gx), "the backward is the adjoint operator"
    # <A x, g> = <x, A^T g> on the linear part, within the two gates
    lin = y.double() - P.ops.augment_tail(torch.zeros_like(xd), *args).double()
    lhs, rhs = float((lin * gd.double()).sum()), float((gx.double() * xd.double()).sum())
    slack = float((2 * R.bound(x) * np.abs(g)).sum() + (R.adjoint_bound(g) * np.abs(x)).sum())
    assert abs(lhs - rhs) <= slack, (lhs, rhs, slack)
    # a double backward returns the forward's bits: d/dg of <A^T g, w> = A_linear w
    w = torch.from_numpy(AC.images(shape, 9)).cuda()
    (h,) = torch.autograd.grad(gx1, gr, w)
    assert torch.equal(h, P.ops.augment_tail(w, args[0], None, None, args[3]))


def test_tail_with_nothing_is_a_copy_and_errors_come_before_any_launch(P):
    x = dev(AC.images((2, 3, 9, 7), 1))
    y = P.ops.augment_tail(x)
    assert torch.equal(y, x) and y.data_ptr() != x.data_ptr() and torch.equal(P.ops.augment_tail_adjoint(x), x)
    taps = torch.full((2, 43), 1 / 43, device="cuda")
    for shape in ((2, 3, 21, 40), (2, 3, 40, 21), (2, 3, 9, 7)):
        with pytest.raises(RuntimeError, match="P3D_E_RANGE"):
            P.ops.augment_tail(torch.zeros(shape, device="cuda"), taps)
        with pytest.raises(RuntimeError, match="P3D_E_RANGE"):
            P.ops.augment_tail_adjoint(torch.zeros(shape, device="cuda"), taps)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.ops.augment_tail(torch.zeros(2, 3, 22, 22), taps)
    with pytest.raises(RuntimeError):
        P.ops.augment_tail(torch.zeros(2, 3, 22, 22, device="cuda"), taps.cpu())
    with pytest.raises(RuntimeError):
        P.ops.augment_tail(x, None, torch.zeros_like(x), None)
    with pytest.raises(RuntimeError):
        P.ops.augment_tail(x, torch.zeros(2, 4, device="cuda"))


# ---- against the reference's float32 runs ------------------------------------------------------------------------------------------------
def _pipe_case(P, hz, golden, pi, q, exact_taps=False):
    """The restatement of one tail-family case.  The operator test feeds the reference's recorded (float32) taps to the operator, and they
    are the truth's taps too; the module forms its own taps, so there the truth takes them in exact arithmetic from the float32 band gain
    (debug_taps64): the reference's rows and the module's are both roundings of those."""
    shape = PC.TAIL_SHAPES[pi]
    d = P.AugmentPipe(**PC.TAIL_PIPES[pi]).draw(*shape, debug_percentile=q)
    M = m = C = None
    if PC.tail_key("theta", pi, q) in golden:
        m = tuple(int(v) for v in golden[PC.tail_key("margins", pi, q)])
        M = AC.matrix_of_theta(golden[PC.tail_key("theta", pi, q)], shape[2], shape[3], m)
        C = AC.colour_of_rows(golden[PC.tail_key("colour", pi, q)], shape[0])
    taps = PC.debug_taps64(PC.TAIL_PIPES[pi], q, golden["Hz_fbank"], shape[0]) if exact_taps else golden[PC.tail_key("taps", pi, q)]
    assert np.abs(taps - golden[PC.tail_key("taps", pi, q)]).max() < 4e-7 and np.abs(taps - d.taps).max() < 4e-7
    return PC.PipeRestated(hz, shape, None, m, C, taps, d.rect, M=M), d


def _four_times(name, ours, ref, truth):
    """the project's rule: at most 4 x as far from the float64 restatement as the reference's own float32 run"""
    e_ours, e_ref = float(np.abs(ours - truth).max()), float(np.abs(ref - truth).max())
    print(f"{name}: |hip - f64| = {e_ours:.2e}, reference's |f32 - f64| = {e_ref:.2e}, ratio {e_ours / e_ref:.2f}")
    assert e_ours <= 4 * e_ref, name
    return e_ours / e_ref


@pytest.mark.parametrize("pi", [0, 1])
def test_tail_operator_against_the_reference(P, hz, golden, pi):
    """The tail-only pipes of the fixture through ops.augment_tail on the taps the reference recorded."""
    x, g = PC.tail_inputs(pi)
    for q in PC.TAIL_PERCENTILES:
        R, d = _pipe_case(P, hz, golden, pi, q)
        args = (dev(golden[PC.tail_key("taps", pi, q)]), None, None, dev(d.rect))
        y, gx = P.ops.augment_tail(dev(x), *args), P.ops.augment_tail_adjoint(dev(g), *args)
        _four_times(f"tail pipe {pi} q={q} output", y.cpu().numpy(), golden[PC.tail_key("out", pi, q)], R.forward(x))
        _four_times(f"tail pipe {pi} q={q} gradient", gx.cpu().numpy(), golden[PC.tail_key("grad", pi, q)], R.adjoint(g))


def _run_pipe(pipe, x, g, **kw):
    xd = dev(x).requires_grad_(True)
    y = pipe(xd, **kw)
    (gx,) = torch.autograd.grad(y, xd, dev(g))
    return y.detach().cpu().numpy(), gx.cpu().numpy()


@pytest.mark.parametrize("si", range(len(AC.SHAPES)))
def test_pipe_against_the_reference_on_the_trainers_transforms(P, hz, golden_op, si):
    """AugmentPipe(**BGC)(x, debug_percentile=q) on the 18 cases of augment_pipe.npz: output and input gradient."""
    shape = AC.SHAPES[si]
    pipe = P.AugmentPipe(**AC.BGC).cuda()
    x, g = AC.images(shape, si), AC.cotangent(shape, si)
    for q in AC.PERCENTILES:
        m = tuple(int(v) for v in golden_op[AC.key("margins", si, q)])
        M = AC.matrix_of_theta(golden_op[AC.key("theta", si, q)], shape[2], shape[3], m)
        R = AC.Restated(hz, shape, None, m, AC.colour_of_rows(golden_op[AC.key("colour", si, q)], shape[0]), M=M)
        y, gx = _run_pipe(pipe, x, g, debug_percentile=q)
        _four_times(f"BGC shape {si} q={q} output", y, golden_op[AC.key("out", si, q)], R.forward(x))
        _four_times(f"BGC shape {si} q={q} gradient", gx, golden_op[AC.key("grad", si, q)], R.adjoint(g))


@pytest.mark.parametrize("pi", range(len(PC.TAIL_PIPES)))
def test_pipe_against_the_reference_on_the_tail_family(P, hz, golden, pi):
    pipe = P.AugmentPipe(**PC.TAIL_PIPES[pi]).cuda()
    x, g = PC.tail_inputs(pi)
    for q in PC.TAIL_PERCENTILES:
        R, _ = _pipe_case(P, hz, golden, pi, q, exact_taps=True)
        y, gx = _run_pipe(pipe, x, g, debug_percentile=q)
        _four_times(f"pipe {pi} q={q} output", y, golden[PC.tail_key("out", pi, q)], R.forward(x))
        _four_times(f"pipe {pi} q={q} gradient", gx, golden[PC.tail_key("grad", pi, q)], R.adjoint(g))


@pytest.mark.parametrize("si", range(len(PC.RANDOM_SHAPES)))
def test_pipe_in_random_mode_against_the_reference(P, hz, golden, si):
    """The seeded random-mode runs (noise off): the module under the fixture's seed against the reference's output, both measured
    from the float64 restatement of the module's own draw."""
    shape = PC.RANDOM_SHAPES[si]
    pipe = P.AugmentPipe(**PC.RANDOM_PIPE).cuda()
    x = PC.random_inputs(si)
    reads = []
    real = pipe._read_p
    pipe._read_p = lambda: (reads.append(1), real())[1]
    for p in PC.RANDOM_P:
        pipe.p.copy_(torch.as_tensor(p))
        for seed in PC.RANDOM_SEEDS:
            torch.manual_seed(seed)
            d = pipe.draw(*shape)
            R = PC.PipeRestated(hz, shape, d.G_inv, d.margins, d.C, d.taps, d.rect)
            torch.manual_seed(seed)
            with torch.no_grad():
                y = pipe(dev(x)).cpu().numpy()
            _four_times(f"random shape {si} p={p} seed {seed}", y, golden[PC.random_key("out", si, p, seed)], R.forward(x))
    assert len(reads) == len(PC.RANDOM_P), "p is read once per write, not once per call"


def test_noise_is_sigma_z_under_the_mask(P):
    """With noise = 1: the output minus the noise-free output of the same draw is sigma * z * mask, for the z the test's generator
    reproduces; each side is one rounding of values bounded by |f| + |sigma z|."""
    shape = (3, 3, 24, 26)
    pipe = P.AugmentPipe(**AC.BGC, imgfilter=1, noise=1, cutout=1).cuda()
    x = dev(AC.images(shape, 2))
    pipe.noise_generator = torch.Generator(device="cuda").manual_seed(7)
    torch.manual_seed(5)
    y = pipe(x)
    torch.manual_seed(5)
    d = pipe.draw(*shape)
    z = torch.randn(shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(7))
    assert d.sigma is not None and (d.sigma > 0).any() and (d.rect[:, 1] > d.rect[:, 0]).any()
    y0 = pipe.apply_draw(x, d._replace(sigma=None))
    keep = torch.from_numpy(PC.TailRestated(shape, rect=d.rect).keep).cuda()
    want = dev(d.sigma).view(-1, 1, 1, 1).double() * z.double() * keep
    err = ((y.double() - y0.double()) - want).abs()
    assert bool((err <= 2 * 2.0 ** -24 * (y0.abs().double() + want.abs())).all()), float(err.max())
    assert bool((y[keep.expand(shape) == 0] == 0).all()) and float(want.abs().max()) > 0.01
    # a debug percentile sets sigma = erfinv(q) * noise_std for every sample
    assert np.allclose(pipe.draw(*shape, debug_percentile=0.8).sigma, float(torch.erfinv(torch.tensor(0.8)) * 0.1), rtol=1e-6)


# ---- in the loss -------------------------------------------------------------------------------------------------------------------------
class _Seeded:
    """Calls `make(call index)` under a seed of its own per call, so that the module and the stand-in see the same draws."""

    def __init__(self, pipe, fn):
        self.pipe, self.fn, self.calls = pipe, fn, 0

    def __call__(self, images):
        torch.manual_seed(1000 + self.calls)
        self.calls += 1
        return self.fn(images)


@pytest.mark.parametrize("phase", ["Dmain", "Dreg"])
def test_pipe_in_the_loss_on_the_real_discriminator(P, hz, monkeypatch, phase):
    """Dmain and Dreg (R1: a double backward through the pipe) of StyleGAN2LossOrthoCondA on DualDiscriminator at 32^2, with
    augment_pipe=AugmentPipe(**BGC, imgfilter=1, cutout=1) against the same loss with a torch stand-in that applies the module's own drawn
    parameters (augment_cases.torch_operator, augment_pipe_cases.torch_tail): the loss tests' bounds, reported values to 1e-5 of the
    tensor's largest magnitude and gradients to rel-L2 1e-4.  Under Dreg the bound holds the weights, as in test_hip_r1.py's Dreg through
    the loss: the network is piecewise linear in its convolution biases, so their gradients of the penalty reach it through its one smooth
    spot, cancel to almost nothing and carry the two pipes' float32 difference at full size (measured: 9e-4 on every one of them, where
    the weights are within 8.7e-6); they are printed and must be finite."""
    pipe = P.AugmentPipe(**AC.BGC, imgfilter=1, cutout=1).cuda()
    pipe.set_p(0.8)
    results = []
    for kind in ("module", "stand-in"):
        D = DC.fill_discriminator(P.DualDiscriminator(**DC.D_KW)).cuda()
        D.set_r1_grad(True)
        G = LC.StandInG(LC.RK).cuda()
        inp = LC.loss_inputs(device="cuda")
        inp["real_cond"]["resnet_feats"] = torch.randn(LC.N, 16, generator=torch.Generator().manual_seed(12)).cuda()
        reports = {}
        monkeypatch.setattr(P.loss, "report", lambda name, value: reports.__setitem__(name, torch.as_tensor(value).detach().float().cpu()))
        if kind == "module":
            aug = _Seeded(pipe, pipe)
        else:
            aug = _Seeded(pipe, lambda images: PC.torch_pipe(hz, pipe.draw(*images.shape))(images))
        loss = P.StyleGAN2LossOrthoCondA(device=torch.device("cuda"), G=G, D=D, augment_pipe=aug, lpips_model=LC.lpips_stand_in, **LC.LOSS_KW)
        torch.manual_seed(11)
        loss.accumulate_gradients(phase=phase, gain=LC.GAIN, cur_nimg=LC.NIMG["s1.5"], **inp)
        assert aug.calls == (2 if phase == "Dmain" else 1)
        results.append((reports, {n: p.grad.detach().cpu() for n, p in D.named_parameters() if p.grad is not None}))
    (r_mod, g_mod), (r_ref, g_ref) = results
    assert set(r_mod) == set(r_ref) and set(g_mod) == set(g_ref) and g_mod
    for k, v in r_ref.items():
        err = float((r_mod[k] - v).abs().max()) / max(float(v.abs().max()), 1e-30)
        print(f"{phase} {k}: {err:.2e}")
        assert err <= 1e-5, (k, err)
    for k, v in g_ref.items():
        assert torch.isfinite(g_mod[k]).all(), k
        err = LC.rel_l2(g_mod[k], v) if float(v.abs().max()) > 0 else float(g_mod[k].abs().max())
        print(f"{phase} grad {k}: {err:.2e}")
        if phase == "Dmain" or k.endswith(".weight"):
            assert err <= 1e-4, (k, err)
