"""CPU (-m "not gpu"): the augmentation pipe's module without a device — the tail's C ABI (include/p3d_augment_tail.h,
_lib.AUGMENT_TAIL_SIGNATURES and the library's exports), the derived filter bank against the buffer the reference wrote, AugmentPipe.draw
against what the reference recorded of its own runs (debug percentiles and seeded random mode), the float64 restatement of the tail and
the gate that tests/test_hip_augment_pipe.py holds the kernels to (adjoint identity, the reference's runs, seeded faults), the host
mirror of p and the ADA controller.  On the parent commit panic3d_amd.AugmentPipe, ops.augment_tail and the symbols do not exist."""
import os
import re

import numpy as np
import pytest
import torch

import augment_cases as AC
import augment_pipe_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def P():
    import panic3d_amd
    panic3d_amd.build()
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


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_tail_header_table_and_exports_agree(P):
    hdr = open(os.path.join(ROOT, "include", "p3d_augment_tail.h")).read()
    declared = set(re.findall(r"\b(p3d_[a-z0-9_]+)\s*\(", hdr))
    lib = P._lib
    assert declared == set(lib.AUGMENT_TAIL_SIGNATURES) and len(declared) == 3
    others = set()
    for name in dir(lib):
        if name.endswith("SIGNATURES") and name != "AUGMENT_TAIL_SIGNATURES":
            others |= set(getattr(lib, name))
    assert others and not declared & others
    L = lib.lib()
    for name in declared:
        assert hasattr(L, name)
    assert "p3d_augment_tail.hip" in P._build.SOURCES and os.path.join("..", "..", "include", "p3d_augment_tail.h") in P._build.HEADERS
    assert "p3d_augment_tail.hip" not in set(P._build.SYNTHESIS_UNIT) | set(P._build.RENDER_UNIT)
    for name in ("MAX_TAPS", "TILE_W", "MAX_SIDE", "LDS_BYTES"):
        assert int(re.search(rf"#define P3D_TAIL_{name} (\d+)", hdr).group(1)) == getattr(lib, f"P3D_TAIL_{name}")
    assert lib.P3D_ABI_VERSION == 9 and L.p3d_abi_version() == 9, "this change only adds symbols"
    assert callable(P.ops.augment_tail) and callable(P.ops.augment_tail_adjoint) and P.AugmentPipe is P.augment.AugmentPipe


def test_tail_argument_errors_without_gpu(P):
    L = P._lib.lib()
    p, q = 256, 512  # never dereferenced: the checks come first

    def fwd(x=p, taps=p, K=43, z=None, sigma=None, rect=None, N=2, C=3, H=22, W=23, y=q):
        return L.p3d_augment_tail_f32(x, taps, K, z, sigma, rect, N, C, H, W, y, None)

    def adj(x=p, taps=p, K=43, rect=None, N=2, C=3, H=22, W=23, y=q, **_):
        return L.p3d_augment_tail_adjoint_f32(x, taps, K, rect, N, C, H, W, y, None)
    for f in (fwd, adj):
        assert f(x=None) == -1 and f(y=None) == -1 and f(y=p) == -1, "null pointers, in place"
        assert f(N=0) == -1 and f(C=0) == -1 and f(H=0) == -1 and f(W=-1) == -1
        assert f(taps=None) == -1 and f(taps=p, K=0) == -1, "taps and K go together"
        assert f(K=42) == -2 and f(K=65) == -2 and f(K=-1) == -2
        assert f(H=21) == -2 and f(W=21) == -2 and f(K=45) == -2, "R >= min(H, W): the reflect index would leave the image"
        assert f(H=32769) == -2
    assert fwd(z=p) == -1 and fwd(sigma=p) == -1, "the noise needs both"
    out = (P._lib.C.c_int * 4)()
    assert L.p3d_augment_tail_plan(43, out, 3) == -1 and L.p3d_augment_tail_plan(44, out, 4) == -2 and L.p3d_augment_tail_plan(65, out, 4) == -2
    for K in (1, 7, 43, 51, 53, 63):
        th_f, lds_f, th_a, lds_a = P.ops.augment_tail_plan(K)
        R = K // 2
        assert lds_f == 4 * (th_f + 2 * R) * (128 + 2 * R) <= P._lib.P3D_TAIL_LDS_BYTES and th_f in (16, 32, 64)
        assert lds_a == 4 * (2 * th_a + 2 * R) * (64 + 2 * R) <= P._lib.P3D_TAIL_LDS_BYTES and th_a in (16, 32, 64)
        assert th_f == 64 or 4 * (2 * th_f + 2 * R) * (128 + 2 * R) > P._lib.P3D_TAIL_LDS_BYTES, "the tallest tile that fits"
    assert P.ops.augment_tail_plan(43)[0] == 64 and P.ops.augment_tail_plan(63)[0] == 32 and P.ops.augment_tail_plan(0) == (0, 0, 0, 0)
    with pytest.raises(RuntimeError):
        P.ops.augment_tail(torch.zeros(1, 1, 22, 22))  # a CPU tensor: no fall-back


# ---- the buffers ------------------------------------------------------------------------------------------------------------------------
def test_filter_bank_is_derived_and_state_dict_is_the_references(P, golden, golden_op):
    bank = P.augment.fbank()
    ref = golden["Hz_fbank"]
    assert bank.shape == (4, 43) and ref.shape == (4, 43)
    mine = bank.astype(np.float32)
    equal = mine == ref
    small = (np.abs(bank) < 1e-12) & (np.abs(ref.astype(np.float64)) < 1e-12)
    assert (equal | small).all(), "equal to the bit, or both magnitudes below 1e-12 (the mathematically zero taps)"
    assert equal.sum() >= 150 and (~equal).sum() <= 22
    pipe = P.AugmentPipe(**AC.BGC)
    assert list(pipe.state_dict().keys()) == ["p", "Hz_geom", "Hz_fbank"]
    assert pipe.p.shape == () and float(pipe.p) == 1.0 and np.array_equal(pipe.Hz_geom.numpy(), golden_op["Hz_geom"])
    state = {"p": torch.tensor(0.25), "Hz_geom": torch.from_numpy(golden_op["Hz_geom"]), "Hz_fbank": torch.from_numpy(ref)}
    assert not any(pipe.load_state_dict(state, strict=True))
    assert pipe.p_host() == 0.25
    ref_args = dict(xflip=0, rotate90=0, xint=0, xint_max=0.125, scale=0, rotate=0, aniso=0, xfrac=0, scale_std=0.2, rotate_max=1, aniso_std=0.2,
                    xfrac_std=0.125, brightness=0, contrast=0, lumaflip=0, hue=0, saturation=0, brightness_std=0.2, contrast_std=0.5, hue_max=1,
                    saturation_std=1, imgfilter=0, imgfilter_bands=[1, 1, 1, 1], imgfilter_std=1, noise=0, cutout=0, noise_std=0.1, cutout_size=0.5)
    d = P.AugmentPipe()
    for k, v in ref_args.items():
        assert getattr(d, k) == (list(v) if isinstance(v, list) else float(v)), k
    with pytest.raises(ValueError, match="Image must be RGB"):
        P.AugmentPipe(brightness=1).draw(1, 2, 8, 8)
    assert P.AugmentPipe(hue=1).draw(1, 1, 8, 8).C is None, "hue and saturation need more than one channel"


# ---- draw at the recorded debug-percentile cases -----------------------------------------------------------------------------------------
def test_draw_equals_the_recorded_debug_percentile_cases(P, golden_op):
    """The 18 cases of augment_pipe.npz: G_inv through compose against the matrix of the recorded theta (the bound test_augment_cpu.py
    uses for that comparison: float32 rounding of positions of magnitude ~100, 1.2e-5 texels), margins equal, colour rows within the
    float32 rounding of a chain of five 4 x 4 products of entries of magnitude <= 4: 5 * 4 * 4 * 2^-24 = 4.8e-6."""
    pipe = P.AugmentPipe(**AC.BGC)
    for si, shape in enumerate(AC.SHAPES):
        for q in AC.PERCENTILES:
            d = pipe.draw(*shape, debug_percentile=q)
            m = tuple(int(v) for v in golden_op[AC.key("margins", si, q)])
            M = AC.matrix_of_theta(golden_op[AC.key("theta", si, q)], shape[2], shape[3], m)
            e = float(np.abs(AC.compose(d.G_inv, shape[2], shape[3], m) - M).max())
            rows = P.ops.augment_colour_rows  # the device function's rule, restated for the host
            col = golden_op[AC.key("colour", si, q)]
            if shape[1] == 1:
                c1 = d.C[:, :3, :].astype(np.float64).mean(axis=1)
                mine = np.stack([np.array([c1[0, :3].sum(), 0, 0, c1[0, 3]])] * 3)
            else:
                mine = d.C[0, :3, :]
            ce = float(np.abs(mine - col).max())
            print(f"shape {si} q={q}: margins {d.margins}, |compose(G_inv) - M| = {e:.1e}, |colour - recorded| = {ce:.1e}")
            assert d.margins == m and e < 1.2e-5 and ce < 4.8e-6 and rows is not None
            assert d.taps is None and d.sigma is None and d.rect is None and (d.G_inv[1:] == d.G_inv[:1]).all()


# ---- the tail's restatement ----------------------------------------------------------------------------------------------------------------
TAIL_EXPLICIT = [((2, 3, 22, 23), 43), ((1, 1, 22, 22), 43), ((2, 6, 24, 40), 7), ((1, 2, 9, 5), 1), ((2, 2, 4, 6), 7)]


@pytest.mark.parametrize("shape,K", TAIL_EXPLICIT)
def test_tail_restatement_adjoint_identity(shape, K):
    x, g, taps, z, sigma, rect = PC.explicit_tail(shape, K, 3)
    R = PC.TailRestated(shape, taps, z, sigma, rect)
    lin = R.forward(x) - R.forward(0 * x)
    lhs, rhs = (lin * g).sum(), (R.adjoint(g) * x).sum()
    assert abs(lhs - rhs) < 1e-12 * max(abs(lhs), 1.0), "<A x, g> = <x, A^T g>"
    assert (R.forward(x)[R.keep.repeat(shape[1], axis=1) == 0] == 0).all() and (R.keep == 0).any()
    none = PC.TailRestated(shape)
    assert np.array_equal(none.forward(x), x.astype(np.float64)) and np.array_equal(none.adjoint(g), g.astype(np.float64))


def _fold_reference(h, n, m):
    """the header's 1-D adjoint spelled out: the transposed correlation onto the padded axis, then the fold (itself, left, right)"""
    K = len(h)
    R = K // 2
    P_ = {q: sum(h[k] * m[q - k + R] for k in range(K) if 0 <= q - k + R < n) for q in range(-R, n + R)}
    return np.array([P_[i] + (P_[-i] if 1 <= i <= R else 0) + (P_[2 * (n - 1) - i] if n - 1 - R <= i <= n - 2 else 0) for i in range(n)])


def test_fold_convention_is_the_transpose():
    g = np.random.default_rng(5)
    for n, K in ((22, 43), (23, 43), (8, 7), (4, 7), (5, 1), (40, 43)):
        h, m = g.standard_normal(K), g.standard_normal(n)
        assert np.abs(_fold_reference(h, n, m) - PC._axis_matrix(h, n).T @ m).max() < 1e-12
    assert all(1 <= i <= 21 and 22 - 1 - 21 <= i <= 22 - 2 for i in range(1, 21)), "at n = R + 1 every interior pixel has both images"


def recorded_tail_case(P, hz, golden, pi, q):
    """One tail-family case from what the reference recorded (taps, theta, margins, colour rows); the rectangle from draw(), which
    evaluates the reference's own float32 expression per pixel."""
    shape = PC.TAIL_SHAPES[pi]
    d = P.AugmentPipe(**PC.TAIL_PIPES[pi]).draw(*shape, debug_percentile=q)
    M = m = C = None
    if PC.tail_key("theta", pi, q) in golden:
        m = tuple(int(v) for v in golden[PC.tail_key("margins", pi, q)])
        M = AC.matrix_of_theta(golden[PC.tail_key("theta", pi, q)], shape[2], shape[3], m)
        C = AC.colour_of_rows(golden[PC.tail_key("colour", pi, q)], shape[0])
        assert d.margins == m
    return PC.PipeRestated(hz, shape, None, m, C, golden[PC.tail_key("taps", pi, q)], d.rect, M=M), d


def reference_errors(P, hz, golden):
    """(pipe index, q) -> (restatement, draw, the reference's float32 error of its output and of its gradient against it)"""
    out = {}
    for pi in range(len(PC.TAIL_PIPES)):
        x, g = PC.tail_inputs(pi)
        for q in PC.TAIL_PERCENTILES:
            R, d = recorded_tail_case(P, hz, golden, pi, q)
            out[pi, q] = (R, d, float(np.abs(golden[PC.tail_key("out", pi, q)] - R.forward(x)).max()),
                          float(np.abs(golden[PC.tail_key("grad", pi, q)] - R.adjoint(g)).max()))
    return out


@pytest.fixture(scope="module")
def ref_err(P, hz, golden):
    return reference_errors(P, hz, golden)


def test_restatement_equals_the_reference_on_the_tail_family(P, ref_err, golden):
    """The reference's float32 run differs from the float64 restatement by its own rounding only.  Tail-only pipes: the gate's own sum,
    8 sqrt(87) 2^-24 sum|terms| (chains of 2 * 43 + 1 roundings).  With the geometry and colour in front: the bound of
    test_augment_cpu.py for that part (2e-5 outputs, 4e-5 gradients) carried through the filter's absolute gain (sum|h|)^2 (at least 1),
    plus 1e-5 for the tail's own chains (measured on the tail-only pipes: below 1.1e-6).  draw()'s taps equal the recorded ones to float32 rounding of a 4-term product."""
    for (pi, q), (R, d, e_out, e_grad) in ref_err.items():
        x, g = PC.tail_inputs(pi)
        taps = golden[PC.tail_key("taps", pi, q)]
        te = float(np.abs(d.taps - taps).max())
        gain = float(np.abs(taps).sum(axis=1).max()) ** 2
        print(f"pipe {pi} q={q}: reference's |out - f64| = {e_out:.2e}, |grad - f64| = {e_grad:.2e}; |draw taps - recorded| = {te:.1e}; filter's absolute gain {gain:.2f}; rect {d.rect.tolist() if d.rect is not None else None}")
        assert te < 8 * 2.0 ** -24 * float(np.abs(taps).max()) * 4
        if R.head is None:
            assert AC.worst_ratio(np.abs(golden[PC.tail_key("out", pi, q)] - R.forward(x)), R.tail.bound(x)) < 1.0
            assert AC.worst_ratio(np.abs(golden[PC.tail_key("grad", pi, q)] - R.adjoint(g)), R.tail.adjoint_bound(g)) < 1.0
        else:
            assert 1e-8 < e_out < 2e-5 * max(gain, 1.0) + 1e-5 and e_grad < 4e-5 * max(gain, 1.0) + 1e-5
        if d.rect is not None:
            assert ((golden[PC.tail_key("out", pi, q)] == 0) == (R.tail.keep.repeat(PC.TAIL_SHAPES[pi][1], axis=1) == 0)).all(), "the rectangle is the reference's zero set"


def test_torch_composition_of_the_tail_agrees_with_the_restatement():
    """The same steps from torch's own operators (the comparator of tools/bench_augment_pipe.py and the loss test's stand-in), in
    float64: equal to the restatement to float64 rounding, forward, gradient and, through linear_twice, the double backward."""
    shape = (2, 3, 22, 23)
    x, g, taps, z, sigma, rect = PC.explicit_tail(shape, 43, 3)
    R = PC.TailRestated(shape, taps, z, sigma, rect)
    t = lambda a: torch.from_numpy(a).double() if a.dtype != np.int32 else torch.from_numpy(a)
    fn = PC.linear_twice(lambda v: PC.torch_tail(v, t(taps), t(z), t(sigma), t(rect)))
    xt, gt = t(x).requires_grad_(True), t(g).requires_grad_(True)
    y = fn(xt)
    (gx,) = torch.autograd.grad(y, xt, gt, create_graph=True)
    assert np.abs(y.detach().numpy() - R.forward(x)).max() < 1e-12 and np.abs(gx.detach().numpy() - R.adjoint(g)).max() < 1e-12
    (h,) = torch.autograd.grad(gx, gt, t(x))
    assert np.abs(h.numpy() - (R.forward(x) - R.forward(0 * x))).max() < 1e-12


@pytest.mark.parametrize("fault", PC.FAULTS)
def test_tail_gate_rejects_seeded_fault(fault):
    worst = 0.0
    for shape, K in (((2, 3, 22, 23), 43), ((2, 6, 24, 40), 7)):
        x, g, taps, z, sigma, rect = PC.explicit_tail(shape, K, 3)
        R, bad = PC.TailRestated(shape, taps, z, sigma, rect), PC.TailRestated(shape, taps, z, sigma, rect, fault=fault)
        if fault == "no_mirror_images":
            worst = max(worst, AC.worst_ratio(np.abs(bad.adjoint(g) - R.adjoint(g)), R.adjoint_bound(g)))
        else:
            worst = max(worst, AC.worst_ratio(np.abs(bad.forward(x) - R.forward(x)), R.bound(x)))
    print(f"{fault}: {worst:.1f} x the gate")
    assert worst > 1.0


def test_pass_order_is_not_a_fault():
    """Columns before rows, with a non-symmetric filter: the two passes act on different axes, so either order is the same operator.
    No gate can reject it; the kernel's order (rows first) is fixed by its rounding, which the bitwise tests pin."""
    shape = (2, 3, 22, 23)
    x, g, taps, z, sigma, rect = PC.explicit_tail(shape, 43, 3)
    assert np.abs(taps - taps[:, ::-1]).max() > 0.02
    a, b = PC.TailRestated(shape, taps, z, sigma, rect), PC.TailRestated(shape, taps, z, sigma, rect, fault=PC.NOT_A_FAULT)
    assert np.abs(a.forward(x) - b.forward(x)).max() < 1e-13 * np.abs(a.forward(x)).max() + 1e-14


# ---- draw parity in random mode --------------------------------------------------------------------------------------------------------------
def test_random_mode_draws_are_the_references(P, hz, golden, golden_op, ref_err):
    """draw() under the fixture's seeds -> the float64 restatement of the whole pipe -> distance to the reference's recorded output.  The
    bound is 4 x the worst such distance over the debug-percentile cases, whose parameters the reference recorded itself (computed here,
    not a literal).  A wrong draw (order, sign, a missed where, p_rot) moves pixels by 0.1 to 1."""
    worst_debug = max(e for (_, _, e, _) in ref_err.values())
    for si, shape in enumerate(AC.SHAPES):
        for q in AC.PERCENTILES:
            m = tuple(int(v) for v in golden_op[AC.key("margins", si, q)])
            M = AC.matrix_of_theta(golden_op[AC.key("theta", si, q)], shape[2], shape[3], m)
            R = AC.Restated(hz, shape, None, m, AC.colour_of_rows(golden_op[AC.key("colour", si, q)], shape[0]), M=M)
            worst_debug = max(worst_debug, float(np.abs(golden_op[AC.key("out", si, q)] - R.forward(AC.images(shape, si))).max()))
    bound = 4 * worst_debug
    print(f"worst distance over the debug-percentile cases {worst_debug:.2e}: bound {bound:.2e}")
    pipe = P.AugmentPipe(**PC.RANDOM_PIPE)
    fired = set()
    for si, shape in enumerate(PC.RANDOM_SHAPES):
        x = PC.random_inputs(si)
        for p in PC.RANDOM_P:
            pipe.p.copy_(torch.as_tensor(p))
            for seed in PC.RANDOM_SEEDS:
                torch.manual_seed(seed)
                d = pipe.draw(*shape)
                m = tuple(int(v) for v in golden[PC.random_key("margins", si, p, seed)])
                M = AC.matrix_of_theta(golden[PC.random_key("theta", si, p, seed)], shape[2], shape[3], m)
                e_theta = float(np.abs(AC.compose(d.G_inv, shape[2], shape[3], m) - M).max())
                R = PC.PipeRestated(hz, shape, d.G_inv, d.margins, d.C, d.taps, d.rect)
                e = float(np.abs(R.forward(x) - golden[PC.random_key("out", si, p, seed)]).max())
                print(f"shape {si} p={p} seed {seed}: margins {d.margins}, |compose(G_inv) - M| = {e_theta:.1e}, |f64(draw) - reference| = {e:.2e}, rect {d.rect.tolist()}")
                side = 2 * max(shape[3] + m[0] + m[2], shape[2] + m[1] + m[3])  # float32 rounding of positions up to the 2x image's side
                assert d.margins == m and e_theta < side * 2.0 ** -23 and e < bound
                fired |= {("rect", bool(r[1] > r[0])) for r in d.rect} | {("same", bool((d.G_inv[1:] == d.G_inv[:1]).all()))}
    assert ("rect", True) in fired and ("rect", False) in fired and ("same", False) in fired, "the seeds cover a cutout that fired and one that did not"


# ---- p's host mirror and the ADA controller -----------------------------------------------------------------------------------------------
def test_p_is_read_once_and_again_after_a_write(P, monkeypatch):
    pipe = P.AugmentPipe(**AC.BGC, imgfilter=1, cutout=1)
    reads = []
    real = pipe._read_p
    monkeypatch.setattr(pipe, "_read_p", lambda: (reads.append(1), real())[1])
    monkeypatch.setattr(pipe, "apply_draw", lambda images, d, z=None: images)  # a stand-in run: the draws without the device operators
    x = torch.zeros(2, 3, 24, 24)
    pipe(x), pipe(x)
    assert len(reads) == 1, "two forwards, one read"
    pipe.p.copy_(torch.as_tensor(0.5))
    pipe(x), pipe(x)
    assert len(reads) == 2 and pipe.p_host() == 0.5, "the reference loop's augment_pipe.p.copy_(...) is seen"
    pipe.load_state_dict(pipe.state_dict())
    pipe(x)
    assert len(reads) == 3
    P.ada_update(pipe, 0.9, 32, 4, 500, 0.6)
    pipe(x)
    assert len(reads) == 3, "ada_update writes the buffer and the mirror together"
    assert float(pipe.p) == pipe.p_host() == float(np.float32(0.5) + np.float32(32 * 4 / 500000))


def test_ada_update_and_stats_follow_the_formula(P):
    pipe = P.AugmentPipe(xflip=1)
    pipe.set_p(0.0)
    step = np.float32(64 * 4 / (100 * 1000))
    assert P.ada_update(pipe, 0.7, 64, 4, 100, 0.6) == float(step)
    assert P.ada_update(pipe, 0.5, 64, 4, 100, 0.6) == 0.0
    assert P.ada_update(pipe, 0.5, 64, 4, 100, 0.6) == 0.0, "clamped at 0"
    assert P.ada_update(pipe, 0.6, 64, 4, 100, 0.6) == 0.0, "sign(0) = 0"
    seen = []
    stats = P.AdaStats("cpu", previous=lambda name, value: seen.append(name))
    streams = [torch.tensor([1.0, -1.0, 1.0, 1.0]), torch.tensor([[1.0], [1.0]]), torch.tensor([-1.0, 0.0])]
    for s in streams:
        stats.report("Loss/signs/real", s)
        stats.report("Loss/signs/fake", -s)
        stats.report("Loss/D/loss", s.sum())
    assert seen == ["Loss/signs/real", "Loss/signs/fake", "Loss/D/loss"] * 3, "every call is passed on"
    assert stats.mean_and_reset() == pytest.approx(3.0 / 8.0, abs=0) and stats.mean_and_reset() == 0.0
    stats.report("Loss/signs/real", torch.tensor([-1.0, -1.0]))
    p0 = pipe.p_host()
    assert P.ada_update(pipe, stats.mean_and_reset(), 64, 4, 100, 0.6) == max(p0 - float(step), 0.0)
