"""CPU (-m "not gpu"): training the illustration-to-render module without a device — the C ABI of its operators
(include/p3d_rmline_grad.h, _lib.RMLINE_GRAD_SIGNATURES; argument errors come back before any launch), the weight gradient's host-side
plan through a small C++ host, the closed-form backward of tests/rmline_train_cases.py against torch's float64 autograd of the
restatement (RMLineModel and its two autograd Functions run on those closed forms in float64, monkeypatched in place of the
operators), seeded faults against the same gates, and RMLineModel's host logic.  On the parent commit the module does not exist."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import host_build
import rmline_train_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def P():
    import panic3d_amd
    panic3d_amd.build()
    return panic3d_amd


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_header_table_and_exports_agree(P):
    hdr = open(os.path.join(ROOT, "include", "p3d_rmline_grad.h")).read()
    declared = set(re.findall(r"\b(p3d_rmline[a-z0-9_]+)\s*\(", hdr))
    lib = P._lib
    assert declared == set(lib.RMLINE_GRAD_SIGNATURES) and len(declared) == 8
    assert not declared & set(lib.RMLINE_SIGNATURES)
    L = lib.lib()
    for name in declared:
        assert hasattr(L, name)
    B = P._build
    assert "p3d_rmline_grad.hip" in B.SOURCES and os.path.join("..", "..", "include", "p3d_rmline_grad.h") in B.HEADERS
    assert "p3d_rmline_grad_plan.hpp" in B.HEADERS and "p3d_rmline_tile.hpp" in B.HEADERS
    for name in ("BN_MAX_GROUPS", "BN_ROWS", "WG_MAX_SLICES", "OUT_OIHW"):
        assert int(re.search(rf"#define P3D_RMLINE_{name} (\d+)", hdr).group(1)) == getattr(lib, f"P3D_RMLINE_{name}")
    src = open(os.path.join(B.CSRC, "p3d_rmline_grad.hip")).read()
    assert "atomic" not in src.replace("with atomics", "")
    # the tile loop lives in ONE place: both translation units call the header's
    tile = open(os.path.join(B.CSRC, "p3d_rmline_tile.hpp")).read()
    assert tile.count("__builtin_amdgcn_mfma_f32_16x16x4f32") == 1
    assert "rm_tile_mma<MB, R, PT>(" in open(os.path.join(B.CSRC, "p3d_rmline.hip")).read()
    assert "rm_tile_mma<MB, R, true>(" in open(os.path.join(B.CSRC, "p3d_rmline_grad.hip")).read()
    assert P.RMLineModel is P.rmline_train.RMLineModel


def test_argument_errors_without_gpu(P):
    L = P._lib.lib()
    p, q = 256, 260  # never dereferenced: the checks come first; q is not 16-byte aligned
    assert L.p3d_rmline_bn_stats_f32(p, 1, 8, 0.1, p, p, p, p, p, p, 1 << 20, None) == -2        # K = 1
    assert L.p3d_rmline_bn_stats_f32(p, 10, 65, 0.1, p, p, p, p, p, p, 1 << 20, None) == -2      # C > 64
    assert L.p3d_rmline_bn_stats_f32(p, 10, 8, 0.1, p, p, p, None, p, p, 1 << 20, None) == -1    # running statistics come together
    assert L.p3d_rmline_bn_stats_f32(p, 10, 8, 0.1, p, p, p, p, p, p, 16, None) == -3            # workspace
    assert L.p3d_rmline_bn_fold_f32(p, p, p, None, p, p, 1e-5, 4, 4, p, p, None) == -1
    assert L.p3d_rmline_bn_fold_f32(p, p, None, None, None, None, 0.0, 65, 4, p, p, None) == -2
    dg = lambda g=p, Co=32, Ci=32, a=p, slope=0.01, out=p, flags=0: L.p3d_rmline_conv_dgrad_f32(g, 1, 5, 5, Co, p, Ci, a, p, p, slope, flags, out, None)
    assert dg(slope=0.0) == -1 and dg(slope=-0.01) == -1 and dg(slope=float("nan")) == -1
    assert dg(g=q) == -1 and dg(a=q) == -1 and dg(out=q) == -1 and dg(out=q, flags=2, a=None) == -1  # (c0 without a)
    assert dg(Co=65) == -2 and dg(Ci=65) == -2 and dg(flags=4) == -2
    wg = lambda x=p, N=4, Hin=9, Ci=32, Co=32, dz=p, force=0, ws=1 << 24, flags=0: L.p3d_rmline_conv_wgrad_f32(x, None, None, None, N, Hin, Hin, 0, Ci, dz, Co, flags, force, p, p, p, ws, None)
    assert wg(x=q) == -1 and wg(dz=q) == -1 and wg(x=None) == -1
    assert wg(Hin=2) == -2 and wg(Ci=65) == -2 and wg(Co=65) == -2 and wg(force=5) == -2 and wg(force=-1) == -2 and wg(flags=2) == -2
    assert wg(ws=10) == -3
    assert L.p3d_rmline_bn_coef_f32(p, p, p, p, p, p, p, 1e-5, 1, 4, 4, p, p, p, p, p, None) == -1  # K = 1
    assert L.p3d_rmline_head_f32(p, p, p, None, 2, 9, 9, 5, p, p, p, None, None) == -2            # nothing left of the crop
    assert L.p3d_rmline_head_f32(p, p, p, None, 2, 9, 9, 2, p, p, p, p, None) == -1               # a hull's crop without a hull
    assert L.p3d_rmline_head_grad_f32(None, None, None, None, p, None, None, 2, 9, 9, 0, p, None) == -1  # an L1 term without img
    # the forward refuses a map smaller than the filter
    assert L.p3d_rmline_conv_f32(p, None, None, None, 1, 2, 2, 0, 4, p, p, 4, 0, 0.01, 0, 0, p, None) == -2


# ---- the plan ---------------------------------------------------------------------------------------------------------------------------
def test_wgrad_plan_and_its_host_program(P, tmp_path):
    exe = host_build.compile_host(tmp_path, "rmline_grad_plan_host.cpp")

    def run(*a):
        r = subprocess.run([exe] + [str(v) for v in a], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, (a, r.stderr)  # the program itself checks coverage and the LDS indices
        return [ln.split() for ln in r.stdout.splitlines()]
    for N in (1, 2, 3, 8, 511, 512, 513, 2048, 65535):
        for ci, co in ((4, 32), (32, 32), (32, 3), (5, 7), (64, 64), (33, 16)):
            for force in (0, 1, 2, N):
                out = run(N, ci, co, force)
                if force > min(N, 512):
                    assert out == [["error", "-2"]]
                    continue
                assert out[0][0] == "plan" and int(out[0][1]) == (force or min(N, 512)) and len(out) == 1 + int(out[0][1])
                assert int(out[0][2]) == (1 if -(-ci // 16) * -(-co // 16) <= 4 else 4)
                covered = [n for _, _, lo, hi in out[1:] for n in range(int(lo), int(hi))]
                assert covered == list(range(N))  # every patch exactly once, in order
                lib = P.ops.rmline_wgrad_plan(N, ci, co, force)  # the library's answer is the header's
                assert [lib["slices"], lib["sets"], lib["lds_bytes"], lib["ws_floats"]] == [int(out[0][1]), int(out[0][2]), int(out[0][5]), int(out[0][6])]
    assert run(0, 4, 4, 0) == [["error", "-1"]] and run(4, 65, 4, 0) == [["error", "-2"]] and run(4, 4, 4, -1) == [["error", "-2"]]
    assert run(65536, 4, 4, 0) == [["error", "-2"]]
    with pytest.raises(ValueError):
        P.ops.rmline_wgrad_plan(4, 4, 4, 5)


# ---- the closed forms against autograd ------------------------------------------------------------------------------------------------------
def _pair(P, name, seed=0):
    cfg = TC.CONFIGS[name]
    model = TC.perturb(P.RMLineModel(**cfg, seed=seed)).double().train()
    return cfg, model, TC.ref_like(model)


def _compare(model, ref, batch, idx, tol=1e-12):
    """The gate of a whole step: loss, every gradient (rel-L2), who has none, every buffer.  Returns the list of what misses."""
    ml, mg, mb = TC.step_results(model, batch, idx)
    rl, rg, rb = TC.step_results(ref, batch, idx)
    bad = []
    if abs(float(ml) - float(rl)) > tol * max(1.0, abs(float(rl))):
        bad.append(("loss", float(ml), float(rl)))
    for n in rg:
        if (mg[n] is None) != (rg[n] is None):
            bad.append((n, "presence"))
        elif rg[n] is not None and TC.rel_l2(mg[n], rg[n]) > tol:
            bad.append((n, TC.rel_l2(mg[n], rg[n])))
    for n in rb:
        if not torch.allclose(mb[n].double(), rb[n].double(), rtol=tol, atol=0):
            bad.append((n, "buffer"))
    return bad


@pytest.mark.parametrize("name", ["real", "small", "ragged"])
@pytest.mark.parametrize("B", [1, 2])
def test_closed_form_backward_equals_autograd(P, monkeypatch, name, B):
    TC.install_ops(monkeypatch, P.ops)
    cfg, model, ref = _pair(P, name)
    batch = TC.make_batch(cfg, B, dtype=torch.float64)
    for idx in (0, 1):  # the second step starts from the first one's running statistics, in both models
        assert _compare(model, ref, batch, idx) == []
    for n, b in model.named_buffers():
        if n.endswith("num_batches_tracked"):
            assert int(b) == 2  # both steps moved every batch norm of BOTH networks


FAULT_NAMES = ["drop_c1", "biased_running", "taps_not_flipped", "stale_running"]


@pytest.mark.parametrize("fault", FAULT_NAMES)
def test_gate_rejects_operator_faults(P, monkeypatch, fault):
    TC.install_ops(monkeypatch, P.ops)
    cfg, model, ref = _pair(P, "small")
    monkeypatch.setattr(TC, "FAULTS", {fault})
    monkeypatch.setattr(TC, "FAULTS_ARG", {"stale_running": cfg["dis_width"]})  # the discriminator's batch norms stay stale
    bad = _compare(model, ref, TC.make_batch(cfg, 2, dtype=torch.float64), 0)
    assert bad, fault
    names = [b[0] for b in bad]
    if fault in ("biased_running", "stale_running"):
        assert any("running" in n or "num_batches" in n for n in names)
        if fault == "stale_running":
            assert all(n.startswith("discriminator.") for n in names)
    else:
        assert any(n.startswith("generator.") and n.endswith("weight") for n in names)


def test_gate_rejects_plain_targets_and_a_generator_step_on_both_patches(P, monkeypatch):
    TC.install_ops(monkeypatch, P.ops)
    cfg, model, ref = _pair(P, "small")
    batch = TC.make_batch(cfg, 2, dtype=torch.float64)
    rl, _, _ = TC.step_results(ref, batch, 1)
    real = torch.nn.functional.binary_cross_entropy_with_logits
    monkeypatch.setattr(torch.nn.functional, "binary_cross_entropy_with_logits", lambda x, t, **kw: real(x, (t > 0.8).to(x.dtype), **kw))  # 0 / 1
    model2 = TC.perturb(P.RMLineModel(**cfg)).double().train()
    ml, _, _ = TC.step_results(model2, batch, 1)
    assert abs(float(ml) - float(rl)) > 1e-3
    monkeypatch.setattr(torch.nn.functional, "binary_cross_entropy_with_logits", real)
    # the generator's step on both patches of a pair, labels forced to 1
    flat = {k: v.reshape(-1, *v.shape[2:]) for k, v in batch.items()}
    flat["real_label"] = torch.ones_like(flat["real_label"])
    model3 = TC.perturb(P.RMLineModel(**cfg)).double().train()
    wrong = model3.loss(model3.forward(flat), flat)["loss"].mean()
    ref3 = TC.ref_like(TC.perturb(P.RMLineModel(**cfg)).double())
    right = ref3.training_step(batch, 0, 0)
    assert abs(float(wrong) - float(right)) > 1e-4


# ---- RMLineModel's host logic ----------------------------------------------------------------------------------------------------------------
def test_model_host_logic(P, monkeypatch):
    TC.install_ops(monkeypatch, P.ops)
    cfg = TC.CONFIGS["small"]
    model = P.RMLineModel(**cfg).double().train()
    ref = TC.ref_like(model)
    assert list(model.state_dict()) == list(ref.state_dict())  # the reference's keys, generator.N.* and discriminator.N.*
    assert [type(m) for m in model.generator] == [type(m) for m in ref.generator] and [type(m) for m in model.discriminator] == [type(m) for m in ref.discriminator]
    d = P.RMLineModel()
    assert (d.patch_size, d.gen_depth, d.gen_width, d.dis_depth, d.dis_width, d.label_smoothing, d.lr_gen, d.lr_dis, d.lambda_l1, d.lambda_adv, d.size) == \
        (9, 6, 32, 4, 16, 0.8, 1e-3, 1e-3, 1.0, 1.0, 21)
    assert torch.equal(d.generator[0].weight, P.RMLineGenerator().generator[0].weight)  # seeded alike
    with pytest.raises(AssertionError):
        P.RMLineModel(patch_size=9, gen_depth=6, size=20)  # the reference's assertion: 9 + 12 > 20
    for switch in ("gen_batchnorm", "gen_use_hull", "gen_mask_input", "dis_batchnorm", "dis_use_hull", "lerp_output"):
        with pytest.raises(NotImplementedError):
            P.RMLineModel(**{switch: False})
    # batch slicing and the label flip: what reaches forward / loss in each step
    seen = []
    real_loss = model.loss
    monkeypatch.setattr(model, "loss", lambda pred, gt: (seen.append({k: v.clone() for k, v in gt.items()}), real_loss(pred, gt))[1])
    batch = TC.make_batch(cfg, 3, dtype=torch.float64)
    opts = [torch.optim.Adam(model.generator.parameters(), lr=1e-3), torch.optim.Adam(model.discriminator.parameters(), lr=1e-3)]
    flags = []
    real_step = model.training_step
    monkeypatch.setattr(model, "training_step", lambda b, i, idx: (flags.append(([p.requires_grad for p in model.generator.parameters()],
                                                                                 [p.requires_grad for p in model.discriminator.parameters()])),
                                                                   real_step(b, i, idx))[1])
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    losses = model.fit_step(batch, opts)
    assert len(losses) == 2 and len(seen) == 2
    assert torch.equal(seen[0]["image"], batch["image"][:, 0]) and torch.equal(seen[0]["real_label"], torch.ones(3, dtype=torch.float64))
    assert torch.equal(seen[1]["image"], batch["image"].reshape(6, 3, 9, 9)) and torch.equal(seen[1]["real_label"], batch["real_label"].reshape(6))
    assert all(flags[0][0]) and not any(flags[0][1]) and not any(flags[1][0]) and all(flags[1][1])  # toggled ...
    assert all(p.requires_grad for p in model.parameters())                                       # ... and restored
    assert all(not torch.equal(before[n], p) for n, p in model.named_parameters())                # both optimisers stepped
    # the same fit_step as the restatement's, parameters and all
    ropts = [torch.optim.Adam(ref.generator.parameters(), lr=1e-3), torch.optim.Adam(ref.discriminator.parameters(), lr=1e-3)]
    rl = ref.fit_step(batch, ropts)
    assert abs(float(rl[0]) - float(losses[0])) < 1e-12 and abs(float(rl[1]) - float(losses[1])) < 1e-12
    for (n, a), (_, b) in zip(model.state_dict().items(), ref.state_dict().items()):
        assert torch.allclose(a, b, rtol=1e-9, atol=1e-12), n
    # errors
    x = {k: v[:, 0].clone() for k, v in batch.items()}
    x["image"].requires_grad_(True)
    with pytest.raises(NotImplementedError):
        model.forward(x)
    one = {k: v[:1, 0, ..., :3, :3].contiguous() for k, v in batch.items() if k != "real_label"}
    with pytest.raises(ValueError):  # one 3 x 3 patch without padding leaves a 1 x 1 map: one value per channel, as torch raises
        model.forward(one, pad=False)
    with pytest.raises(ValueError):
        model.fit_step(batch, opts[:1])
    cfgd = model.configure_optimizers.__doc__
    assert "Adam" in cfgd
