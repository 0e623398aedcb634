"""GPU: the optimiser step's kernel (csrc/p3d_optim.hip) against the float64 restatement of tests/optim_cases.py under the project's gate,
its bit-level promises (skipped tensors, the 4-byte path, w = 0 and w = 1, the fused launch, run to run), the five-step trajectory
against torch.optim.Adam in float64, and what the module is for: every parameter-derived cache of the package sees a step without
clear_memo().  On the parent commit panic3d_amd.optim and the exports do not exist."""
import copy
import json
import os
import subprocess
import sys

import pytest
import torch

import optim_cases as OC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")]
C = OC.CHUNK


@pytest.fixture(scope="module")
def P():
    import panic3d_amd
    panic3d_amd._lib.lib()
    return panic3d_amd


def _state(numels, seed, moments=True):
    """p, m, v on the device: m and v as an optimiser would hold them after some steps (v >= 0)."""
    ps = [t.cuda() for t in OC.make_params(numels, seed)]
    if not moments:
        return ps, [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps]
    return ps, [t.cuda() * 0.1 for t in OC.make_params(numels, seed + 1)], [t.cuda().square() * 0.01 for t in OC.make_params(numels, seed + 2)]


def _adam(P, ps, gs, ms, vs, step, betas, **kw):
    ss, bc = OC.bias_corrections(OC.LR, betas[0], betas[1], step)
    return P.ops.adam_ema_step(ps, gs, ms, vs, [ss] * len(ps), [bc] * len(ps), beta1=betas[0], beta2=betas[1], eps=OC.EPS, **kw)


def _bits(ts):
    return [t.detach().clone() for t in ts]


def _same(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


# ---- one step against float64 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("betas", OC.BETAS)
def test_one_step_against_float64(P, betas):
    """Steps 1 .. 5 of every numel of the list (the zero-numel parameter rides along), each compared from the kernel's own previous state."""
    ps, ms, vs = _state(OC.NUMELS, 1, moments=False)
    table, bad, zeros = None, [], 0
    for step in range(1, 6):
        gs = [OC.make_grad(n, 10 * step + i).cuda() for i, n in enumerate(OC.NUMELS)]
        p0, m0, v0 = _bits(ps), _bits(ms), _bits(vs)
        table = _adam(P, ps, gs, ms, vs, step, betas, table=table)
        for i, n in enumerate(OC.NUMELS):
            if n == 0:
                continue
            r = OC.step_f64(p0[i].cpu(), m0[i].cpu(), v0[i].cpu(), gs[i].cpu(), OC.LR, betas[0], betas[1], OC.EPS, step)
            for name, got, key in (("p", ps[i], "p"), ("m", ms[i], "m"), ("v", vs[i], "v")):
                bad += OC.gate(f"step {step} {name}[{n}]", got, r[key], r[key + "_abs"], verbose=False)
            if betas[0] == 0:
                assert torch.equal(ms[i], gs[i]), "beta1 == 0: m is the gradient, bit for bit"
            still = (gs[i] == 0) & (v0[i] == 0)
            zeros += int(still.sum())
            assert torch.equal(ps[i][still].view(torch.int32), p0[i][still].view(torch.int32)), "g = 0 and v0 = 0: p unchanged"
    assert bad == [] and zeros >= 5 * len(OC.NUMELS) - 5
    assert table.n_chunks == 17 and table.n == len(OC.NUMELS)


def test_a_tensor_without_a_gradient_is_untouched(P):
    numels = [C + 5, 2 * C + 3, 70]
    for betas in ((0.0, 0.99), (0.9, 0.999)):
        ps, ms, vs = _state(numels, 5)
        before = _bits(ps + ms + vs)
        gs = [OC.make_grad(numels[0], 1).cuda(), None, OC.make_grad(numels[2], 3).cuda()]
        _adam(P, ps, gs, ms, vs, 3, betas)
        after = ps + ms + vs
        for k in range(9):
            same = torch.equal(after[k].view(torch.int32), before[k].view(torch.int32))
            assert same == (k % 3 == 1), ("p", "m", "v")[k // 3] + str(k % 3)


def test_unaligned_views_and_strided_gradients_give_the_same_bits(P):
    numels = [2 * C + 5, C, 300]
    betas = (0.9, 0.999)
    gs = [OC.make_grad(n, 20 + i).cuda() for i, n in enumerate(numels)]
    ps, ms, vs = _state(numels, 7)
    ref_p, ref_m, ref_v = _bits(ps), _bits(ms), _bits(vs)
    _adam(P, ref_p, gs, ref_m, ref_v, 2, betas)
    assert all(g.data_ptr() % 16 == 0 for g in gs)
    for off in (1, 2, 3):  # segments of one flat vector at float offsets 1, 2, 3: the 4-byte path for the gradient alone
        flat = torch.zeros(off + sum(numels) + 8, device="cuda")
        views, at = [], off
        for g in gs:
            views.append(flat[at:at + g.numel()])
            views[-1].copy_(g)
            at += g.numel() + (1 if off == 2 else 0)
        assert views[0].data_ptr() % 16 == 4 * off
        p, m, v = _bits(ps), _bits(ms), _bits(vs)
        _adam(P, p, views, m, v, 2, betas)
        assert _same(p + m + v, ref_p + ref_m + ref_v), off
    # the state itself at a 4-byte offset
    hold = [torch.zeros(1 + sum(numels), device="cuda") for _ in range(3)]
    p, m, v = ([h[1 + sum(numels[:i]):1 + sum(numels[:i + 1])] for i in range(3)] for h in hold)
    for dst, src in zip(p + m + v, ps + ms + vs):
        dst.copy_(src)
    assert p[0].data_ptr() % 16 == 4
    _adam(P, p, gs, m, v, 2, betas)
    assert _same(p + m + v, ref_p + ref_m + ref_v)
    # a transposed gradient is copied first: the same bits as its contiguous copy
    pt, mt, vt = _state([64 * 65], 9)
    g2 = OC.make_grad(64 * 65, 30).cuda().reshape(65, 64).t()
    assert not g2.is_contiguous()
    a = [_bits(x) for x in (pt, mt, vt)]
    _adam(P, pt, [g2], mt, vt, 1, betas)
    _adam(P, a[0], [g2.contiguous()], a[1], a[2], 1, betas)
    assert _same(pt + mt + vt, a[0] + a[1] + a[2])


def test_sanitising_scales_first_and_leaves_finite_values(P):
    n = C + 9
    for betas in ((0.0, 0.99), (0.9, 0.999)):
        ps, ms, vs = _state([n], 11)
        g = OC.make_grad(n, 40)
        special = torch.tensor([float("nan"), float("inf"), -float("inf"), 3e7, -3e7])
        for at in (0, 1000, C - 2, C + 4):  # on both paths: the full chunk and the tail
            g[at:at + 5] = special
        p0, m0, v0 = _bits(ps), _bits(ms), _bits(vs)
        _adam(P, ps, [g.cuda()], ms, vs, 2, betas, grad_scale=0.5, sanitize=OC.SANITIZE)
        r = OC.step_f64(p0[0].cpu(), m0[0].cpu(), v0[0].cpu(), g, OC.LR, betas[0], betas[1], OC.EPS, 2, grad_scale=0.5, sanitize=OC.SANITIZE)
        assert r["g"][0] == 0 and r["g"][1] == 1e5 and r["g"][2] == -1e5 and r["g"][3] == 1.5e7 and r["g"][4] == -1.5e7
        bad = []
        for name, got in (("p", ps[0]), ("m", ms[0]), ("v", vs[0])):
            assert bool(torch.isfinite(got).all()), name
            bad += OC.gate(f"sanitised {name}", got, r[name], r[name + "_abs"], verbose=False)
        assert bad == []
        # 3e7 * 0.5 was not clamped to 1e5: v holds (1 - beta2) * (1.5e7)^2, 22500 times what a clamped value would leave
        assert float(vs[0][3]) > 0.9 * (1 - betas[1]) * 1.5e7 ** 2 and float(vs[0][C + 8]) > 0.9 * (1 - betas[1]) * 1.5e7 ** 2
        # without sanitising the non-finite values go through
        p, m, v = _bits(p0), _bits(m0), _bits(v0)
        _adam(P, p, [g.cuda()], m, v, 2, betas, grad_scale=0.5)
        assert not bool(torch.isfinite(p[0][:3]).any()) and bool(torch.isfinite(p[0][3:1000]).all())


def test_five_step_trajectory_against_torch_adam_in_float64(P):
    numels = [n for n in OC.NUMELS if n]
    betas = (0.0, 0.99)
    start = OC.make_params(numels, 13)
    grads = [[OC.make_grad(n, 50 * s + i) for i, n in enumerate(numels)] for s in range(5)]
    ours = [torch.nn.Parameter(t.clone().cuda()) for t in start]
    dev = [torch.nn.Parameter(t.clone().cuda()) for t in start]
    ref = [torch.nn.Parameter(t.clone().double()) for t in start]
    opts = [P.optim.Adam(ours, lr=OC.LR, betas=betas, eps=OC.EPS), torch.optim.Adam(dev, lr=OC.LR, betas=betas, eps=OC.EPS),
            torch.optim.Adam(ref, lr=OC.LR, betas=betas, eps=OC.EPS)]
    for s in range(5):
        for xs, opt in zip((ours, dev, ref), opts):
            for x, g in zip(xs, grads[s]):
                x.grad = g.to(x.device, x.dtype)
            opt.step()
    cat = lambda xs: torch.cat([x.detach().double().cpu() for x in xs])
    e_ours, e_dev = (float((cat(xs) - cat(ref)).norm() / cat(ref).norm()) for xs in (ours, dev))
    print(f"five steps, rel-L2 of p against float64: fused {e_ours:.3e}, torch.optim.Adam on the device {e_dev:.3e} (not gated)")
    assert e_ours <= 1e-6
    assert float((cat(ours) - torch.cat(start).double()).norm()) > 1e-3, "the parameters moved"


# ---- the EMA ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", OC.EMA_WEIGHTS)
def test_ema_against_float64(P, w):
    numels = [n for n in OC.NUMELS if n]
    ps = [t.cuda() for t in OC.make_params(numels, 15)]
    es = [t.cuda() for t in OC.make_params(numels, 16)]
    ps[3][0], es[3][1], ps[3][2] = -0.0, -0.0, float("inf")  # signed zeros and an infinity survive the two ends
    p0, e0 = _bits(ps), _bits(es)
    P.ops.adam_ema_step(ps, ema_params=es, ema_weights=[w] * len(ps))
    assert _same(ps, p0), "the EMA launch does not write p"
    bad = []
    for i, n in enumerate(numels):
        keep = torch.isfinite(p0[i].cpu())
        r = OC.ema_f64(p0[i].cpu(), e0[i].cpu(), w)
        bad += OC.gate(f"ema w={w} [{n}]", es[i].cpu()[keep], r["e"][keep], r["e_abs"][keep], verbose=False)
    assert bad == []
    if w == 0:
        assert _same(es, p0), "w = 0 copies p bit for bit"
    if w == 1:
        assert _same(es, e0), "w = 1 leaves e bit for bit"


def test_fused_launch_equals_adam_then_ema(P):
    numels = [C + 5, 2 * C, 70, 1]
    for betas in ((0.0, 0.99), (0.9, 0.999)):
        ps, ms, vs = _state(numels, 17)
        es = [t.cuda() for t in OC.make_params(numels, 20)]
        gs = [OC.make_grad(n, 60 + i).cuda() for i, n in enumerate(numels)]
        gs[1] = None  # skipped by Adam; its EMA copy still follows p
        ws = [0.99778, 0.3, 0.0, 0.5]
        ss, bc = OC.bias_corrections(OC.LR, betas[0], betas[1], 4)
        kw = dict(beta1=betas[0], beta2=betas[1], eps=OC.EPS, sanitize=OC.SANITIZE)
        a = [_bits(x) for x in (ps, ms, vs, es)]
        P.ops.adam_ema_step(a[0], gs, a[1], a[2], [ss] * 4, [bc] * 4, ema_params=a[3], ema_weights=ws, **kw)
        b = [_bits(x) for x in (ps, ms, vs, es)]
        P.ops.adam_ema_step(b[0], gs, b[1], b[2], [ss] * 4, [bc] * 4, **kw)
        P.ops.adam_ema_step(b[0], ema_params=b[3], ema_weights=ws)
        assert _same(sum(a, []), sum(b, []))
        assert not torch.equal(a[3][1], es[1]) and torch.equal(a[0][1], ps[1]), "the skipped tensor: p kept, e moved"
        # run to run: the same call from the same state gives the same bits
        c = [_bits(x) for x in (ps, ms, vs, es)]
        P.ops.adam_ema_step(c[0], gs, c[1], c[2], [ss] * 4, [bc] * 4, ema_params=c[3], ema_weights=ws, **kw)
        assert _same(sum(a, []), sum(c, []))


class _Toy(torch.nn.Module):
    def __init__(self, seed):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.a = torch.nn.Parameter(torch.randn(70, 65, generator=g))
        self.b = torch.nn.Parameter(torch.randn(1, generator=g))
        self.register_buffer("avg", torch.randn(C + 3, generator=g))
        self.register_buffer("count", torch.tensor([seed], dtype=torch.int64))
        self.neural_rendering_resolution = 64 + seed
        self.rendering_kwargs = {"seed": seed}


def test_update_ema_against_the_reference_loop(P):
    beta = 0.99778
    G, G_ema = _Toy(1).cuda(), _Toy(2).cuda()
    ref, e0 = copy.deepcopy(G_ema), copy.deepcopy(G_ema)
    OC.reference_update_ema(ref, G, beta)
    versions = [t._version for t in list(G_ema.parameters()) + [G_ema.avg]]
    P.optim.update_ema(G_ema, G, beta)
    P.optim.update_ema(ref, G, 1.0)  # w = 1 on parameters: nothing moves
    bad = []
    for (n, a), b, e in zip(G_ema.named_parameters(), ref.parameters(), e0.parameters()):
        r = OC.ema_f64(dict(G.named_parameters())[n].detach().cpu(), e.detach().cpu(), beta)
        bad += OC.gate(f"update_ema {n}", a.detach(), r["e"], r["e_abs"], verbose=False)
        bad += OC.gate(f"torch's loop {n}", b.detach(), r["e"], r["e_abs"], verbose=False)
    assert bad == []
    assert torch.equal(G_ema.avg, G.avg) and torch.equal(G_ema.count, G.count) and G_ema.count.dtype == torch.int64, "buffers are copied exactly"
    assert all(t._version > v for t, v in zip(list(G_ema.parameters()) + [G_ema.avg], versions))
    assert G_ema.neural_rendering_resolution == 65 and G_ema.rendering_kwargs == {"seed": 1} and G_ema.rendering_kwargs is not G.rendering_kwargs


# ---- the caches see it ------------------------------------------------------------------------------------------------------------------
def test_mapping_memo_sees_a_step_without_clear_memo(P):
    import train_step_cases as TC
    from panic3d_amd.generator import TriPlaneGenerator
    G = TC.fill_mapping(TriPlaneGenerator(**TC.mapping_kw(2)).eval(), 7).cuda()
    mp = G.backbone.mapping
    inp = {k: v.cuda() for k, v in TC.mapping_inputs(G.backbone.num_ws, 8).items()}
    call = lambda: G.mapping_zplus(inp["zs"], inp["c"], {"resnet_feats": inp["feats"]}, truncation_psi=TC.PSI, truncation_cutoff=TC.CUTOFF)
    with torch.no_grad():
        cold = call().clone()
    memo = mp.fc0._scaled_wb
    (call() * inp["g_ws"]).sum().backward()
    with torch.no_grad():
        assert torch.equal(call(), cold) and mp.fc0._scaled_wb is memo
    opt = P.optim.Adam(G.parameters(), lr=0.05, betas=(0.0, 0.99))  # (every parameter outside the mapping network has no gradient: skipped)
    opt.step()
    with torch.no_grad():
        stepped = call().clone()
    assert not torch.equal(stepped, cold) and mp.fc0._scaled_wb is not memo, "the memoised pre-scaled weights were replaced without clear_memo()"
    fresh = TriPlaneGenerator(**TC.mapping_kw(2)).eval().cuda()
    fresh.load_state_dict(G.state_dict())
    with torch.no_grad():
        want = fresh.mapping_zplus(inp["zs"], inp["c"], {"resnet_feats": inp["feats"]}, truncation_psi=TC.PSI, truncation_cutoff=TC.CUTOFF)
    assert torch.equal(stepped, want)


def _view(G, cond, n):
    torch.manual_seed(1000 + n)
    x = dict(seeds=[4], cond=cond, elevations=torch.zeros(1, device="cuda"), azimuths=torch.zeros(1, device="cuda"), neural_rendering_resolution=16,
             noise_mode="const", triplane_crop=0.1, cull_clouds=0.5)
    return G.f(x)


def _replays(G):
    vg = G.__dict__.get("_view_graphs")
    return sum(e.get("replays", 0) for e in vg["entries"].values()) if vg else 0


def test_replayed_views_see_a_step_and_an_ema_update(P):
    import p3d_shared_cases as MC
    import p3d_testing as T
    g = torch.Generator().manual_seed(3)
    cond = {"image_ortho_front": torch.rand(1, 3, 32, 32, generator=g).cuda(), "resnet_feats": torch.randn(1, 16, generator=g).cuda()}

    def fresh_image(state):
        F = MC.memo_generator("cuda")
        F.load_state_dict(state)
        F.set_view_replay(False)
        with torch.no_grad():
            return _view(F, cond, 9)["image"].clone()

    def warm(G):
        with torch.no_grad():
            for n in (1, 2, 3):
                _view(G, cond, n)
            return _view(G, cond, 9)["image"].clone()

    G = MC.memo_generator("cuda")
    T.fill_generator_params(G, 3)
    G.set_view_replay(True)
    G_ema = copy.deepcopy(G)
    G_ema.set_view_replay(True)
    before, before_ema = warm(G), warm(G_ema)
    assert _replays(G) > 0 and _replays(G_ema) > 0, "the views were replays"
    assert torch.equal(before, before_ema)
    out = _view(G, cond, 5)  # a real gradient: the render-resolution outputs (the super-resolution gets none and is skipped)
    (out["image_raw"].square().mean() + out["image_weights"].mean()).backward()
    opt = P.optim.Adam(G.parameters(), lr=0.01, betas=(0.0, 0.99))
    assert any(p.grad is None for p in G.parameters()) and any(p.grad is not None for p in G.parameters())
    P.optim.phase_step(G, opt)
    with torch.no_grad():
        after = _view(G, cond, 9)["image"].clone()
    assert not torch.equal(after, before), "the image changed"
    assert torch.equal(after, fresh_image(G.state_dict())), "the view after the step is the stepped generator's view"
    P.optim.update_ema(G_ema, G, 0.5)
    with torch.no_grad():
        after_ema = _view(G_ema, cond, 9)["image"].clone()
    assert not torch.equal(after_ema, before_ema) and not torch.equal(after_ema, after)
    assert torch.equal(after_ema, fresh_image(G_ema.state_dict()))


# ---- a real gradient set ------------------------------------------------------------------------------------------------------------------
def test_phase_step_on_the_discriminator_against_torch_adam(P):
    import discriminator_cases as DC
    D = DC.fill_discriminator(P.DualDiscriminator(**DC.D_KW)).cuda()
    D.b4.out.bias.requires_grad_(False)  # a parameter without a gradient
    inp = DC.discriminator_inputs()
    logits = D({"image": inp["image"].cuda(), "image_raw": inp["image_raw"].cuda()}, inp["c"].cuda(), {"resnet_feats": inp["feats"].cuda()})
    (logits * inp["g"].cuda()).sum().backward()
    twin = copy.deepcopy(D)
    for p, q in zip(D.parameters(), twin.parameters()):
        q.grad = None if p.grad is None else p.grad.clone()
    start = {n: p.detach().clone() for n, p in D.named_parameters()}
    kw = dict(lr=0.002, betas=(0.0, 0.99), eps=1e-8)
    opt = P.optim.Adam(D.parameters(), **kw)
    P.optim.phase_step(D, opt)
    torch.optim.Adam(twin.parameters(), **kw).step()
    bad, stepped = [], 0
    for (n, p), q in zip(D.named_parameters(), twin.parameters()):
        if p.grad is None:
            assert torch.equal(p.detach().view(torch.int32), start[n].view(torch.int32)) and p not in opt.state, n
            continue
        stepped += 1
        z = torch.zeros(p.numel())
        r = OC.step_f64(start[n].cpu().flatten(), z, z, p.grad.cpu().flatten(), 0.002, 0.0, 0.99, 1e-8, 1)
        bad += OC.gate(n, p.detach().flatten(), q.detach().double().cpu().flatten(), r["p_abs"], verbose=False)
        bad += OC.gate(n + " vs float64", p.detach().flatten(), r["p"], r["p_abs"], verbose=False)
        assert not torch.equal(p.detach(), start[n])
    assert bad == [] and stepped == len(start) - 1 and len(opt._tables) == 1


# ---- RCCL ---------------------------------------------------------------------------------------------------------------------------------
RANK_SCRIPT = r'''
import json, os, sys
for p in (%r, %r):
    sys.path.insert(0, p)
import torch, torch.distributed as dist
import panic3d_amd as P
import optim_cases as OC
dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
torch.cuda.set_device(dev)
dist.init_process_group("nccl", device_id=dev)
numels = [5, 4096 + 3, 0, 2 * 4096, 70]
def run(flat):
    mod = torch.nn.ParameterList([torch.nn.Parameter(t.to(dev)) for t in OC.make_params(numels, 31)])
    opt = P.optim.Adam(mod.parameters(), lr=0.002, betas=(0.0, 0.99))
    for step in (1, 2):
        for i, p in enumerate(mod):
            p.grad = None if i == 4 and step == 2 else OC.make_grad(p.numel(), 70 * step + i).to(dev)
        mod[0].grad[:3] = torch.tensor([float("nan"), float("inf"), 3e7], device=dev)
        P.optim.phase_step(mod, opt, num_gpus=1, flat=flat)
    return [p.detach().clone() for p in mod] + [opt.state[p][k] for p in mod for k in ("exp_avg", "exp_avg_sq")]
a, b = run(False), run(True)
torch.cuda.synchronize()
out = {"backend": dist.get_backend(), "world": dist.get_world_size(),
       "same_bits": all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b)),
       "finite": all(bool(torch.isfinite(x).all()) for x in a), "moved": not torch.equal(a[1], OC.make_params(numels, 31)[1].to(dev))}
dist.barrier()
dist.destroy_process_group()
print(json.dumps(out))
'''


def test_flat_path_on_rccl_in_a_one_rank_group(tmp_path):
    """phase_step's multi-GPU path (torch.cat -> all_reduce on RCCL -> one launch over the segments of the flat vector) forced on with one
    rank: the same bits as the direct path.  (The arithmetic of a world of two: tests/test_optim_cpu.py on gloo.)"""
    script = tmp_path / "rank.py"
    script.write_text(RANK_SCRIPT % (ROOT, os.path.join(ROOT, "tests")))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1", "--master-addr", "127.0.0.1", "--master-port", "29583",
           str(script)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert out["backend"] == "nccl" and out["world"] == 1
    assert out["same_bits"] and out["finite"] and out["moved"]
