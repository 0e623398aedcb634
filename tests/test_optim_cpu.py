"""CPU (-m "not gpu"): the optimiser step without a device — the C ABI of include/p3d_optim.h (header, _lib.OPTIM_SIGNATURES and the
library's exports; struct layouts; argument errors before any launch), the chunk plan of csrc/p3d_optim_plan.hpp compiled into a host
program, and the host logic of panic3d_amd/optim.py on a numpy stand-in of the launch (tests/optim_cases.py) against torch.optim.Adam
in float64: skipped parameters, state_dict exchange, param groups, edited lr / betas, the order of / num_gpus and nan_to_num on gloo,
the helpers, and the version bump that is the point of the module.  On the parent commit the module, the table and the symbols do not
exist."""
import copy
import ctypes as C
import json
import os
import re
import subprocess
import sys

import pytest
import torch

import optim_cases as OC
from host_build import compile_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def P():
    import panic3d_amd
    panic3d_amd.build()
    return panic3d_amd


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_optim_header_table_and_exports_agree(P):
    hdr = open(os.path.join(ROOT, "include", "p3d_optim.h")).read()
    declared = set(re.findall(r"\b(p3d_optim_[a-z0-9_]+)\s*\(", hdr))
    lib = P._lib
    assert declared == set(lib.OPTIM_SIGNATURES) and len(declared) == 4
    others = set(lib.SIGNATURES) | set(lib.GRAD_SIGNATURES) | set(lib.SYN_GRAD_SIGNATURES) | set(lib.PASTE_GRAD_SIGNATURES) | set(lib.DISC_SIGNATURES) \
        | set(lib.LOSS_SIGNATURES)
    assert not declared & others
    L = lib.lib()
    for name in declared:
        assert hasattr(L, name)
    B = P._build
    assert "p3d_optim.hip" in B.SOURCES and "p3d_optim_plan.hpp" in B.HEADERS and os.path.join("..", "..", "include", "p3d_optim.h") in B.HEADERS
    for unit in (B.RENDER_UNIT, B.SYNTHESIS_UNIT):
        assert not any("p3d_optim" in s for s in unit)
    assert int(re.search(r"#define P3D_OPTIM_CHUNK (\d+)", hdr).group(1)) == lib.P3D_OPTIM_CHUNK == OC.CHUNK
    for name in ("ADAM", "ADAM_EMA", "EMA"):
        assert int(re.search(rf"#define P3D_OPTIM_{name} (\d+)", hdr).group(1)) == getattr(lib, f"P3D_OPTIM_{name}")
    assert lib.P3D_ABI_VERSION == 9 and L.p3d_abi_version() == 9
    assert "k_adam_ema" in open(os.path.join(B.CSRC, "p3d_optim.hip")).read()  # the kernel's name is part of what profiles record


def test_optim_struct_layouts(P):
    lib = P._lib
    L = lib.lib()  # (check_struct_layouts has compared the four mirrors)
    buf = (C.c_size_t * 32)()
    sizes = {}
    for which, cls in lib.OPTIM_STRUCT_MIRRORS.items():
        n = L.p3d_optim_struct_layout(which, buf, 32)
        assert n == 1 + len(cls._fields_) and list(buf[:n]) == [C.sizeof(cls)] + [getattr(cls, f).offset for f, _ in cls._fields_]
        sizes[cls.__name__] = buf[0]
    assert sizes == {"OptimTensor": 48, "OptimStep": 24, "OptimChunk": 16, "OptimArgs": 80}
    assert P.ops._OPTIM_STEP_DTYPE.itemsize == 24 and [P.ops._OPTIM_STEP_DTYPE.fields[f][1] for f, _ in lib.OptimStep._fields_] == \
        [getattr(lib.OptimStep, f).offset for f, _ in lib.OptimStep._fields_]
    assert L.p3d_optim_struct_layout(4, buf, 32) == -2 and L.p3d_optim_struct_layout(0, buf, 3) == -2 and L.p3d_optim_struct_layout(0, None, 32) == -1

    class Wrong(C.Structure):
        _fields_ = [("grad", C.c_void_p), ("step_size", C.c_float), ("bc2_sqrt", C.c_float), ("ema_w", C.c_double), ("grad_aligned16", C.c_int32)]
    saved = dict(lib.OPTIM_STRUCT_MIRRORS)
    try:
        lib.OPTIM_STRUCT_MIRRORS[1] = Wrong
        with pytest.raises(RuntimeError, match="Wrong"):
            lib.check_struct_layouts(L)
    finally:
        lib.OPTIM_STRUCT_MIRRORS.clear()
        lib.OPTIM_STRUCT_MIRRORS.update(saved)


def test_optim_argument_errors_without_gpu(P):
    lib = P._lib
    L = lib.lib()
    p = 256  # never dereferenced: the checks come first

    def step(**kw):
        a = dict(tensors=p, steps=p, chunks=p, n_chunks=3, n_tensors=2, mode=lib.P3D_OPTIM_ADAM, sanitize=1, grad_scale=1.0, eps=1e-8, beta1=0.0, beta2=0.99)
        a.update(kw)
        return L.p3d_optim_step_f32(C.byref(lib.OptimArgs(**a)), None)
    assert L.p3d_optim_step_f32(None, None) == -1
    assert step(tensors=None) == -1 and step(steps=None) == -1 and step(chunks=None) == -1
    assert step(n_tensors=0) == -1 and step(n_tensors=-1) == -1 and step(n_chunks=0) == -1 and step(n_chunks=-5) == -1
    assert step(mode=0) == -2 and step(mode=4) == -2 and step(n_chunks=1 << 31) == -2
    assert step(beta1=1.0) == -2 and step(beta2=-0.1) == -2 and step(beta2=float("nan")) == -2 and step(eps=-1.0) == -2

    nm = (C.c_int64 * 3)(1, 0, OC.CHUNK + 1)
    plan = (lib.OptimChunk * 3)()
    assert L.p3d_optim_plan(None, 3, None, 0) == -1 and L.p3d_optim_plan(nm, 0, None, 0) == -1 and L.p3d_optim_plan(nm, -2, None, 0) == -1
    assert L.p3d_optim_plan((C.c_int64 * 2)(4, -1), 2, None, 0) == -1
    assert L.p3d_optim_plan((C.c_int64 * 1)((1 << 31) * OC.CHUNK), 1, None, 0) == -2
    assert L.p3d_optim_plan((C.c_int64 * 2)(((1 << 31) - 1) * OC.CHUNK, 1), 2, None, 0) == -2
    assert L.p3d_optim_plan(nm, 3, None, 0) == 3 and L.p3d_optim_plan(nm, 3, plan, 2) == -3 and L.p3d_optim_plan(nm, 3, plan, 3) == 3
    assert [(c.tensor, c.offset, c.count) for c in plan] == [(0, 0, 1), (2, 0, OC.CHUNK), (2, OC.CHUNK, 1)]
    assert L.p3d_optim_aligned16(None, 4) == 0 and L.p3d_optim_aligned16((C.c_void_p * 2)(32, 48), 0) == 0
    assert L.p3d_optim_aligned16((C.c_void_p * 4)(32, 48, None, 64), 4) == 1 and L.p3d_optim_aligned16((C.c_void_p * 4)(32, 52, None, 64), 4) == 0


# ---- the chunk plan, compiled without a device ---------------------------------------------------------------------------------------------
def test_chunk_plan_host_program(P, tmp_path):
    exe = compile_host(tmp_path, "optim_plan_host.cpp")
    r = subprocess.run([exe] + [str(n) for n in OC.NUMELS], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    chunks = [tuple(int(x) for x in l.split()[1:]) for l in lines if l.startswith("chunk")]
    assert int(lines[0].split()[1]) == len(chunks)
    covered = [torch.zeros(n, dtype=torch.int32) for n in OC.NUMELS]
    for t, off, count in chunks:
        assert 1 <= count <= OC.CHUNK and off % OC.CHUNK == 0 and off + count <= OC.NUMELS[t], "no chunk crosses a tensor"
        covered[t][off:off + count] += 1
    assert all(bool((c == 1).all()) for c in covered), "every element exactly once"
    assert OC.NUMELS.index(0) not in {t for t, _, _ in chunks}, "the zero-numel tensor gets no chunk"
    assert len(chunks) == sum(-(-n // OC.CHUNK) for n in OC.NUMELS) == 17
    # the library's export is the same function
    L = P._lib.lib()
    nm = (C.c_int64 * len(OC.NUMELS))(*OC.NUMELS)
    plan = (P._lib.OptimChunk * len(chunks))()
    assert L.p3d_optim_plan(nm, len(OC.NUMELS), plan, len(chunks)) == len(chunks)
    assert [(c.tensor, c.offset, c.count) for c in plan] == chunks
    # the 16-byte flag: only when every pointer passed is aligned; a pointer the mode does not use (NULL) does not count
    flags = {l.split(" = ")[0][len("aligned "):]: int(l.split(" = ")[1]) for l in lines if l.startswith("aligned")}
    assert flags == {"0 16 32 48": 1, "0 16 32 52": 0, "4 16 32 48": 0, "0 8 32 48": 0, "0 16 33 48": 0, "0 16 -1 -1": 1, "0 12 -1 -1": 0, "none": 0}
    # errors come back as codes
    r = subprocess.run([exe, "5", "-1"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.splitlines()[0] == "count -1"


# ---- the host logic on the stand-in of the launch ------------------------------------------------------------------------------------------
NUMELS = [1, 5, 257, 0, OC.CHUNK + 1]


def _pair(P, betas, lr=OC.LR, seed=3, groups=None):
    """Our Adam on float32 parameters and torch.optim.Adam on float64 copies, from the same start."""
    ps = [torch.nn.Parameter(t) for t in OC.make_params(NUMELS, seed)]
    qs = [torch.nn.Parameter(p.detach().double()) for p in ps]
    if groups is None:
        mk = lambda cls, xs: cls(xs, lr=lr, betas=betas, eps=OC.EPS)
    else:
        mk = lambda cls, xs: cls([dict(params=xs[:2], lr=groups[0]), dict(params=xs[2:], lr=groups[1])], lr=lr, betas=betas, eps=OC.EPS)
    return ps, qs, mk(P.optim.Adam, ps), mk(torch.optim.Adam, qs)


def _set_grads(ps, qs, step, skip=()):
    for i, (p, q) in enumerate(zip(ps, qs)):
        if i in skip:
            p.grad = q.grad = None
        else:
            p.grad = OC.make_grad(p.numel(), 100 * step + i)
            q.grad = p.grad.double()


def _compare(ps, qs, ours, theirs, before, what):
    """The gate on p, m, v of every stepped parameter; `before`: the reference's exp_avg before its step (for the absolute sums)."""
    bad = []
    for i, (p, q) in enumerate(zip(ps, qs)):
        if q not in theirs.state or q.grad is None or p.numel() == 0:
            continue
        so, st = ours.state[p], theirs.state[q]
        group = next(g for g in theirs.param_groups if any(x is q for x in g["params"]))
        (b1, b2), lr = group["betas"], group["lr"]
        assert float(so["step"]) == float(st["step"]), f"{what}: step count of parameter {i}"
        step_size, bc2 = OC.bias_corrections(lr, b1, b2, float(st["step"]))
        m_abs = (b1 * before[i]).abs() + ((1 - b1) * q.grad).abs()
        denom = st["exp_avg_sq"].sqrt() / bc2 + OC.EPS
        bad += OC.gate(f"{what} p[{i}]", p.detach(), q.detach(), q.detach().abs() + step_size * m_abs / denom, verbose=False)
        bad += OC.gate(f"{what} m[{i}]", so["exp_avg"], st["exp_avg"], m_abs, verbose=False)
        bad += OC.gate(f"{what} v[{i}]", so["exp_avg_sq"], st["exp_avg_sq"], st["exp_avg_sq"], verbose=False)
    return bad


def _sync(ps, qs, ours, theirs):
    """The float64 reference takes over OUR binary32 state before a step (the step counts stay its own), so that every step is compared
    from the same start.  Left free-running, the two drift apart by the sum of the steps' rounding errors, each a few units of an UPDATE
    (2e-3), while the gate of p is in units of |p| + one update: an element with |p| < 1e-3 — there are some among 4097 normal draws —
    leaves it after a few steps whoever computes them in binary32."""
    with torch.no_grad():
        for p, q in zip(ps, qs):
            q.copy_(p)
            if q in theirs.state and p in ours.state:
                for k in ("exp_avg", "exp_avg_sq"):
                    theirs.state[q][k].copy_(ours.state[p][k])


def _before(qs, theirs):
    return [theirs.state[q]["exp_avg"].clone() if q in theirs.state and "exp_avg" in theirs.state[q] else torch.zeros_like(q) for q in qs]


@pytest.mark.parametrize("betas", OC.BETAS)
def test_five_steps_against_torch_adam_with_skipped_parameters(P, monkeypatch, betas):
    """Parameter 1 has no gradient in steps 2 and 4: its value, moments and step count stay exactly as they are, as torch keeps them,
    and its later bias corrections use its own count (3 after five steps)."""
    OC.install_ops(monkeypatch, P.ops)
    ps, qs, ours, theirs = _pair(P, betas)
    for step in range(1, 6):
        skip = (1,) if step in (2, 4) else ()
        _sync(ps, qs, ours, theirs)
        _set_grads(ps, qs, step, skip)
        before = _before(qs, theirs)
        frozen = [t.clone() for t in (ps[1].detach(), ours.state[ps[1]]["exp_avg"], ours.state[ps[1]]["exp_avg_sq"])] if skip else None
        ours.step()
        theirs.step()
        if skip:
            st = ours.state[ps[1]]
            assert all(torch.equal(a, b) for a, b in zip(frozen, (ps[1].detach(), st["exp_avg"], st["exp_avg_sq"])))
        assert _compare(ps, qs, ours, theirs, before, f"step {step}") == []
    assert float(ours.state[ps[1]]["step"]) == float(theirs.state[qs[1]]["step"]) == 3 and float(ours.state[ps[0]]["step"]) == 5
    assert set(ours.state[ps[0]]) == {"step", "exp_avg", "exp_avg_sq"} and ours.state[ps[0]]["step"].dtype == torch.float32
    if betas[0] == 0:
        assert torch.equal(ours.state[ps[2]]["exp_avg"], ps[2].grad), "beta1 == 0: m is the gradient, bit for bit"


def test_state_dict_exchange_with_torch_adam(P, monkeypatch):
    OC.install_ops(monkeypatch, P.ops)
    betas = (0.9, 0.999)
    # ours -> torch
    ps, qs, ours, theirs = _pair(P, betas)
    for step in (1, 2):
        _set_grads(ps, qs, step)
        ours.step()
    with torch.no_grad():
        for p, q in zip(ps, qs):
            q.copy_(p)
    theirs.load_state_dict(copy.deepcopy(ours.state_dict()))  # (a copy, as a saved file is: load_state_dict keeps the 'step' tensors it is given)
    plain = torch.optim.Adam([torch.nn.Parameter(p.detach().clone()) for p in ps], lr=OC.LR, betas=betas, eps=OC.EPS)
    plain.load_state_dict(copy.deepcopy(ours.state_dict()))  # float32 torch.optim.Adam takes it too, and steps
    for x, p in zip(plain.param_groups[0]["params"], ps):
        x.grad = OC.make_grad(p.numel(), 300)
    plain.step()
    _set_grads(ps, qs, 3)
    before = _before(qs, theirs)
    ours.step()
    theirs.step()
    assert _compare(ps, qs, ours, theirs, before, "ours -> torch") == []
    # torch -> ours
    ps, qs, ours, theirs = _pair(P, betas, seed=4)
    src = torch.optim.Adam([torch.nn.Parameter(p.detach().clone()) for p in ps], lr=OC.LR, betas=betas, eps=OC.EPS)
    for step in (1, 2):
        for x, p in zip(src.param_groups[0]["params"], ps):
            x.grad = OC.make_grad(p.numel(), 100 * step)
        src.step()
    with torch.no_grad():
        for x, p, q in zip(src.param_groups[0]["params"], ps, qs):
            p.copy_(x)
            q.copy_(x)
    ours.load_state_dict(copy.deepcopy(src.state_dict()))
    theirs.load_state_dict(copy.deepcopy(src.state_dict()))
    assert float(ours.state[ps[2]]["step"]) == 2
    _set_grads(ps, qs, 3)
    before = _before(qs, theirs)
    ours.step()
    theirs.step()
    assert _compare(ps, qs, ours, theirs, before, "torch -> ours") == []
    assert float(ours.state[ps[2]]["step"]) == 3


def test_param_groups_and_edited_lr_and_betas(P, monkeypatch):
    OC.install_ops(monkeypatch, P.ops)
    ps, qs, ours, theirs = _pair(P, (0.0, 0.99), groups=(0.002, 0.0005))
    for step in range(1, 5):
        if step == 2:
            for opt in (ours, theirs):
                opt.param_groups[0]["lr"] = 0.01
        if step == 3:
            for opt in (ours, theirs):
                opt.param_groups[1]["betas"] = (0.5, 0.9)
        _sync(ps, qs, ours, theirs)
        _set_grads(ps, qs, step)
        before = _before(qs, theirs)
        moved = [p.detach().clone() for p in ps]
        ours.step()
        theirs.step()
        assert _compare(ps, qs, ours, theirs, before, f"step {step}") == []
        if step == 2:  # the gate alone would pass an lr that was not read: the displacement shows it
            d = lambda i: float((ps[i].detach() - moved[i]).abs().max())
            assert d(1) > 5 * d(2), "group 0 steps with lr 0.01, group 1 with 0.0005"


def test_step_count_follows_the_state_tensor(P, monkeypatch):
    """The optimiser keeps a host copy of each step count; state['step'] stays the truth: a count edited in place, or replaced by
    load_state_dict, is the one the next bias correction uses."""
    OC.install_ops(monkeypatch, P.ops)
    ps, qs, ours, theirs = _pair(P, (0.9, 0.999))
    for step in (1, 2):
        _set_grads(ps, qs, step)
        ours.step()
        theirs.step()
    for opt, xs in ((ours, ps), (theirs, qs)):
        opt.state[xs[2]]["step"].fill_(10.0)
    _sync(ps, qs, ours, theirs)
    _set_grads(ps, qs, 3)
    before = _before(qs, theirs)
    ours.step()
    theirs.step()
    assert float(ours.state[ps[2]]["step"]) == 11 and float(ours.state[ps[1]]["step"]) == 3
    assert _compare(ps, qs, ours, theirs, before, "edited count") == []


def test_unsupported_options_raise(P, monkeypatch):
    A = P.optim.Adam
    cpu = [torch.nn.Parameter(torch.zeros(4))]
    with pytest.raises(ValueError, match="CUDA/ROCm"):
        A(cpu, lr=0.002)  # without the stand-in a CPU parameter is refused: there is no fallback
    with pytest.raises(RuntimeError, match="CUDA/ROCm"):
        P.ops.adam_ema_step(cpu, [torch.zeros(4)], [torch.zeros(4)], [torch.zeros(4)], [1.0], [1.0])
    OC.install_ops(monkeypatch, P.ops)
    A(cpu, lr=0.002)
    for kw in (dict(weight_decay=0.01), dict(amsgrad=True), dict(maximize=True), dict(capturable=True), dict(differentiable=True), dict(lr=torch.tensor(0.002)),
               dict(betas=(1.0, 0.99)), dict(lr=-1.0)):
        with pytest.raises(ValueError):
            A(cpu, **kw)
    with pytest.raises(ValueError, match="float32"):
        A([torch.nn.Parameter(torch.zeros(4, dtype=torch.float64))])
    with pytest.raises(ValueError, match="contiguous"):
        A([torch.nn.Parameter(torch.zeros(4, 4).t()[:, :2])])
    opt = A(cpu, lr=0.002)
    cpu[0].grad = torch.zeros(4)
    opt.param_groups[0]["amsgrad"] = True  # (as a loaded state_dict could bring it)
    with pytest.raises(ValueError, match="amsgrad"):
        opt.step()
    opt.param_groups[0]["amsgrad"] = False
    with pytest.raises(ValueError, match="flat"):
        opt.step(flat=torch.zeros(5))
    with pytest.raises(ValueError, match="ema"):
        opt.step(ema=([], 0.5))
    with pytest.raises(RuntimeError, match="ema_weights"):
        opt.step(ema=([torch.zeros(4)], 1.5))
    assert float(opt.state[cpu[0]]["step"]) == 0, "a step that raised did not count"
    opt.step()
    assert float(opt.state[cpu[0]]["step"]) == 1


def test_versions_move_by_the_wrappers_doing(P, monkeypatch):
    """The stand-in writes through numpy views, which no version counter sees — like the kernel's raw pointers.  What moves is what
    ops.adam_ema_step bumps: p, m, v of the stepped tensors and every EMA target; nothing of a skipped tensor."""
    OC.install_ops(monkeypatch, P.ops)
    ps = [torch.nn.Parameter(t) for t in OC.make_params([5, 7, 3], 1)]
    es = [p.detach().clone() for p in ps]
    opt = P.optim.Adam(ps, lr=0.002, betas=(0.0, 0.99))
    for p in ps:
        p.grad = torch.ones_like(p)
    opt.step()
    ps[0].grad, ps[1].grad, ps[2].grad = 2 * torch.ones_like(ps[0]), None, 3 * torch.ones_like(ps[2])
    tensors = lambda: [ps[i] for i in range(3)] + [opt.state[p][k] for p in ps for k in ("exp_avg", "exp_avg_sq")] + es
    v0, old = [t._version for t in tensors()], [t.detach().clone() for t in tensors()]
    opt.step(ema=(es, 0.5))
    v1 = [t._version for t in tensors()]
    moved = [b > a for a, b in zip(v0, v1)]
    assert moved == [True, False, True] + [True, True, False, False, True, True] + [True, True, True]
    changed = [not torch.equal(a, b.detach()) for a, b in zip(old, tensors())]
    assert changed == moved, "the stand-in did write what the wrapper says was written"
    # update_ema: parameters and float buffers through the launch, everything it wrote bumped
    G, G_ema = _toy(1), _toy(2)
    v0 = [t._version for t in list(G_ema.parameters()) + list(G_ema.buffers())]
    P.optim.update_ema(G_ema, G, 0.5)
    assert all(t._version > a for t, a in zip(list(G_ema.parameters()) + list(G_ema.buffers()), v0))


class _Toy(torch.nn.Module):
    def __init__(self, seed):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.a = torch.nn.Parameter(torch.randn(3, 5, generator=g))
        self.b = torch.nn.Parameter(torch.randn(1, generator=g))
        self.register_buffer("avg", torch.randn(7, generator=g))
        self.register_buffer("count", torch.tensor([seed], dtype=torch.int64))
        self.neural_rendering_resolution = 64 + seed
        self.rendering_kwargs = {"seed": seed}


def _toy(seed):
    return _Toy(seed)


def test_update_ema_against_the_reference_loop(P, monkeypatch):
    OC.install_ops(monkeypatch, P.ops)
    for beta in (0.0, 0.3, 0.99778, 1.0):
        G, G_ema = _toy(1), _toy(2)
        ref = copy.deepcopy(G_ema)
        OC.reference_update_ema(ref, G, beta)
        P.optim.update_ema(G_ema, G, beta)
        for (n, a), b in zip(G_ema.named_parameters(), ref.parameters()):
            e = OC.ema_f64(dict(G.named_parameters())[n].detach(), dict(_toy(2).named_parameters())[n].detach(), beta)
            assert OC.gate(f"ema {n} w={beta}", a.detach(), e["e"], e["e_abs"], verbose=False) == []
            assert float((a.detach() - b.detach()).abs().max()) <= 2 ** -22 * float(e["e_abs"].max())
        assert torch.equal(G_ema.avg, G.avg) and torch.equal(G_ema.count, G.count) and G_ema.count.dtype == torch.int64
        assert G_ema.neural_rendering_resolution == 65 and G_ema.rendering_kwargs == {"seed": 1} and G_ema.rendering_kwargs is not G.rendering_kwargs


# ---- phase_step: / num_gpus comes before nan_to_num --------------------------------------------------------------------------------------
RANK_SCRIPT = r'''
import json, os, sys
for p in (%r, %r):
    sys.path.insert(0, p)
import torch, torch.distributed as dist
import panic3d_amd as P
import optim_cases as OC
P.ops._adam_ema_impl, P.ops._optim_is_device = OC.adam_ema_impl_numpy, (lambda t: True)   # the stand-in of the launch
dist.init_process_group("gloo")
rank = dist.get_rank()
mk = lambda: torch.nn.ParameterList([torch.nn.Parameter(t) for t in OC.make_params([6, 300, 0, 9], 11)])
mod, ref = mk(), mk()
special = [float("nan"), float("inf"), -float("inf"), 3e7, -3e7, 1.0] if rank == 0 else [1.0, 2.0, 3.0, 1e7, 4.0, float("nan")]
for i in (0, 1, 3):                      # parameter 2 is empty; every rank has other gradients
    g = OC.make_grad(mod[i].numel(), 50 + 10 * rank + i)
    if i == 0:
        g = torch.tensor(special)
    mod[i].grad, ref[i].grad = g.clone(), g.clone()
kept = mod[0].grad.clone()
opt = P.optim.Adam(mod.parameters(), lr=0.002, betas=(0.0, 0.99))
P.optim.phase_step(mod, opt, num_gpus=2)
ropt = torch.optim.Adam(ref.parameters(), lr=0.002, betas=(0.0, 0.99), eps=1e-8)
OC.reference_phase_step(list(ref.parameters()), ropt, 2, all_reduce=dist.all_reduce)
out = {"world": dist.get_world_size(), "bad": [], "m_equal": True}
for i in (0, 1, 3):
    clean = ref[i].grad                 # the reference leaves the cleaned gradient here
    out["m_equal"] &= bool(torch.equal(opt.state[mod[i]]["exp_avg"], clean))
    r = OC.step_f64(mk()[i].detach(), torch.zeros_like(clean), torch.zeros_like(clean), clean, 0.002, 0.0, 0.99, 1e-8, 1)
    out["bad"] += OC.gate("p[%%d]" %% i, mod[i].detach(), r["p"], r["p_abs"], verbose=False)
    out["bad"] += OC.gate("torch p[%%d]" %% i, ref[i].detach(), r["p"], r["p_abs"], verbose=False)
    out["bad"] += OC.gate("v[%%d]" %% i, opt.state[mod[i]]["exp_avg_sq"], r["v"], r["v_abs"], verbose=False)
out["clean0"] = ref[0].grad.tolist()
out["grad_kept"] = bool(torch.equal(torch.nan_to_num(mod[0].grad, nan=-7.0), torch.nan_to_num(kept, nan=-7.0)))
out["finite"] = all(bool(torch.isfinite(p).all()) for p in mod)
dist.barrier()
dist.destroy_process_group()
if rank == 0:
    print(json.dumps(out))
'''


def test_phase_step_divides_before_it_cleans_on_gloo(tmp_path):
    script = tmp_path / "rank.py"
    script.write_text(RANK_SCRIPT % (ROOT, os.path.join(ROOT, "tests")))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", "29581",
           str(script)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert out["world"] == 2 and out["bad"] == [] and out["finite"]
    assert out["m_equal"], "beta1 == 0: exp_avg is the cleaned gradient of the reference's lines, bit for bit"
    # nan + 1 -> nan -> 0;  inf + 2 -> inf / 2 -> 1e5 (cleaning first would give 5e4);  (3e7 + 1e7) / 2 = 2e7 passes unchanged;  1 + nan -> 0
    assert out["clean0"] == [0.0, 1e5, -1e5, 2e7, (-3e7 + 4.0) / 2, 0.0]
    assert out["grad_kept"], "param.grad is not overwritten (the documented difference from the reference)"


# ---- the helpers ----------------------------------------------------------------------------------------------------------------------------
def test_lazy_regularization(P):
    kw = dict(lr=0.002, betas=[0, 0.99], eps=1e-8)
    for interval in (4, 16):
        c = interval / (interval + 1)
        out = P.optim.lazy_regularization(kw, interval)
        assert out == dict(lr=0.002 * c, betas=[0 ** c, 0.99 ** c], eps=1e-8) and out is not kw
        assert kw == dict(lr=0.002, betas=[0, 0.99], eps=1e-8), "the input is not mutated"
    assert P.optim.lazy_regularization(kw, 16)["betas"][1] == OC.BETAS[1][1]
    out = P.optim.lazy_regularization(kw, None)
    assert out == kw and out is not kw


def test_ema_beta(P):
    f = P.optim.ema_beta
    assert f(0, 32, 10, 0.05) == 0.0                                   # ema_nimg = 0 -> 0.5 ** (32 / 1e-8) underflows to 0
    assert f(20000, 32, 10, 0.05) == 0.5 ** (32 / 1000.0)              # ramp-up: min(10000, 20000 * 0.05)
    assert f(400000, 32, 10, 0.05) == 0.5 ** (32 / 10000.0)            # after it
    assert f(0, 32, 10, None) == 0.5 ** (32 / 10000.0) and abs(f(0, 32, 10) - 0.99778) < 1e-5
