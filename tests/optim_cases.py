"""Cases of the optimiser step (panic3d_amd/optim.py, include/p3d_optim.h), shared by tests/test_optim_cpu.py and tests/test_hip_optim.py:
  * the float64 restatement of one step, written from the formulas of include/p3d_optim.h, with the absolute-value sums of the gate;
  * the gate: the project's 8 * 2^-24 gate (tests/loss_cases.py, K = 1);
  * a stand-in of ops._adam_ema_impl for the CPU tests: the kernel's formulas in numpy binary32, written THROUGH numpy views so that
    no version counter moves by its doing (what ops.adam_ema_step bumps is then visible);
  * the seeded inputs.
Not a test file."""
import math

import numpy as np
import torch

import loss_cases as LC

CHUNK = 4096  # P3D_OPTIM_CHUNK
NUMELS = [1, 3, 4, 5, 63, 64, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 7, 0]
BETAS = [(0.0, 0.99), (0.0, 0.99 ** (16 / 17)), (0.9, 0.999)]
LR, EPS = 0.002, 1e-8
SANITIZE = (0.0, 1e5, -1e5)
EMA_WEIGHTS = [0.0, 0.3, 0.5, 0.99778, 1.0]
f32 = lambda x: float(np.float32(x))


def make_grad(numel, seed):
    """randn x logspace(-6, 2), every 97th value exactly 0."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(numel, generator=g) * torch.logspace(-6, 2, numel)
    x[::97] = 0.0
    return x


def make_params(numels, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=g) for n in numels]


def bias_corrections(lr, beta1, beta2, step):
    """(step_size, bc2_sqrt) as the host computes them: doubles, from the tensor's own step count."""
    return lr / (1.0 - beta1 ** step), math.sqrt(1.0 - beta2 ** step)


def clean_f64(g, grad_scale, sanitize):
    """g * grad_scale in binary32 (one rounding), THEN nan_to_num; float64 out."""
    g = (g.float() * torch.tensor(grad_scale, dtype=torch.float32)).double()
    if sanitize is not None:
        g = torch.nan_to_num(g, nan=sanitize[0], posinf=sanitize[1], neginf=sanitize[2])
    return g


def step_f64(p0, m0, v0, grad, lr, beta1, beta2, eps, step, grad_scale=1.0, sanitize=None):
    """One Adam step of include/p3d_optim.h in float64 from the binary32 state; the scalars are the binary32 values the kernel is
    handed.  Returns p, m, v, the cleaned gradient g and the gate's absolute-value sums."""
    step_size, bc2_sqrt = (f32(x) for x in bias_corrections(lr, beta1, beta2, step))
    b1, c1, b2, c2, eps = f32(beta1), f32(1.0 - beta1), f32(beta2), f32(1.0 - beta2), f32(eps)
    p0, m0, v0 = p0.double(), m0.double(), v0.double()
    g = clean_f64(grad, grad_scale, sanitize)  # (the product by grad_scale is exact in float64 only for a power of two: the tests use 1 and 0.5)
    m1 = b1 * m0 + c1 * g
    v1 = b2 * v0 + (c2 * g) * g
    denom = v1.sqrt() / bc2_sqrt + eps
    p1 = p0 - step_size * (m1 / denom)
    m_abs = (b1 * m0).abs() + (c1 * g).abs()
    return dict(p=p1, m=m1, v=v1, g=g, p_abs=p1.abs() + step_size * m_abs / denom, m_abs=m_abs, v_abs=v1)


def ema_f64(p1, e0, w):
    """p + w (e - p) in float64, and the gate's sum |p1| + |e0|."""
    p1, e0 = p1.double(), e0.double()
    return dict(e=p1 + f32(w) * (e0 - p1), e_abs=p1.abs() + e0.abs())


def gate(name, ours, ref, absref, verbose=True):
    """The project's gate with K = 1: per value 8 * 2^-24 * absref (exact where absref == 0), and rel-L2 <= 1e-5."""
    return LC.gate(name, ours, ref, absref, 1, verbose=verbose)


# ---- the stand-in of the launch ---------------------------------------------------------------------------------------------------------
def _np(t):
    return t.detach().numpy().reshape(-1)  # shares the memory; a write through it moves no version counter


def adam_ema_impl_numpy(params, grads, exp_avgs, exp_avg_sqs, emas, step_sizes, bc2_sqrts, ema_weights, beta1, beta2, eps, grad_scale, sanitize, table,
                        key=None):
    """ops._adam_ema_impl on CPU tensors: the formulas of include/p3d_optim.h, every operation in numpy binary32."""
    F = np.float32
    adam, ema = grads is not None, emas is not None
    with np.errstate(all="ignore"):
        for i, p in enumerate(params):
            P = _np(p)
            if adam and grads[i] is not None:
                g = grads[i].detach().contiguous().numpy().reshape(-1).astype(F) * F(grad_scale)
                if sanitize is not None:
                    g = np.where(np.isnan(g), F(sanitize[0]), np.where(g == np.inf, F(sanitize[1]), np.where(g == -np.inf, F(sanitize[2]), g))).astype(F)
                M, V = _np(exp_avgs[i]), _np(exp_avg_sqs[i])
                M[:] = (F(beta1) * M + F(1.0 - beta1) * g) if F(beta1) != 0 else g
                V[:] = F(beta2) * V + (F(1.0 - beta2) * g) * g
                P[:] = P - F(step_sizes[i]) * (M / (np.sqrt(V) / F(bc2_sqrts[i]) + F(eps)))
            if ema:
                E, w = _np(emas[i]), F(ema_weights[i])
                d = E - P
                E[:] = P if w == 0 else E if w == 1 else (P + w * d) if w < 0.5 else (E - d * (F(1) - w))
    return None


def install_ops(monkeypatch, ops):
    """The launch on numpy, and CPU tensors accepted as 'device' tensors."""
    monkeypatch.setattr(ops, "_adam_ema_impl", adam_ema_impl_numpy)
    monkeypatch.setattr(ops, "_optim_is_device", lambda t: True)


# ---- the reference's lines, restated in torch ---------------------------------------------------------------------------------------------
def reference_phase_step(params, opt, num_gpus, all_reduce=None):
    """training_loop_v0.py:365-375 for `params` (those with numel > 0 and a gradient) and a torch.optim.Adam."""
    params = [p for p in params if p.numel() > 0 and p.grad is not None]
    if params:
        flat = torch.cat([p.grad.flatten() for p in params])
        if num_gpus > 1:
            if all_reduce is not None:
                all_reduce(flat)
            flat /= num_gpus
        torch.nan_to_num(flat, nan=0, posinf=1e5, neginf=-1e5, out=flat)
        for p, g in zip(params, flat.split([p.numel() for p in params])):
            p.grad = g.reshape(p.shape)
    opt.step()


def reference_update_ema(G_ema, G, beta):
    """training_loop_v0.py:387-390."""
    with torch.no_grad():
        for p_ema, p in zip(G_ema.parameters(), G.parameters()):
            p_ema.copy_(p.lerp(p_ema, beta))
        for b_ema, b in zip(G_ema.buffers(), G.buffers()):
            b_ema.copy_(b)
