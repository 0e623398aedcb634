"""The second half of a training iteration (training_loop_v0.py:363-392) on one HIP launch per step (ops.adam_ema_step,
include/p3d_optim.h):

  Adam                  a torch.optim.Optimizer with torch.optim.Adam's state and state_dict; one launch for all its tensors
  phase_step            "Update weights" of a phase (:364-375): gather, all-reduce, / num_gpus, nan_to_num, opt.step()
  update_ema            "Update G_ema" (:382-392): the lerp of every parameter and the copy of every buffer in one launch
  ema_beta              the EMA weight of an iteration (:383-386)
  lazy_regularization   the rescaled lr / betas of a lazily regularised optimiser (:226-229)

Why the step lives in this package: every parameter-derived cache here (memo.py) is keyed on a tensor's `_version`, and the kernel
writes through raw pointers.  ops.adam_ema_step bumps the version of everything it wrote, so no caller needs `clear_memo()` after a
step.  Not here: the R1 penalty (loss.py's Dreg / Dboth with DualDiscriminator.set_r1_grad()), LPIPS, the augment pipe's module (its operator is ops.augment_apply), the data loader and the loop itself.
"""
import math
import weakref

import torch

from . import ops

__all__ = ["Adam", "phase_step", "update_ema", "ema_beta", "lazy_regularization", "SANITIZE"]

SANITIZE = (0.0, 1e5, -1e5)  # training_loop_v0.py:371: misc.nan_to_num(flat, nan=0, posinf=1e5, neginf=-1e5)


class Adam(torch.optim.Optimizer):
    """torch.optim.Adam's update (its non-capturable form: the bias corrections are host doubles from each tensor's own step count)
    for float32 device parameters, all tensors of a param group in one launch.  Per-parameter state is torch's:
    {'step' (a float32 CPU scalar tensor), 'exp_avg', 'exp_avg_sq'}, created when a parameter first has a gradient; the param groups
    carry torch.optim.Adam's keys, so state_dict() loads into torch.optim.Adam and torch's loads here.  A parameter whose `.grad` is
    None in a step is skipped: its value, moments and step count stay as they are.  `lr` and `betas` are read from the group at
    every step.  Not supported (ValueError at construction, or at the step that meets them in a loaded state): weight_decay != 0,
    amsgrad, maximize, capturable, differentiable, a tensor lr, parameters that are not float32 device tensors."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, foreach=None, maximize=False,
                 capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False):
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize, foreach=foreach,
                        capturable=capturable, differentiable=differentiable, fused=fused, decoupled_weight_decay=decoupled_weight_decay)
        super().__init__(params, defaults)
        for group in self.param_groups:
            self._check_group(group)
            for i, p in enumerate(group["params"]):
                try:
                    ops._optim_chk(p, f"parameter {i}")
                except RuntimeError as e:
                    raise ValueError(str(e)) from None
        self._tables = {}  # (index of the param group, with EMA) -> the uploaded table of ops.adam_ema_step
        self._steps = {}   # parameter -> what step() last left in state['step']: a host copy of the count, dropped when the tensor changed

    @staticmethod
    def _check_group(group):
        lr, (beta1, beta2), eps = group["lr"], group["betas"], group["eps"]
        if isinstance(lr, torch.Tensor) or isinstance(beta1, torch.Tensor) or isinstance(beta2, torch.Tensor):
            raise ValueError("panic3d_amd.optim.Adam: lr and betas must be Python numbers, not tensors")
        if not lr >= 0.0 or not eps >= 0.0 or not 0.0 <= beta1 < 1.0 or not 0.0 <= beta2 < 1.0:
            raise ValueError(f"panic3d_amd.optim.Adam: invalid lr / betas / eps: {lr}, {(beta1, beta2)}, {eps}")
        for name in ("amsgrad", "maximize", "capturable", "differentiable"):
            if group.get(name):
                raise ValueError(f"panic3d_amd.optim.Adam: {name} is not supported")
        if group.get("weight_decay", 0) != 0:
            raise ValueError("panic3d_amd.optim.Adam: weight_decay != 0 is not supported")

    @torch.no_grad()
    def step(self, closure=None, *, grad_scale=1.0, sanitize=None, flat=None, ema=None):
        """One update.  The gradient of a parameter is `p.grad`, or with `flat` (one flat float32 vector, already reduced) the next
        p.numel() elements of it, for the parameters with `p.grad is not None and p.numel() > 0` in the optimiser's own order; the
        segments are read in place.  The kernel computes g = grad * grad_scale FIRST and then, with sanitize = (nan, posinf, neginf),
        cleans g as torch.nan_to_num does.  ema = (ema_params, beta): one tensor per parameter of the optimiser, in its order;
        ema <- lerp(p, ema, beta) on the new p rides in the same launch, for the parameters without a gradient too."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        ema_params, ema_w = (list(ema[0]), float(ema[1])) if ema is not None else (None, None)
        n_all = sum(len(g["params"]) for g in self.param_groups)
        if ema_params is not None and len(ema_params) != n_all:
            raise ValueError(f"panic3d_amd.optim.Adam.step: ema names {len(ema_params)} tensors for {n_all} parameters")
        if flat is not None:
            if not isinstance(flat, torch.Tensor) or flat.ndim != 1 or not flat.is_contiguous():
                raise ValueError("panic3d_amd.optim.Adam.step: flat must be one contiguous 1-D tensor")
            want = sum(p.numel() for g in self.param_groups for p in g["params"] if p.grad is not None)
            if want != flat.numel():
                raise ValueError(f"panic3d_amd.optim.Adam.step: flat has {flat.numel()} elements, the parameters with a gradient {want}")
        at, first = 0, 0
        for gi, group in enumerate(self.param_groups):
            self._check_group(group)
            params = group["params"]
            lr, (beta1, beta2), eps = group["lr"], group["betas"], group["eps"]
            grads, ms, vs, step_sizes, bc2_sqrts, bumped, corr = [], [], [], [], [], [], {}
            for p in params:
                g = p.grad
                if g is None:
                    state = self.state.get(p)
                    grads.append(None), step_sizes.append(0.0), bc2_sqrts.append(1.0)
                    ms.append(state["exp_avg"] if state else None), vs.append(state["exp_avg_sq"] if state else None)
                    continue
                if g.is_sparse:
                    raise RuntimeError("panic3d_amd.optim.Adam does not support sparse gradients")
                state = self.state[p]
                if len(state) == 0:  # torch.optim.Adam._init_group
                    state["step"] = torch.tensor(0.0, dtype=torch.float32)
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                t = state["step"]
                seen = self._steps.get(p)  # (the step tensor, its value, its version) as this optimiser left them
                step = seen[1] if seen is not None and seen[0] is t and seen[2] == t._version else float(t)
                step += 1.0
                bumped.append((p, t, step))
                if flat is None or p.numel() == 0:
                    grads.append(g)
                else:
                    grads.append(flat[at:at + p.numel()])
                    at += p.numel()
                ms.append(state["exp_avg"]), vs.append(state["exp_avg_sq"])
                c = corr.get(step)
                if c is None:
                    c = corr[step] = (lr / (1.0 - beta1 ** step), math.sqrt(1.0 - beta2 ** step))
                step_sizes.append(c[0]), bc2_sqrts.append(c[1])
            emas = ema_params[first:first + len(params)] if ema_params is not None else None
            first += len(params)
            if not params or (emas is None and all(g is None for g in grads)):
                continue
            slot = (gi, emas is not None)  # (a table names the EMA targets: the plain and the fused form keep one each)
            self._tables[slot] = ops.adam_ema_step(params, grads, ms, vs, step_sizes, bc2_sqrts, beta1=beta1, beta2=beta2, eps=eps,
                                                   grad_scale=grad_scale, sanitize=sanitize, ema_params=emas,
                                                   ema_weights=[ema_w] * len(params) if emas is not None else None, table=self._tables.get(slot))
            if bumped:  # after the launch: state['step'] stays torch's tensor; one call adds to all of them
                torch._foreach_add_([t for _, t, _ in bumped], 1)
                for p, t, step in bumped:
                    self._steps[p] = (t, step, t._version)
        return loss


def phase_step(module, opt, num_gpus=1, ema=None, flat=None):
    """"Update weights" of one phase (training_loop_v0.py:364-375) for an `Adam` of this module over `module`'s parameters.

    One GPU: a single launch that reads every `param.grad` where it lies; nothing is concatenated.  num_gpus > 1 (or flat=True, which
    forces that path, with the all-reduce whenever a process group is up): torch.cat of the gradients ->
    torch.distributed.all_reduce -> one launch that reads the segments of the flat vector with grad_scale = 1 / num_gpus.

    The order is the reference's: the sum over the ranks, the division by num_gpus, THEN nan_to_num(nan=0, posinf=1e5,
    neginf=-1e5) — so a rank's NaN poisons the sum and is replaced after it, and a finite value passes however large.  The division is
    a multiplication by the binary32 1 / num_gpus: exact for a power of two.  The one observable difference: the reference
    overwrites `param.grad` with the cleaned values; here `param.grad` keeps what backward wrote and only the update sees the
    cleaned gradient.  ema: passed to `Adam.step`."""
    params = [p for p in module.parameters() if p.numel() > 0 and p.grad is not None]
    theirs = [p for g in opt.param_groups for p in g["params"] if p.grad is not None and p.numel() > 0]
    if {id(p) for p in params} != {id(p) for p in theirs}:
        raise ValueError("phase_step: the optimiser must hold exactly the module's parameters")
    if flat is None:
        flat = num_gpus > 1
    if not flat or not theirs:
        return opt.step(grad_scale=1.0 / num_gpus, sanitize=SANITIZE, ema=ema)
    vec = torch.cat([p.grad.flatten() for p in theirs])  # (the optimiser's order: the segments are consumed in it)
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        torch.distributed.all_reduce(vec)
    return opt.step(grad_scale=1.0 / num_gpus, sanitize=SANITIZE, flat=vec, ema=ema)


_EMA_TABLES = weakref.WeakKeyDictionary()  # G_ema -> the uploaded table of its update


@torch.no_grad()
def update_ema(G_ema, G, beta):
    """"Update G_ema" (training_loop_v0.py:387-392): p_ema <- p.lerp(p_ema, beta) for every parameter and b_ema <- b for every buffer, in
    one launch (a buffer rides with weight 0, which copies bit for bit); a buffer that is not a float32 device tensor is copied with
    copy_.  Then G_ema takes G's neural_rendering_resolution and a copy of its rendering_kwargs, where G has them."""
    src, dst, w = [], [], []
    for p_ema, p in zip(G_ema.parameters(), G.parameters()):
        src.append(p), dst.append(p_ema), w.append(float(beta))
    for b_ema, b in zip(G_ema.buffers(), G.buffers()):
        if b.dtype == torch.float32 and b_ema.dtype == torch.float32 and ops._optim_is_device(b) and b.is_contiguous() and b_ema.is_contiguous() \
                and b.shape == b_ema.shape:
            src.append(b), dst.append(b_ema), w.append(0.0)
        else:
            b_ema.copy_(b)
    if src:
        _EMA_TABLES[G_ema] = ops.adam_ema_step(src, ema_params=dst, ema_weights=w, table=_EMA_TABLES.get(G_ema))
    if hasattr(G, "neural_rendering_resolution"):
        G_ema.neural_rendering_resolution = G.neural_rendering_resolution
    if hasattr(G, "rendering_kwargs"):
        G_ema.rendering_kwargs = G.rendering_kwargs.copy()


def ema_beta(cur_nimg, batch_size, ema_kimg, ema_rampup=None):
    """The EMA weight of an iteration (training_loop_v0.py:383-386): 0.5 ** (batch_size / max(ema_nimg, 1e-8)), ema_nimg = ema_kimg * 1000,
    during ramp-up at most cur_nimg * ema_rampup.  0 at cur_nimg = 0 with a ramp-up."""
    ema_nimg = ema_kimg * 1000
    if ema_rampup is not None:
        ema_nimg = min(ema_nimg, cur_nimg * ema_rampup)
    return 0.5 ** (batch_size / max(ema_nimg, 1e-8))


def lazy_regularization(opt_kwargs, reg_interval):
    """The optimiser arguments of a lazily regularised network (training_loop_v0.py:226-229): lr * c and beta ** c with
    c = reg_interval / (reg_interval + 1).  Returns a new dict; reg_interval None returns a plain copy."""
    out = dict(opt_kwargs)
    if reg_interval is None:
        return out
    mb_ratio = reg_interval / (reg_interval + 1)
    out["lr"] = opt_kwargs["lr"] * mb_ratio
    out["betas"] = [beta ** mb_ratio for beta in opt_kwargs["betas"]]
    return out
