"""Cases of the illustration-to-render module's training (panic3d_amd/rmline_train.py, include/p3d_rmline_grad.h): a restatement of the
reference's rmlineganA.Model (rmlineganA.py:57-298) with torch's own modules in any dtype (float64: the reference of every test),
seeded patches, the closed-form operators the kernels implement written with plain tensor ops (they double as CPU stand-ins of
panic3d_amd.ops.rmline_* and as the float64 references of the GPU tests), seedable faults, and the gates.

The reference's lines, restated (Lightning and kornia are absent, so the model itself cannot be imported):
  networks           :65-100   unpadded 3 x 3 convolutions; LeakyReLU(0.01) then BatchNorm2d after every one but the last; Tanh ends the
                               generator, nothing the discriminator
  forward            :108-143  cat(image (1 - mask), hull), replicate-padded by gen_depth
  loss               :174-208  torch.lerp, L1 mean, the discriminator on the centre crop (F.pad by (patch_size - S) // 2 < 0), BCE with
                               logits against real_label sm + sm / 2 (0.4 and 1.2 — sic)
  training_step      :209-233  step 0: index 0 of every pair, labels forced to 1; step 1: both indices flattened, true labels
"""
import torch

F = torch.nn.functional
SLOPE = 0.01

CONFIGS = {
    "real": dict(gen_depth=6, gen_width=32, dis_depth=4, dis_width=16, size=21, patch_size=9),
    "small": dict(gen_depth=2, gen_width=8, dis_depth=2, dis_width=4, size=9, patch_size=5),
    # the odd difference crops by (5 - 10) // 2 = -3: a 4 x 4 window, which leaves room for one discriminator layer
    "ragged": dict(gen_depth=2, gen_width=5, dis_depth=1, dis_width=7, size=10, patch_size=5),
}
FAULTS = set()  # names of seeded faults the stand-ins below honour (tests add and remove them)


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------
class RefModel(torch.nn.Module):
    def __init__(self, patch_size=9, gen_depth=6, gen_width=32, dis_depth=4, dis_width=16, size=21, label_smoothing=0.8, lambda_l1=1.0,
                 lambda_adv=1.0, lr_gen=0.001, lr_dis=0.001):
        super().__init__()
        assert patch_size + 2 * gen_depth <= size  # :63
        self.patch_size, self.gen_depth, self.label_smoothing = patch_size, gen_depth, label_smoothing
        self.lambda_l1, self.lambda_adv, self.lr_gen, self.lr_dis = lambda_l1, lambda_adv, lr_gen, lr_dis
        gen, w = [], gen_width
        for i in range(gen_depth):  # :65-82
            gen.append(torch.nn.Conv2d(4 if i == 0 else w, w if i != gen_depth - 1 else 3, 3, stride=1, padding=0))
            if i != gen_depth - 1:
                gen += [torch.nn.LeakyReLU(), torch.nn.BatchNorm2d(w)]
        gen.append(torch.nn.Tanh())
        self.generator = torch.nn.Sequential(*gen)
        dis, w = [], dis_width
        for i in range(dis_depth):  # :84-100
            dis.append(torch.nn.Conv2d(4 if i == 0 else w, w, 3, stride=1, padding=0))
            if i != dis_depth - 1:
                dis += [torch.nn.LeakyReLU(), torch.nn.BatchNorm2d(w)]
        self.discriminator = torch.nn.Sequential(*dis)

    def forward(self, x, pad=True):  # :108-143
        img = x["image"] * (1 - x["line_mask"])
        stackin = torch.cat([img, x["face_hull"]], dim=1)
        if pad:
            stackin = F.pad(stackin, (self.gen_depth,) * 4, mode="replicate")
        return {"image": self.generator(stackin), "line_mask": x["line_mask"], "face_hull": x["face_hull"]}

    def forward_discriminator(self, x):  # :145-172
        stackin = torch.cat([x["image"], x["face_hull"]], dim=1)
        stackin = F.pad(stackin, ((self.patch_size - x["image"].shape[-1]) // 2,) * 4, mode="replicate")
        return {"logits": self.discriminator(stackin).mean((1, 2, 3))}

    def loss(self, pred, gt):  # :174-208
        pred["image"] = torch.lerp(gt["image"], pred["image"], gt["line_mask"])
        loss_l1 = (pred["image"] - gt["image"]).abs().mean((1, 2, 3))
        outd = self.forward_discriminator(pred)
        sm = self.label_smoothing
        loss_adv = F.binary_cross_entropy_with_logits(outd["logits"], gt["real_label"] * sm + sm / 2, reduction="none")
        return {"loss": self.lambda_l1 * loss_l1 + self.lambda_adv * loss_adv, "loss_l1": loss_l1, "loss_adv": loss_adv}

    def training_step(self, batch, batch_idx, optimizer_idx):  # :209-233
        if optimizer_idx == 0:
            batch = {k: v[:, 0] for k, v in batch.items()}
            batch["real_label"] = torch.ones_like(batch["real_label"])
        else:
            batch = {k: v.reshape(-1, *v.shape[2:]) for k, v in batch.items()}
        loss = self.loss(self.forward(batch), batch)
        self.last = {k: v.detach().mean() for k, v in loss.items()}
        return loss["loss"].mean()

    def fit_step(self, batch, optimizers):
        """Lightning's automatic optimisation of one batch (toggle_optimizer, training_step, zero_grad, backward, step, untoggle)."""
        nets, out = (self.generator, self.discriminator), []
        for idx, opt in enumerate(optimizers):
            for p in nets[1 - idx].parameters():
                p.requires_grad_(False)
            loss = self.training_step(batch, 0, idx)
            opt.zero_grad()
            loss.backward()
            opt.step()
            for p in nets[1 - idx].parameters():
                p.requires_grad_(True)
            out.append(loss.detach())
        return out


def ref_like(model, dtype=torch.float64, device="cpu"):
    """The restatement holding `model`'s (an RMLineModel's) parameters and buffers, in dtype."""
    ref = RefModel(patch_size=model.patch_size, gen_depth=model.gen_depth, gen_width=model.gen_width, dis_depth=model.dis_depth,
                   dis_width=model.dis_width, size=model.size, label_smoothing=model.label_smoothing, lambda_l1=model.lambda_l1,
                   lambda_adv=model.lambda_adv)
    ref.load_state_dict({k: v.detach().cpu() for k, v in model.state_dict().items()})
    return ref.to(device=device, dtype=dtype).train()


def make_batch(cfg, B, seed=0, dtype=torch.float32, device="cpu"):
    """Seeded patches: images in [0, 1], a line mask of 0 / 1 with both values present, a hull, labels (0, 1).  Where the mask is 0 the
    lerped image IS the ground truth (|img - gt| = 0: the sign(0) = 0 case)."""
    g = torch.Generator().manual_seed(1000 + seed)
    S = cfg["size"]
    batch = {
        "image": torch.rand((B, 2, 3, S, S), generator=g),
        "line_mask": (torch.rand((B, 2, 1, S, S), generator=g) > 0.6).float(),
        "face_hull": (torch.rand((B, 2, 1, S, S), generator=g) > 0.8).float(),
        "real_label": torch.tensor([0.0, 1.0]).expand(B, 2).contiguous(),
    }
    return {k: v.to(device=device, dtype=dtype) for k, v in batch.items()}


def perturb(model, seed=0):
    """Make the batch norms' affine parameters non-trivial, so that every term of their backward is exercised."""
    g = torch.Generator().manual_seed(77 + seed)
    with torch.no_grad():
        for m in list(model.generator) + list(model.discriminator):
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.copy_(0.5 + torch.rand(m.weight.shape, generator=g))
                m.bias.copy_(torch.rand(m.bias.shape, generator=g) - 0.5)
    return model


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


# ---- the closed forms: what the kernels implement, with plain tensor ops in the dtype of their arguments ----------------------------------
def stack_input(image, mask, hull, pad):
    """The first layer's input, channel-last: cat(image (1 - mask), hull) replicate-padded (rmlineganA.py:117-130)."""
    x = image * (1 - mask) if mask is not None else image
    if hull is not None:
        x = torch.cat([x, hull], dim=1)
    if pad:
        x = F.pad(x, (pad,) * 4, mode="replicate")
    return x.permute(0, 2, 3, 1).contiguous()


def conv(x, wk, bias, act="none", slope=0.01, stack=None, pad=0, planar=False, lerp=None, plan=0, per_tap=False):
    x = stack_input(*stack, pad) if stack is not None else x
    Ho, Wo = x.shape[1] - 2, x.shape[2] - 2
    z = sum(x[:, t // 3:t // 3 + Ho, t % 3:t % 3 + Wo, :] @ wk[t] for t in range(9)) + bias
    z = F.leaky_relu(z, slope) if act == "leaky" else (torch.tanh(z) if act == "tanh" else z)
    return z.permute(0, 3, 1, 2).contiguous() if planar else z


def bn_stats(x, running_mean=None, running_var=None, counter=None, momentum=0.1):
    C = x.shape[-1]
    xf = x.reshape(-1, C)
    K = xf.shape[0]
    if K <= 1:
        raise ValueError("Expected more than 1 value per channel when training")
    mean = xf.mean(0)
    var = ((xf - mean) ** 2).mean(0)
    if running_mean is not None and not ("stale_running" in FAULTS and C == FAULTS_ARG.get("stale_running")):
        unbiased = var if "biased_running" in FAULTS else var * (K / (K - 1))
        with torch.no_grad():
            running_mean.mul_(1 - momentum).add_(momentum * mean.to(running_mean.dtype))
            running_var.mul_(1 - momentum).add_(momentum * unbiased.to(running_var.dtype))
            counter.add_(1)
    return mean, var


FAULTS_ARG = {}


def bn_fold(w, bias, bn=None):
    wk = w.permute(2, 3, 1, 0).reshape(9, w.shape[1], w.shape[0])
    if bn is None:
        return wk.contiguous(), bias.clone()
    gamma, beta, mean, var, eps = bn
    s = gamma / torch.sqrt(var + eps)
    sh = beta - mean * s
    return (wk * s.view(1, -1, 1)).contiguous(), bias + (wk * sh.view(1, -1, 1)).sum((0, 1))


def conv_dgrad(g, wk, a=None, c0=None, c1=None, slope=0.01, planar=False):
    N, Hg, Wg, Co = g.shape
    Ci = wk.shape[1]
    dx = torch.zeros((N, Hg + 2, Wg + 2, Ci), dtype=g.dtype, device=g.device)
    for t in range(9):
        tt = t if "taps_not_flipped" not in FAULTS else 8 - t
        dx[:, t // 3:t // 3 + Hg, t % 3:t % 3 + Wg, :] += g @ wk[tt].transpose(0, 1)
    if a is not None:
        if not slope > 0:
            raise ValueError("slope")
        if c0 is not None:
            dx = dx + c0 + (0 if "drop_c1" in FAULTS else c1 * a)
        dx = dx * torch.where(a > 0, torch.ones_like(a), torch.full_like(a, slope))
    return dx.permute(0, 3, 1, 2).contiguous() if planar else dx


def conv_wgrad(x, dz, stack=None, pad=0, force_slices=0, oihw=False):
    x = stack_input(*stack, pad) if stack is not None else x
    Ho, Wo = dz.shape[1], dz.shape[2]
    dw = torch.stack([torch.einsum("nyxi,nyxo->io", x[:, t // 3:t // 3 + Ho, t % 3:t % 3 + Wo, :], dz) for t in range(9)])
    if oihw:
        dw = dw.reshape(3, 3, dw.shape[1], dw.shape[2]).permute(3, 2, 0, 1).contiguous()
    return dw, dz.sum((0, 1, 2))


def bn_coef(dwk_f, db_f, w, gamma, beta, mean, var, eps, K, want_dw=True, want_affine=True):
    wk = w.permute(2, 3, 1, 0).reshape(9, w.shape[1], w.shape[0])
    r = 1 / torch.sqrt(var + eps)
    s = gamma * r
    ds = (dwk_f * wk).sum((0, 2))
    dt = (db_f.view(1, 1, -1) * wk).sum((0, 2))
    c1h = (ds * gamma - dt * mean * gamma) * (-0.5 * r ** 3) / K
    c0, c1 = -s * dt / K - 2 * mean * c1h, 2 * c1h
    dw = (dwk_f * s.view(1, -1, 1) + db_f.view(1, 1, -1) * (beta - mean * s).view(1, -1, 1)).reshape(3, 3, w.shape[1], w.shape[0]).permute(3, 2, 0, 1).contiguous() if want_dw else None
    return ((ds - mean * dt) * r if want_affine else None), (dt if want_affine else None), dw, c0, c1


def head(t, image, mask, hull=None, crop=0):
    img = torch.lerp(image, t, mask)
    l1 = (img - image).abs().mean((1, 2, 3))
    if not crop:
        return img, l1, None, None
    return img, l1, img[..., crop:-crop, crop:-crop].contiguous(), (hull[..., crop:-crop, crop:-crop].contiguous() if hull is not None else None)


def head_grad(t, img, image, mask, g_l1, d, crop=0, shape=None):
    ref = t if t is not None else img
    N, H, W = (ref.shape[0], ref.shape[2], ref.shape[3]) if ref is not None else shape
    like = ref if ref is not None else d
    v = torch.zeros((N, 3, H, W), dtype=like.dtype, device=like.device)
    if g_l1 is not None:
        v = v + g_l1.view(-1, 1, 1, 1) * torch.sign(img - image) / (3 * H * W)
    if d is not None:
        v[..., crop:H - crop, crop:W - crop] += d
    if mask is not None:
        v = mask * v
    if t is not None:
        v = (1 - t * t) * v
    return v.permute(0, 2, 3, 1).contiguous()


STAND_INS = dict(rmline_conv=conv, rmline_bn_stats=bn_stats, rmline_bn_fold=bn_fold, rmline_conv_dgrad=conv_dgrad, rmline_conv_wgrad=conv_wgrad,
                 rmline_bn_coef=bn_coef, rmline_head=head, rmline_head_grad=head_grad)


def install_ops(monkeypatch, ops):
    """Replace panic3d_amd.ops' operators by the closed forms above: RMLineModel and the two autograd Functions then run on the CPU in
    whatever dtype the model holds."""
    for name, fn in STAND_INS.items():
        monkeypatch.setattr(ops, name, fn)


# ---- gates -----------------------------------------------------------------------------------------------------------------------------------
EPS32 = 2.0 ** -24


def stats_bounds(x64):
    """(mean bound [C], var bound [C]) of the statistics of x64 [K, C] (float64 of the binary32 values)."""
    K = x64.shape[0]
    e = 8 * K ** 0.5 * EPS32
    mabs = x64.abs().mean(0)
    v = ((x64 - x64.mean(0)) ** 2).mean(0)
    return e * mabs, e * v + (e * mabs) ** 2


def step_results(model, batch, idx):
    """One training_step and backward of `model` (an RMLineModel or a RefModel) without an optimiser: the mean loss, the parameter
    gradients by name (None where there is none) and the buffers afterwards."""
    nets = (model.generator, model.discriminator)
    for p in model.parameters():
        p.grad = None
    for p in nets[1 - idx].parameters():
        p.requires_grad_(False)
    try:
        loss = model.training_step({k: v.clone() for k, v in batch.items()}, 0, idx)
        loss.backward()
    finally:
        for p in nets[1 - idx].parameters():
            p.requires_grad_(True)
    grads = {n: (p.grad.detach().clone() if p.grad is not None else None) for n, p in model.named_parameters()}
    bufs = {n: b.detach().clone() for n, b in model.named_buffers()}
    return loss.detach(), grads, bufs
