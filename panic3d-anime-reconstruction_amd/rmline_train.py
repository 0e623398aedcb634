"""Training the illustration-to-render module on the HIP operators of include/p3d_rmline_grad.h: `RMLineModel` has the
surface of the reference's `rmlineganA.Model` (rmlineganA.py:57-298) without Lightning — the generator of rmline.RMLineGenerator and
the patch discriminator as trainable `nn.Sequential`s of torch's own modules under the reference's names, `forward`,
`forward_discriminator`, `loss`, `training_step`, `validation_step`, `configure_optimizers`, and `fit_step`, which does for one batch
what Lightning's automatic optimisation does with the two optimisers.

Both networks stay in train mode in both steps: every batch norm normalises with that call's batch statistics and updates its running
statistics and `num_batches_tracked` in the generator's step (B patches) and again in the discriminator's (2 B patches).

Everything is binary32, as the inference module is.  The reference trains under Lightning's `precision=16` (AMP): that is NOT reproduced.
The reference's patch pickles (`rmlineERA_train.pkl`), its data loader and the dilation augment are not part of this module, and the
module is unchecked against them; it is checked against a float64 restatement of the reference's lines on seeded patches.
"""
import torch

from . import ops
from .rmline import LEAKY_SLOPE, RMLineGenerator

__all__ = ["RMLineModel"]


class RMLineModel(torch.nn.Module):
    """rmlineganA.Model on the HIP path.  Keyword arguments under the reference's names with its defaults (rmlineganA.py:32-55), plus
    `size` (prep.size: the side of a training patch) and `seed`.  The boolean switches are built at the reference's values only.

    A batch is {'image' [B,2,3,S,S], 'line_mask' [B,2,1,S,S], 'face_hull' [B,2,1,S,S], 'real_label' [B,2] = (0, 1)} of float32 device
    tensors: index 0 of a pair an illustration patch, index 1 a render patch.  Inputs must not require grad.  In eval mode `forward`
    runs the folded inference path of RMLineGenerator (the same bits); `to_generator()` hands the weights to RMLineWrapper."""

    def __init__(self, patch_size=9, gen_depth=6, gen_width=32, gen_batchnorm=True, gen_use_hull=True, gen_mask_input=True, dis_depth=4,
                 dis_width=16, dis_batchnorm=True, dis_use_hull=True, lerp_output=True, label_smoothing=0.8, lr_gen=0.001, lr_dis=0.001,
                 lambda_l1=1.0, lambda_adv=1.0, size=21, seed=0):
        super().__init__()
        for name, v in (("gen_batchnorm", gen_batchnorm), ("gen_use_hull", gen_use_hull), ("gen_mask_input", gen_mask_input),
                        ("dis_batchnorm", dis_batchnorm), ("dis_use_hull", dis_use_hull), ("lerp_output", lerp_output)):
            if not v:
                raise NotImplementedError(f"RMLineModel: {name}=False is not built (the reference trains with True)")
        self.patch_size, self.size = int(patch_size), int(size)
        self.gen_depth, self.gen_width, self.dis_depth, self.dis_width = int(gen_depth), int(gen_width), int(dis_depth), int(dis_width)
        self.gen_batchnorm = self.gen_use_hull = self.gen_mask_input = self.dis_batchnorm = self.dis_use_hull = self.lerp_output = True
        self.label_smoothing, self.lr_gen, self.lr_dis = float(label_smoothing), float(lr_gen), float(lr_dis)
        self.lambda_l1, self.lambda_adv = float(lambda_l1), float(lambda_adv)
        if self.gen_depth < 1 or self.dis_depth < 1 or not 1 <= self.gen_width <= 64 or not 1 <= self.dis_width <= 64:
            raise ValueError("RMLineModel: depths >= 1 and 1 <= widths <= 64")
        assert self.patch_size + 2 * self.gen_depth <= self.size  # rmlineganA.py:63
        if self.patch_size - 2 * self.dis_depth < 1:
            raise ValueError(f"RMLineModel: a {self.patch_size} x {self.patch_size} patch is too small for {self.dis_depth} unpadded layers")

        def stack(chin, w, depth, cout, tail):  # rmlineganA.py:65-100
            mods = []
            for i in range(depth):
                mods.append(torch.nn.Conv2d(chin if i == 0 else w, w if i != depth - 1 else cout, 3, stride=1, padding=0))
                if i != depth - 1:
                    mods += [torch.nn.LeakyReLU(), torch.nn.BatchNorm2d(w)]
            return torch.nn.Sequential(*(mods + tail))
        self.generator = stack(4, self.gen_width, self.gen_depth, 3, [torch.nn.Tanh()])
        self.discriminator = stack(4, self.dis_width, self.dis_depth, self.dis_width, [])
        g = torch.Generator().manual_seed(int(seed))
        with torch.no_grad():  # seeded like RMLineGenerator: the generator of a fresh model is RMLineGenerator(seed)'s
            for seq in (self.generator, self.discriminator):
                for m in seq:
                    if isinstance(m, torch.nn.Conv2d):
                        bound = 1.0 / float(m.weight[0].numel()) ** 0.5
                        m.weight.copy_((torch.rand(m.weight.shape, generator=g) * 2 - 1) * bound)
                        m.bias.copy_((torch.rand(m.bias.shape, generator=g) * 2 - 1) * bound)
        self._cache = {}  # (a dict: the cached RMLineGenerator must not become a submodule)

    # ---- the two stacks ----------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _stack_args(seq):
        """(params in RmlineStackFunction's order, the batch norms) of one nn.Sequential."""
        convs = [m for m in seq if isinstance(m, torch.nn.Conv2d)]
        bns = [m for m in seq if isinstance(m, torch.nn.BatchNorm2d)]
        params = []
        for i, c in enumerate(convs):
            params += [c.weight, c.bias]
            if i < len(bns):
                params += [bns[i].weight, bns[i].bias]
        return params, bns

    @staticmethod
    def _check_inputs(x, names):
        for n in names:
            t = x[n]
            if not isinstance(t, torch.Tensor):
                raise ValueError(f"RMLineModel: {n} is a tensor")
            if torch.is_grad_enabled() and t.requires_grad:
                raise NotImplementedError(f"RMLineModel: {n} requires grad; gradients with respect to the inputs are not built")

    def forward(self, x, pad=True):
        """rmlineganA.py:108-143: {'image': the tanh output, 'line_mask', 'face_hull'}."""
        self._check_inputs(x, ("image", "line_mask", "face_hull"))
        if not self.training:
            return self.to_generator().forward(x, pad=pad)
        image, mask, hull = x["image"], x["line_mask"], x["face_hull"]
        params, bns = self._stack_args(self.generator)
        spec = dict(pad=self.gen_depth if pad is True else (0 if pad is False else int(pad)), slope=LEAKY_SLOPE, last_act="tanh", planar=True, bns=bns)
        out = ops.RmlineStackFunction.apply(spec, image, mask, hull, *params)
        return {"image": out, "line_mask": mask, "face_hull": hull}

    def forward_discriminator(self, x):
        """rmlineganA.py:145-172 on an UNCROPPED {'image', 'face_hull'}: the centre patch_size window (F.pad by a negative amount) through
        the discriminator -> {'logits' [N], 'probability'}.  Used by `loss` through its fused head; this form is for callers."""
        img, hull = x["image"], x["face_hull"]
        crop = -((self.patch_size - img.shape[-1]) // 2)
        if crop < 0:
            raise NotImplementedError("RMLineModel: a patch larger than the image (replicate padding in front of the discriminator)")
        if crop:
            img, hull = img[..., crop:-crop, crop:-crop].contiguous(), hull[..., crop:-crop, crop:-crop].contiguous()
        return self._discriminate(img, hull)

    def _discriminate(self, crop_img, crop_hull):
        if not self.training:
            raise NotImplementedError("RMLineModel: the discriminator runs in train mode only (the reference never evaluates it)")
        params, bns = self._stack_args(self.discriminator)
        spec = dict(pad=0, slope=LEAKY_SLOPE, last_act="none", planar=False, bns=bns)
        out = ops.RmlineStackFunction.apply(spec, crop_img, None, crop_hull, *params)  # [N, h, w, C]
        logits = out.mean((1, 2, 3))
        return {"logits": logits, "probability": logits.sigmoid()}

    def loss(self, pred, gt):
        """rmlineganA.py:174-208 -> {'loss', 'loss_l1', 'loss_adv'} per sample.  pred['image'] becomes the lerped image, as there."""
        self._check_inputs(gt, ("image", "line_mask", "face_hull"))
        S = gt["image"].shape[-1]
        crop = -((self.patch_size - S) // 2)
        if crop <= 0:
            raise NotImplementedError("RMLineModel: patch_size must be smaller than the image")
        img, loss_l1, crop_img, crop_hull = ops.RmlineHeadFunction.apply(pred["image"], gt["image"], gt["line_mask"], gt["face_hull"], crop)
        pred["image"] = img
        outd = self._discriminate(crop_img, crop_hull)
        sm = self.label_smoothing
        loss_adv = torch.nn.functional.binary_cross_entropy_with_logits(outd["logits"], gt["real_label"] * sm + sm / 2, reduction="none")
        return {"loss": self.lambda_l1 * loss_l1 + self.lambda_adv * loss_adv, "loss_l1": loss_l1, "loss_adv": loss_adv}

    # ---- the steps ---------------------------------------------------------------------------------------------------------------------
    def training_step(self, batch, batch_idx=0, optimizer_idx=0):
        """rmlineganA.py:209-233: the mean loss of the generator's step (fakes only, labels forced to 1) or the discriminator's (both
        patches of every pair, true labels).  The last step's mean losses are kept in `self.logged`, as the reference logs them."""
        if optimizer_idx == 0:
            batch = {k: v[:, 0] for k, v in batch.items() if isinstance(v, torch.Tensor)}
            batch["real_label"] = torch.ones_like(batch["real_label"])
            tag = "train_gen_"
        elif optimizer_idx == 1:
            batch = {k: v.reshape(-1, *v.shape[2:]) for k, v in batch.items() if isinstance(v, torch.Tensor)}
            tag = "train_dis_"
        else:
            raise ValueError("optimizer_idx: 0 (generator) or 1 (discriminator)")
        batch = {k: v.contiguous() for k, v in batch.items()}
        pred = self.forward(batch)
        loss = self.loss(pred, batch)
        reduced = {k: v.mean() for k, v in loss.items()}
        self.logged = getattr(self, "logged", {})
        self.logged.update({tag + k: v.detach() for k, v in reduced.items()})
        return reduced["loss"]

    def validation_step(self, batch, batch_idx=0, dataloader_idx=0):
        """rmlineganA.py:234-251: the lerped output of index 0 of every pair."""
        bns = batch.get("bn")
        batch = {k: v[:, 0].contiguous() for k, v in batch.items() if isinstance(v, torch.Tensor) and k != "bn"}
        with torch.no_grad():
            pred = self.forward(batch)
            return {"bns": bns, "images": torch.lerp(batch["image"], pred["image"], batch["line_mask"])}

    def configure_optimizers(self):
        """rmlineganA.py:294-298 with this project's Adam (torch.optim.Adam's update in one launch per network)."""
        from . import optim
        return [optim.Adam(self.generator.parameters(), lr=self.lr_gen), optim.Adam(self.discriminator.parameters(), lr=self.lr_dis)], []

    def fit_step(self, batch, optimizers, batch_idx=0):
        """One batch of Lightning's automatic optimisation: for optimiser 0 (the generator's) then 1 (the discriminator's): the other
        network's parameters stop requiring grad, training_step, zero_grad, backward, step, and they require grad again.  optimizers:
        the two optimisers, or what configure_optimizers returns.  Returns the two mean losses (device tensors: nothing synchronises)."""
        if isinstance(optimizers, tuple) and len(optimizers) == 2 and isinstance(optimizers[0], (list, tuple)):
            optimizers = optimizers[0]
        if len(optimizers) != 2:
            raise ValueError("fit_step: two optimisers, the generator's and the discriminator's")
        nets, losses = (self.generator, self.discriminator), []
        for idx, opt in enumerate(optimizers):
            other = [p for p in nets[1 - idx].parameters()]
            was = [p.requires_grad for p in other]
            for p in other:
                p.requires_grad_(False)
            try:
                loss = self.training_step(batch, batch_idx, idx)
                opt.zero_grad()
                loss.backward()
                opt.step()
            finally:
                for p, r in zip(other, was):
                    p.requires_grad_(r)
            losses.append(loss.detach())
        return losses

    # ---- hand-over ---------------------------------------------------------------------------------------------------------------------
    def to_generator(self):
        """An RMLineGenerator (inference, folded batch norms) holding this model's generator, on its device; cached until a parameter
        or buffer of the generator is written."""
        src = list(self.generator.parameters()) + list(self.generator.buffers())
        key = tuple((id(t), t._version, t.device) for t in src)
        if self._cache.get("key") != key:
            gen = RMLineGenerator(gen_depth=self.gen_depth, gen_width=self.gen_width)
            gen.load_state_dict({k: v.detach() for k, v in self.state_dict().items()})
            self._cache = {"key": key, "gen": gen.to(src[0].device)}
        return self._cache["gen"]
