"""The training loss: the counterpart of the reference's StyleGAN2LossOrthoCondA (training/loss_orthocondA.py:56-738), the object its
training loop calls once per phase.

Device work goes through ops: the Gaussian blur in front of the discriminator and of the raw target (ops.blur), the L1 image term
(ops.l1_mean) and the render-resolution terms of a supervised view (ops.view_terms: two resizes, the box filter, three masks, the
alpha and depth terms and their gradients in one launch).  G, D, the resizes of the real images, the logistic terms and LPIPS are
the caller's modules and torch plumbing.  Random draws come from torch's global generator, on the same device and in the same order
as the reference's, so a seeded CPU run of both sees the same numbers.

The R1 penalty (Dreg / Dboth) runs when the discriminator has its recorded backward switched on (D.set_r1_grad(), DESIGN.md §4.21;
see StyleGAN2LossOrthoCondA); the sum of squares is ops.r1_penalty.  Not covered: the augmentation pipeline (any callable is applied as the reference
applies its own; its image-side operator is ops.augment_apply, DESIGN.md §4.20, but the pipe module that draws the parameters is not
ported).  LPIPS is any callable returning [N]; panic3d_amd.lpips.LPIPSLoss() is the HIP one
(DESIGN.md §4.14).
"""
import numpy as np
import torch

from . import ops
from .discriminator import filtered_resizing

F = torch.nn.functional

stats = {}  # name -> the last detached value reported (the default report hook)


def _store(name, value):
    stats[name] = value.detach() if isinstance(value, torch.Tensor) else value


report = _store  # the reference's training_stats.report(name, value): replace this module attribute to collect elsewhere


def mask_view_orthofront(front_xyz, front_alpha, view_xyz, view_alpha, boxwarp):
    """loss_orthocondA.py:35-54: which texels of a view show a surface point that the front view also shows.  The view's xyz are
    looked up (nearest, zeros outside) in the front view's alpha and depth; a texel counts when the front view is opaque there and
    the point lies no more than 1.5/255 of the box behind the front surface.  No gradient."""
    with torch.no_grad():
        grid = (1 - (view_xyz[:, [1, 0]] + boxwarp / 2) / boxwarp).permute(0, 2, 3, 1) * 2 - 1
        src = torch.cat([(front_alpha > 0.5).float(), front_xyz[:, 2:3]], dim=1).permute(0, 1, 3, 2)
        qs = F.grid_sample(src, grid, padding_mode="zeros", mode="nearest")
        behind = (view_xyz[:, 2:3] - qs[:, -1:]) < (1.5 / 255) * boxwarp
        return qs[:, :-1] * behind * (view_alpha > 0.5)


def _window(x, k, fill):
    o = k // 2  # the structuring element's origin
    return F.pad(x, [o, k - o - 1, o, k - o - 1], value=fill)


def dilation(x, k):
    """Grey dilation by a flat k x k structuring element with a geodesic border: the maximum over the in-bounds window.  Restates
    kornia.morphology.dilation(x, ones(k, k)) at kornia 0.6.5's defaults; NOT pinned against kornia (which this project cannot
    import), as paste.sobel_magnitude is not."""
    return F.max_pool2d(_window(x, k, float("-inf")), k, stride=1)


def erosion(x, k):
    """Grey erosion, the minimum over the in-bounds window: see dilation (equally unpinned against kornia)."""
    return -F.max_pool2d(_window(-x, k, float("-inf")), k, stride=1)


class StyleGAN2LossOrthoCondA:
    """accumulate_gradients(phase, real_img, real_c, real_cond, gen_z, gen_c, gain, cur_nimg) as the reference's training loop calls it,
    with the reference's constructor signature, defaults and attribute names, so that
    dnnlib.util.construct_class_by_name(device=..., G=..., D=..., augment_pipe=..., lpips_model=..., **loss_kwargs) works unchanged.

    Phases: Gcond, Gside-left / -right / -back, Grand, Gmain (with the lossmask_mode_adv / lossmask_mode_recon branches), Greg
    (reg_type l1, monotonic-detach, monotonic-fixed), Dmain, and Gboth / Dboth as the reference combines them.

    R1: the penalty differentiates the discriminator's input gradient a second time.  The discriminator's HIP backward is first order
    unless its recorded backward is switched on: with D.r1_grad true (DualDiscriminator.set_r1_grad()), Dreg and Dboth run as the
    reference's (:690-738: the real images' logits, torch.autograd.grad(..., create_graph=True, only_inputs=True) inside
    ops.no_weight_gradients(), ops.r1_penalty, the backward of the penalty times r1_gamma / 2).  Without the switch, with r1_gamma > 0
    a Dreg or Dboth phase raises RuntimeError(ops.R1_MESSAGE) before any forward; running the forward first would spend a generator
    and a discriminator pass on a phase that cannot finish.

    A defect of the reference that is not reproduced: its Greg style-mixing lines (:591, :635, :679) name the undefined variables z
    and c, a NameError whenever style_mixing_prob > 0; gen_z and gen_c are used here.

    lpips_model: any callable (image, target) -> [N] — panic3d_amd.lpips.LPIPSLoss() for the HIP path, or the trainer's own network,
    which torch differentiates; a positive LPIPS weight without one raises here.  The image receives the L1 gradient from ops.l1_mean
    and the LPIPS gradient from the model, both through autograd."""

    def __init__(self, device, G, D, lpips_model=None, augment_pipe=None, r1_gamma=10, style_mixing_prob=0,
                 pl_weight=0, pl_batch_shrink=2, pl_decay=0.01, pl_no_weight_grad=False, blur_init_sigma=0, blur_fade_kimg=0,
                 r1_gamma_init=0, r1_gamma_fade_kimg=0, neural_rendering_resolution_initial=64, neural_rendering_resolution_final=None,
                 neural_rendering_resolution_fade_kimg=0, gpc_reg_fade_kimg=1000, gpc_reg_prob=None, dual_discrimination=False,
                 filter_mode="antialiased", lambda_Gcond_lpips=10.0, lambda_Gcond_l1=1.0, lambda_Gcond_alpha_l2=0.0,
                 lambda_Gcond_depth_l2=0.0, lambda_Gcond_sides_lpips=0.0, lambda_Gcond_sides_l1=0.0, lambda_Gcond_sides_alpha_l2=0.0,
                 lambda_Gcond_sides_depth_l2=0.0, lambda_Gcond_back_lpips=0.0, lambda_Gcond_back_l1=0.0, lambda_Gcond_back_alpha_l2=0.0,
                 lambda_Gcond_back_depth_l2=0.0, lambda_Gcond_rand_lpips=0.0, lambda_Gcond_rand_l1=0.0, lambda_Gcond_rand_alpha_l2=0.0,
                 lambda_Gcond_rand_depth_l2=0.0, lossmask_mode_adv="none", lossmask_mode_recon="none", lambda_recon_lpips=0.0,
                 lambda_recon_l1=0.0, lambda_recon_alpha_l2=0.0, lambda_recon_depth_l2=0.0, paste_params_mode=None):
        given = dict(locals())
        for name, value in given.items():
            if name not in ("self", "paste_params_mode"):
                setattr(self, name, value)
        self.pl_mean = torch.zeros([], device=device)
        self.resample_filter = ops.setup_filter([1, 3, 3, 1], device=device)
        self.blur_raw_target = True
        assert self.gpc_reg_prob is None or (0 <= self.gpc_reg_prob <= 1)
        if lpips_model is None:
            wanted = [n for n, v in given.items() if n.startswith("lambda_") and n.endswith("_lpips") and v > 0]
            if wanted:
                raise ValueError(f"{', '.join(wanted)} > 0 needs an lpips_model (any callable (image, target) -> [N])")
        default_pp = {"mode": "default", "thresh_weight": 0.95, "thresh_edges": 0.02, "thresh_occ": 0.05, "offset_occ": 0.01,
                      "thresh_dxyz": 0.000005}
        self.paste_params_mode = paste_params_mode
        if paste_params_mode in ("A", "Agrad"):
            self.paste_params = dict(default_pp, grad_sample=paste_params_mode == "Agrad")
        elif paste_params_mode in (None, "none"):
            self.paste_params = None
        else:
            raise AssertionError(f"paste_params_mode {paste_params_mode!r} not understood")

    # ---- the two runs ------------------------------------------------------------------------------------------------------------------
    def _conditioning(self, c, swapping_prob, shape):
        if swapping_prob is None:
            return torch.zeros_like(c)
        return torch.where(torch.rand(shape, device=c.device) < swapping_prob, torch.roll(c.clone(), 1, 0), c)

    def _style_mix(self, ws, z, c, cond):
        if self.style_mixing_prob > 0:
            cutoff = torch.empty([], dtype=torch.int64, device=ws.device).random_(1, ws.shape[1])
            cutoff = torch.where(torch.rand([], device=ws.device) < self.style_mixing_prob, cutoff, torch.full_like(cutoff, ws.shape[1]))
            ws[:, cutoff:] = self.G.mapping(torch.randn_like(z), c, cond, update_emas=False)[:, cutoff:]
        return ws

    def run_G(self, z, c, cond, swapping_prob, neural_rendering_resolution, update_emas=False):
        ws = self.G.mapping(z, self._conditioning(c, swapping_prob, (c.shape[0], 1)), cond, update_emas=update_emas)
        ws = self._style_mix(ws, z, c, cond)
        gen_output = self.G.f({"ws": ws, "camera_params": c, "cond": cond, "normalize_images": True,
                               "neural_rendering_resolution": neural_rendering_resolution, "update_emas": update_emas,
                               "paste_params": self.paste_params})
        return gen_output, ws

    def run_D(self, img, c, cond, blur_sigma=0, blur_sigma_raw=0, update_emas=False):
        img["image"] = ops.blur(img["image"], blur_sigma)
        if self.augment_pipe is not None:
            ch, size, raw_size = img["image"].shape[1], img["image"].shape[2:], img["image_raw"].shape[2:]
            pair = self.augment_pipe(torch.cat([img["image"], F.interpolate(img["image_raw"], size=size, mode="bilinear", antialias=True)],
                                               dim=1))
            img["image"] = pair[:, :ch]
            img["image_raw"] = F.interpolate(pair[:, ch:], size=raw_size, mode="bilinear", antialias=True)
        return self.D(img, c, cond, update_emas=update_emas)

    # ---- one supervised view -----------------------------------------------------------------------------------------------------------
    def _view_loss(self, out, target, gt_alpha, gt_xyz, depth_mode, lambdas, names, q=None):
        """The block the reference writes out four times (:281-317, :345-402, :428-464, :534-570): LPIPS and L1 on the image, the alpha
        and depth terms at the render resolution, the weighted sum.  names: the five report names (lpips, l1, alpha, depth, total)."""
        lam_lpips, lam_l1, lam_alpha, lam_depth = lambdas
        lpips = self.lpips_model(out["image"], target).mean() if self.lpips_model is not None else None
        l1 = ops.l1_mean(out["image"], target)
        weights, xyz = out["image_weights"], out["image_xyz"]
        n = weights.shape[0]
        if n > 1:
            # The reference multiplies its [N,r,r] depth residual by the [N,1,r,r] mask (:307, :372-374, :454, :560), which broadcasts
            # to [N,N,r,r]: every sample's residual under every sample's mask, the mean over all N^2 r^2 values.  Reproduced through
            # the per-sample operator on the N^2 (mask sample, residual sample) pairs; the alpha term's mean is the same either way.
            i = torch.arange(n, device=weights.device)
            mask_of, resid_of = i.repeat_interleave(n), i.repeat(n)
            weights, gt_alpha, q = weights[mask_of], gt_alpha[mask_of], (q[mask_of] if q is not None else None)
            xyz, gt_xyz = xyz[resid_of], gt_xyz[resid_of]
        terms = ops.view_terms(weights, xyz, gt_alpha, gt_xyz, depth_mode, q)
        alpha_l2, depth_l2 = terms[0], terms[1]
        for name, value in zip(names, (lpips, l1, alpha_l2, depth_l2)):
            if value is not None:
                report(name, value)
        total = lam_l1 * l1 + lam_alpha * alpha_l2 + lam_depth * depth_l2 if lpips is None else \
            lam_lpips * lpips + lam_l1 * l1 + lam_alpha * alpha_l2 + lam_depth * depth_l2
        report(names[4], total)
        return total

    def _render_view(self, gen_z, real_cond, camera, azimuth=None):
        xin = {"z": gen_z, "cond": real_cond, "camera_params": camera, "paste_params": self.paste_params}
        if azimuth is not None:
            n, dev = len(gen_z), gen_z.device
            xin.update(elevations=torch.zeros(n, device=dev), azimuths=azimuth * torch.ones(n, device=dev) if azimuth else
                       torch.zeros(n, device=dev), distances=torch.ones(n, device=dev))
        return self.G.f(xin)

    def _supervised(self):
        mode = self.G.cond_mode
        if mode == "none":
            return False
        assert mode.startswith("ortho_front."), f"cond_mode {mode} not understood"
        return True

    def _sigma_pair(self, ws, real_cond, n_points, perturb):
        initial = torch.rand((ws.shape[0], n_points, 3), device=ws.device) * 2 - 1
        coords = torch.cat([initial, perturb(initial)], dim=1)
        sigma = self.G.sample_mixed(coords, torch.randn_like(coords), ws, real_cond, update_emas=False)["sigma"]
        half = sigma.shape[1] // 2
        return sigma[:, :half], sigma[:, half:]

    # ---- the phases --------------------------------------------------------------------------------------------------------------------
    def accumulate_gradients(self, phase, real_img, real_c, real_cond, gen_z, gen_c, gain, cur_nimg):
        rk = self.G.rendering_kwargs
        if rk.get("density_reg", 0) == 0:
            phase = {"Greg": "none", "Gboth": "Gmain"}.get(phase, phase)
        if self.r1_gamma == 0:
            phase = {"Dreg": "none", "Dboth": "Dmain"}.get(phase, phase)
        if phase in ("Dreg", "Dboth") and not getattr(self.D, "r1_grad", False):
            raise RuntimeError(ops.R1_MESSAGE)
        blur_sigma = max(1 - cur_nimg / (self.blur_fade_kimg * 1e3), 0) * self.blur_init_sigma if self.blur_fade_kimg > 0 else 0
        fade = min(cur_nimg / (self.gpc_reg_fade_kimg * 1e3), 1) if self.gpc_reg_fade_kimg > 0 else 1
        swapping_prob = (1 - fade) * 1 + fade * self.gpc_reg_prob if self.gpc_reg_prob is not None else None
        if self.neural_rendering_resolution_final is not None:
            fade = min(cur_nimg / (self.neural_rendering_resolution_fade_kimg * 1e3), 1)
            res = int(np.rint(self.neural_rendering_resolution_initial * (1 - fade) + self.neural_rendering_resolution_final * fade))
        else:
            res = self.neural_rendering_resolution_initial

        real_raw = filtered_resizing(real_img, size=res, f=self.resample_filter, filter_mode=self.filter_mode)
        if self.blur_raw_target:
            real_raw = ops.blur(real_raw, blur_sigma)
        real_img = {"image": real_img, "image_raw": real_raw,
                    "image_raw_noblur": F.interpolate(real_img, real_raw.shape[-1], mode="bilinear")}

        lmask = mask_view_orthofront(real_cond["image_ortho_front_xyz"], real_cond["image_ortho_front_alpha"], real_cond["image_xyz"],
                                     real_cond["image_alpha"], rk["box_warp"])
        raw_size = real_img["image_raw"].shape[-1]
        if self.lossmask_mode_adv != "none":
            lmask_adv = 1 - erosion(lmask, int(self.lossmask_mode_adv.split("_")[-1]))
            lmask_adv_raw = (F.interpolate(lmask_adv, raw_size, mode="bilinear") > 0.5).float()
        if self.lossmask_mode_recon != "none":
            lmask_recon = dilation(lmask, int(self.lossmask_mode_recon.split("_")[-1]))
            lmask_recon_raw = (F.interpolate(lmask_recon, raw_size, mode="bilinear") > 0.5).float()

        # the conditioned synthesis must match the condition (the front view)
        if phase in ("Gcond", "Gboth") and self._supervised():
            out = self._render_view(gen_z, real_cond, real_cond["image_ortho_front_camera"], azimuth=0)
            self._view_loss(out, real_cond["image_ortho_front"], real_cond["image_ortho_front_alpha"], real_cond["image_ortho_front_xyz"],
                            "z", (self.lambda_Gcond_lpips, self.lambda_Gcond_l1, self.lambda_Gcond_alpha_l2, self.lambda_Gcond_depth_l2),
                            [f"Loss/G/cond/{t}" for t in ("lpips", "l1", "alpha_l2", "depth_l2")] + ["Loss/G/cond"]).backward()

        # ... the left, right and back views
        if phase in ("Gside-left", "Gside-right", "Gside-back") and self._supervised():
            view = phase.split("-")[-1]
            out = self._render_view(gen_z, real_cond, real_cond[f"image_ortho_{view}_camera"], azimuth={"left": 90, "right": -90, "back": 180}[view])
            side = "back" if view == "back" else "sides"
            lambdas = tuple(getattr(self, f"lambda_Gcond_{side}_{t}") for t in ("lpips", "l1", "alpha_l2", "depth_l2"))
            self._view_loss(out, real_cond[f"image_ortho_{view}"], real_cond[f"image_ortho_{view}_alpha"], real_cond[f"image_ortho_{view}_xyz"],
                            "z" if view == "back" else "x", lambdas,
                            [f"Loss/G/sides/{view}/{t}" for t in ("lpips", "l1", "alpha_l2", "depth_l2")] + [f"Loss/G/sides/{view}"]).backward()

        # ... and the random view
        if phase in ("Grand", "Gboth") and self._supervised():
            out = self._render_view(gen_z, real_cond, real_cond["image_camera"])
            self._view_loss(out, real_cond["image"], real_cond["image_alpha"], real_cond["image_xyz"], "norm",
                            (self.lambda_Gcond_rand_lpips, self.lambda_Gcond_rand_l1, self.lambda_Gcond_rand_alpha_l2,
                             self.lambda_Gcond_rand_depth_l2),
                            [f"Loss/G/rand/{t}" for t in ("lpips", "l1", "alpha_l2", "depth_l2")] + ["Loss/G/rand"]).backward()

        # Gmain: maximise the logits of generated images
        if phase in ("Gmain", "Gboth"):
            gen_img, _ = self.run_G(gen_z, gen_c, real_cond, swapping_prob=swapping_prob, neural_rendering_resolution=res)
            if self.lossmask_mode_adv != "none":
                assert self.lossmask_mode_adv.split("_")[0] == "replace"
                for_adv = {"image": torch.lerp(real_img["image"], gen_img["image"], lmask_adv),
                           "image_raw": torch.lerp(real_img["image_raw_noblur"], gen_img["image_raw"], lmask_adv_raw)}
            else:
                for_adv = gen_img
            gen_logits = self.run_D(for_adv, gen_c, real_cond, blur_sigma=blur_sigma)
            report("Loss/scores/fake", gen_logits)
            report("Loss/signs/fake", gen_logits.sign())
            loss_Gmain = F.softplus(-gen_logits)
            report("Loss/G/loss", loss_Gmain)
            if self.lossmask_mode_recon != "none":
                # as in the reference, run_D has replaced gen_img["image"] by its blurred version when no adversarial mask copied it
                out = dict(gen_img, image=torch.lerp(real_img["image"], gen_img["image"], lmask_recon) * 0.5 + 0.5)
                loss_Grecon = self._view_loss(out, real_cond["image"], real_cond["image_alpha"], real_cond["image_xyz"], "norm",
                                              (self.lambda_recon_lpips, self.lambda_recon_l1, self.lambda_recon_alpha_l2,
                                               self.lambda_recon_depth_l2),
                                              [f"Loss/G/recon/{t}" for t in ("lpips", "l1", "alpha_l2", "depth_l2")] + ["Loss/G/loss_recon"],
                                              q=lmask_recon_raw)
            else:
                loss_Grecon = torch.zeros_like(loss_Gmain)
            (loss_Gmain.mean().mul(gain) + loss_Grecon.mean()).backward()

        # Greg: the density regularisation
        reg_type = rk.get("reg_type") if phase in ("Greg", "Gboth") and rk.get("density_reg", 0) > 0 else None
        if reg_type in ("monotonic-detach", "monotonic-fixed"):
            ws = self.G.mapping(gen_z, self._conditioning(gen_c, swapping_prob, []), real_cond, update_emas=False)
            behind = lambda p: p + torch.tensor([0, 0, -1], device=p.device) * (1 / 256) * rk["box_warp"]
            front, back = self._sigma_pair(ws, real_cond, 2000, behind)
            if reg_type == "monotonic-detach":
                front = front.detach()
            (torch.relu(front - back).mean() * 10).mul(gain).backward()
        if reg_type in ("l1", "monotonic-detach", "monotonic-fixed"):
            ws = self.G.mapping(gen_z, self._conditioning(gen_c, swapping_prob, []), real_cond, update_emas=False)
            ws = self._style_mix(ws, gen_z, gen_c, real_cond)
            dist = rk["density_reg_p_dist"] if reg_type == "l1" else None
            jitter = (lambda p: p + torch.randn_like(p) * dist) if reg_type == "l1" else \
                (lambda p: p + torch.randn_like(p) * (1 / 256) * rk["box_warp"])
            a, b = self._sigma_pair(ws, real_cond, 1000, jitter)
            (F.l1_loss(a, b) * rk["density_reg"]).mul(gain).backward()

        # Dmain: minimise the logits of generated images, maximise those of real ones
        loss_Dgen = 0
        if phase in ("Dmain", "Dboth"):
            gen_img, _ = self.run_G(gen_z, gen_c, real_cond, swapping_prob=swapping_prob, neural_rendering_resolution=res, update_emas=True)
            gen_logits = self.run_D(gen_img, gen_c, real_cond, blur_sigma=blur_sigma, update_emas=True)
            report("Loss/scores/fake", gen_logits)
            report("Loss/signs/fake", gen_logits.sign())
            loss_Dgen = F.softplus(gen_logits)
            loss_Dgen.mean().mul(gain).backward()

        # Dmain: ... and maximise those of real ones; Dreg: the R1 penalty on the real images (:702-738)
        if phase in ("Dmain", "Dreg", "Dboth"):
            with_r1 = phase in ("Dreg", "Dboth")
            real = {"image": real_img["image"].detach().requires_grad_(with_r1), "image_raw": real_img["image_raw"].detach().requires_grad_(with_r1)}
            real_logits = self.run_D(real, real_c, real_cond, blur_sigma=blur_sigma)  # (run_D replaces real["image"] by its blurred version)
            report("Loss/scores/real", real_logits)
            report("Loss/signs/real", real_logits.sign())
            loss_Dreal = 0
            if phase in ("Dmain", "Dboth"):
                loss_Dreal = F.softplus(-real_logits)
                report("Loss/D/loss", loss_Dgen + loss_Dreal)
            loss_Dr1 = 0
            if with_r1:
                inputs = [real["image"], real["image_raw"]] if self.dual_discrimination else [real["image"]]
                with ops.no_weight_gradients():
                    r1_grads = torch.autograd.grad(outputs=[real_logits.sum()], inputs=inputs, create_graph=True, only_inputs=True)
                r1_penalty = ops.r1_penalty(*r1_grads)
                loss_Dr1 = r1_penalty * (self.r1_gamma / 2)
                report("Loss/r1_penalty", r1_penalty)
                report("Loss/D/reg", loss_Dr1)
            (loss_Dreal + loss_Dr1).mean().mul(gain).backward()
