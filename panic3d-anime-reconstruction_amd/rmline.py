"""The illustration-to-render module on the HIP operators of include/p3d_rmline.h: what the reference runs on every
subject before `G.f` (generate.py:68-92) to make `cond['image_ortho_front']`, the illustration with its drawn lines removed.

`RMLineWrapper(model_or_path)` has the reference wrapper's call (rmline_wrapper.py:15-50): a Difference-of-Gaussians response of the
image composited on white is thresholded, dilated by a 2 x 2 element and cleared inside the face hull; the generator repaints the image
from what is left, and the result is `lerp(image, generated, mask)` with the input's alpha put back.  `RMLineGenerator` is that generator
(rmlineganA.py:57-143): `gen_depth` UNPADDED 3 x 3 convolutions, LeakyReLU(0.01) and BatchNorm2d between them, tanh at the end, on the
replicate-padded stack of image * (1 - mask) and hull; parameters under the reference's names `generator.<index>.*`.  Inference only,
in binary32 as the reference's evaluation runs it (generate.py:38: `.eval().to(device)`, no autocast), eval-mode batch norm only.  The
batch norm follows the activation and no convolution pads with zeros, so each one folds EXACTLY into the convolution after it.

`face_hull(kpts, size)` restates the wrapper's hull of the detected face (rmline_wrapper.py:65-120) on the host.  It is NOT pinned
against skimage.morphology.convex_hull_image, which this project cannot import: see its docstring.

The released checkpoint `rmlineE_rmlineganA_n04` was not available where this was written.  A freshly built model holds seeded random
weights: it is a line remover's architecture, not THE line remover, until `load_state_dict` / `load_checkpoint` are given the real
arrays.  Reading the real file is best-effort and UNCHECKED against it.
"""
import numpy as np
import torch

from . import memo, ops

LEAKY_SLOPE = 0.01  # nn.LeakyReLU()'s default (rmlineganA.py:73)
KEYPOINT_GROUPS = dict(chin=[0, 1, 2, 3, 4], eyelash_right=[5, 6, 7], eyelash_left=[8, 9, 10], eye_right=[11, 12, 13, 14, 15, 16],
                       eye_left=[17, 18, 19, 20, 21, 22], nose=[23], mouth=[24, 25, 26, 27])  # rmline_wrapper.py:65-93


def fold_generator(seq):
    """[(wk [9,Ci,Co], bias [Co], act, slope)] per convolution of the generator's nn.Sequential, each eval-mode batch norm folded into
    the NEXT convolution in float64 and rounded once: with s = gamma / sqrt(var + eps) (that batch norm's own eps) and
    shift = beta - mean s of the batch norm in front, w' = w s[ci] and b' = b + sum over (ci, taps) of w shift[ci].  Exact because the batch norm follows the activation and the
    convolutions are unpadded: every tap of every output sees a real, shifted input.  wk is w'.permute(2, 3, 1, 0)."""
    out, scale, shift = [], None, None
    mods = list(seq)
    for i, m in enumerate(mods):
        if isinstance(m, torch.nn.Conv2d):
            w, b = m.weight.detach().double(), m.bias.detach().double()
            if scale is not None:
                b = b + (w * shift.view(1, -1, 1, 1)).sum(dim=(1, 2, 3))
                w = w * scale.view(1, -1, 1, 1)
                scale = shift = None
            Co, Ci = w.shape[:2]
            nxt = mods[i + 1] if i + 1 < len(mods) else None
            act, slope = ("leaky", float(nxt.negative_slope)) if isinstance(nxt, torch.nn.LeakyReLU) else (("tanh", 0.0) if isinstance(nxt, torch.nn.Tanh) else ("none", 0.0))
            out.append((w.permute(2, 3, 1, 0).reshape(9, Ci, Co).float().contiguous(), b.float().contiguous(), act, slope))
        elif isinstance(m, torch.nn.BatchNorm2d):
            scale = m.weight.detach().double() / torch.sqrt(m.running_var.detach().double() + float(m.eps))
            shift = m.bias.detach().double() - m.running_mean.detach().double() * scale
    if scale is not None:
        raise ValueError("fold_generator: a batch norm with no convolution after it")
    return out


class RMLineGenerator(torch.nn.Module):
    """The generator of the reference's rmlineganA model on the HIP path.

    forward(x, pad=True) with x = {'image' [N,3,H,W] in [0, 1], 'line_mask' [N,1,H,W], 'face_hull' [N,1,H,W]} returns
    {'image': tanh output, 'line_mask', 'face_hull'} like rmlineganA.py:105-143: the stack of image * (1 - mask) (gen_mask_input) and
    hull (gen_use_hull), replicate-padded by gen_depth when pad (so that the output has the input's size; without it the output loses
    gen_depth pixels on each side), through the convolutions.  fused=True runs all layers in ONE call into the library; fused=False
    calls the operator layer by layer (the same kernels, the same bits).

    `generator` is an nn.Sequential of torch's own modules at the reference's indices (convolutions 0, 3, 6, ..., batch norms 2, 5, ...)
    — containers of the names and arrays only, never called.  A Lightning checkpoint's `state_dict` loads; its `discriminator.*` entries
    are ignored.  Every parameter has requires_grad=False; the module is always in eval mode."""

    def __init__(self, gen_depth=6, gen_width=32, gen_batchnorm=True, gen_use_hull=True, gen_mask_input=True, seed=0):
        super().__init__()
        self.gen_depth, self.gen_width = int(gen_depth), int(gen_width)
        self.gen_batchnorm, self.gen_use_hull, self.gen_mask_input = bool(gen_batchnorm), bool(gen_use_hull), bool(gen_mask_input)
        if self.gen_depth < 1 or not 1 <= self.gen_width <= 64:
            raise ValueError("RMLineGenerator: gen_depth >= 1 and 1 <= gen_width <= 64")
        gen, chin, w = [], 3 + int(self.gen_use_hull), self.gen_width
        for i in range(self.gen_depth):  # rmlineganA.py:65-82
            gen.append(torch.nn.Conv2d(chin if i == 0 else w, w if i != self.gen_depth - 1 else 3, 3, stride=1, padding=0))
            if i != self.gen_depth - 1:
                gen.append(torch.nn.LeakyReLU())
                if self.gen_batchnorm:
                    gen.append(torch.nn.BatchNorm2d(w))
        gen.append(torch.nn.Tanh())
        self.generator = torch.nn.Sequential(*gen)
        g = torch.Generator().manual_seed(int(seed))
        with torch.no_grad():  # seeded: two fresh models are the same model
            for m in self.generator:
                if isinstance(m, torch.nn.Conv2d):
                    bound = 1.0 / float(np.sqrt(m.weight[0].numel()))
                    m.weight.copy_((torch.rand(m.weight.shape, generator=g) * 2 - 1) * bound)
                    m.bias.copy_((torch.rand(m.bias.shape, generator=g) * 2 - 1) * bound)
        for p in self.parameters():
            p.requires_grad_(False)
        super().train(False)
        self._folded, self._folded_key, self._programs = None, None, {}

    def train(self, mode=True):
        if mode:
            raise NotImplementedError("RMLineGenerator is inference only: eval-mode batch norm, no backward")
        return super().train(False)

    # ---- parameters ------------------------------------------------------------------------------------------------------------------
    def load_state_dict(self, state_dict, strict=True, **kw):
        """The reference model's `state_dict` (generator.* and discriminator.*): the discriminator's entries are ignored."""
        return super().load_state_dict({k: v for k, v in state_dict.items() if not k.startswith("discriminator.")}, strict=strict, **kw)

    @staticmethod
    def hyper_parameters(ck):
        """The constructor's arguments from a Lightning checkpoint's `hyper_parameters` (`model.gen_*`), defaults where absent."""
        hp = ck.get("hyper_parameters", {}) or {}
        margs = hp.get("model", hp) if hasattr(hp, "get") else {}
        names = ("gen_depth", "gen_width", "gen_batchnorm", "gen_use_hull", "gen_mask_input")
        return {n: margs[n] for n in names if hasattr(margs, "get") and margs.get(n) is not None}

    @classmethod
    def from_checkpoint(cls, path):
        """Build from {'state_dict', 'hyper_parameters'} as Lightning writes them.  Best-effort and unchecked against the real file:
        torch.load runs with its default `weights_only` (True in recent torch), which refuses a checkpoint whose hyper_parameters pickle
        the reference's own `Dict` class — load such a file yourself (`torch.load(path, weights_only=False)` with the reference tree
        importable) and pass its `state_dict` to load_state_dict and its `hyper_parameters['model']` to the constructor."""
        ck = torch.load(path, map_location="cpu")
        model = cls(**cls.hyper_parameters(ck))
        model.load_state_dict(ck.get("state_dict", ck))
        return model

    def load_checkpoint(self, path):
        """The Lightning checkpoint's `state_dict` into this model; its hyper_parameters must describe this architecture.  The same
        caveat as from_checkpoint: torch.load's default `weights_only` refuses pickled objects of the reference's classes."""
        ck = torch.load(path, map_location="cpu")
        for n, v in self.hyper_parameters(ck).items():
            if type(getattr(self, n))(v) != getattr(self, n):
                raise ValueError(f"load_checkpoint: the checkpoint has {n}={v}, this model {getattr(self, n)}")
        self.load_state_dict(ck.get("state_dict", ck))
        return self

    def _sources(self):
        return [t for t in list(self.parameters()) + list(self.buffers()) if t.dtype.is_floating_point]

    def folded(self):
        """The operators' operands, derived from the parameters (fold_generator) and moved to their device.  Cached under memo's
        convention — identity and `_version` of every tensor they were derived from — so an in-place write (`copy_`, `load_state_dict`)
        re-derives them; memo.set_enabled(False) derives them on every call."""
        key = tuple((id(t), t._version, t.device) for t in self._sources())
        if self._folded is None or self._folded_key != key or not memo.enabled():
            dev = self.generator[0].weight.device
            self._folded = [(wk.to(dev), b.to(dev), act, slope) for wk, b, act, slope in fold_generator(self.generator)]
            self._folded_key, self._programs = key, {}
        return self._folded

    def program(self, plan=0):
        """The ops.RmlineProgram of the folded layers, cached with them."""
        f = self.folded()
        if plan not in self._programs or not memo.enabled():
            layers = [dict(wk=wk, bias=b, act=act, slope=slope, plan=plan) for wk, b, act, slope in f]
            self._programs[plan] = ops.RmlineProgram(layers, f[0][0].device)
        return self._programs[plan]

    # ---- the call ----------------------------------------------------------------------------------------------------------------------
    def _check(self, image, mask, hull):
        for name, t, ch in (("image", image, 3), ("line_mask", mask, 1), ("face_hull", hull, 1)):
            if t is None:
                continue
            if not isinstance(t, torch.Tensor) or t.ndim != 4 or t.shape[1] != ch:
                raise ValueError(f"RMLineGenerator: {name} is [N,{ch},H,W]")
            if t.dtype != torch.float32:
                raise RuntimeError(f"{name} must be torch.float32, got {t.dtype}")
            if t.shape[0] != image.shape[0] or t.shape[2:] != image.shape[2:]:
                raise ValueError(f"RMLineGenerator: {name} {tuple(t.shape)} does not match the image {tuple(image.shape)}")
            if torch.is_grad_enabled() and t.requires_grad:
                raise NotImplementedError("RMLineGenerator is inference only: detach the inputs or call it under torch.no_grad()")

    def run(self, image, mask=None, hull=None, dog=None, pad=True, lerp=False, fused=True, plan=0):
        """(out, mask, image3): the layers on image [N,3,H,W] ([N,4,H,W] with dog) — with `dog` (a dict of detector overrides) the mask
        comes from the line detector, else it is the caller's.  lerp: the wrapper's lerp(image, out, mask) in the last layer's store."""
        if dog is None and (self.gen_mask_input or lerp) and mask is None:
            raise ValueError("RMLineGenerator: a line_mask is needed")
        if self.gen_use_hull and hull is None:
            raise ValueError("RMLineGenerator: gen_use_hull wants a face_hull")
        pad = self.gen_depth if pad is True else (0 if pad is False else int(pad))
        with torch.no_grad():
            if fused:
                return ops.rmline_forward(self.program(plan), image, hull=hull, dog=dog, mask=mask, pad=pad, mask_input=self.gen_mask_input, lerp=lerp)
            if dog is not None:
                mask, image, _ = ops.rmline_mask(image, hull, dog)
            f = self.folded()
            stack = (image, mask if self.gen_mask_input else None, hull if self.gen_use_hull else None)
            x = None
            for i, (wk, b, act, slope) in enumerate(f):
                last = i == len(f) - 1
                x = ops.rmline_conv(x, wk, b, act, slope, stack=stack if i == 0 else None, pad=pad if i == 0 else 0, planar=last,
                                    lerp=(image, mask) if last and lerp else None, plan=plan)
            return x, mask, image

    def forward(self, x, pad=True, fused=True, plan=0):
        image, mask, hull = x["image"], x["line_mask"], x["face_hull"]
        self._check(image, mask, hull)
        out, _, _ = self.run(image.detach(), mask.detach() if mask is not None else None, hull.detach() if hull is not None else None,
                             pad=pad, fused=fused, plan=plan)
        return {"image": out, "line_mask": mask, "face_hull": hull}


# ---- the face hull ----------------------------------------------------------------------------------------------------------------------
def convex_hull_mask(points, size):
    """bool [H,W]: the pixels whose centres lie in the closed convex hull of integer `points` [(row, col)], by half-plane tests in exact
    integer arithmetic (a degenerate hull — one point, or collinear points — is the pixels ON the segment)."""
    H, W = size
    pts = sorted({(int(r), int(c)) for r, c in points})
    if not pts:
        return np.zeros((H, W), dtype=bool)

    def cross(o, a, b):
        return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])
    lower, upper = [], []
    for p in pts:  # Andrew's monotone chain
        while len(lower) >= 2 and cross(lower[-2], lower[-1], p) <= 0:
            lower.pop()
        lower.append(p)
    for p in reversed(pts):
        while len(upper) >= 2 and cross(upper[-2], upper[-1], p) <= 0:
            upper.pop()
        upper.append(p)
    hull = lower[:-1] + upper[:-1] if len(pts) > 1 else pts
    rr, cc = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    if len(hull) < 3:
        a, b = hull[0], hull[-1]
        on = (b[0] - a[0]) * (cc - a[1]) - (b[1] - a[1]) * (rr - a[0]) == 0
        return on & (rr >= min(a[0], b[0])) & (rr <= max(a[0], b[0])) & (cc >= min(a[1], b[1])) & (cc <= max(a[1], b[1]))
    inside = np.ones((H, W), dtype=bool)
    for a, b in zip(hull, hull[1:] + hull[:1]):
        inside &= (b[0] - a[0]) * (cc - a[1]) - (b[1] - a[1]) * (rr - a[0]) >= 0
    return inside


def face_hull(kpts, size, dilate=5):
    """The wrapper's face hull (rmline_wrapper.py:94-120) -> float32 [1,1,H,W] of 0 / 1, on the host.  kpts: [28, 2] (row, column) of the
    anime face detector's landmarks, truncated to integers as the reference does; size: (H, W) or one integer.  The convex hulls of the
    two eye groups and of the mouth, the nose pixel, the two eyelash polylines (one pixel wide, through PIL.ImageDraw as the reference's
    image class draws them), then a grey dilation by a flat dilate x dilate element (loss.dilation's restatement of kornia 0.6.5).

    The hulls restate skimage.morphology.convex_hull_image as half-plane tests at pixel centres (convex_hull_mask).  skimage cannot be
    imported here, so this is NOT pinned against it: skimage's default offsets every point by half a pixel before taking the hull, which
    can add boundary pixels that this helper leaves out."""
    from PIL import Image, ImageDraw
    from .loss import dilation
    H, W = (int(size), int(size)) if np.isscalar(size) else (int(size[0]), int(size[1]))
    kpts = np.asarray(kpts, dtype=np.float64)
    if kpts.ndim != 2 or kpts.shape[0] < 28 or kpts.shape[1] < 2:
        raise ValueError("face_hull: kpts is [28, 2] (row, column)")
    kpts = kpts[:, :2]
    ipts = kpts.astype(int)
    if (ipts < 0).any() or (ipts[:, 0] >= H).any() or (ipts[:, 1] >= W).any():
        raise ValueError("face_hull: a keypoint lies outside the image")
    v = np.zeros((H, W), dtype=bool)
    for grp in ("eye_right", "eye_left", "mouth"):
        v |= convex_hull_mask(ipts[KEYPOINT_GROUPS[grp]], (H, W))
    v[tuple(ipts[KEYPOINT_GROUPS["nose"][0]])] = True
    img = Image.fromarray(v.astype(np.uint8) * 255, mode="L")
    draw = ImageDraw.Draw(img)
    for grp in ("eyelash_left", "eyelash_right"):
        g = np.floor(kpts[KEYPOINT_GROUPS[grp]]).astype(int)
        for a, b in zip(g[:-1], g[1:]):
            draw.line([(int(a[1]), int(a[0])), (int(b[1]), int(b[0]))], fill=255, width=1)
    v = torch.from_numpy(np.asarray(img, dtype=np.uint8).copy() > 0).float()[None, None]
    return dilation(v, int(dilate)) if int(dilate) > 1 else v


_face_hull = face_hull  # (RMLineWrapper.forward has an argument of that name)


class RMLineWrapper(torch.nn.Module):
    """rmline_wrapper.py:10-50 on the HIP path.  forward(img, kpts=None, face_hull=None): img a float32 tensor [N,3|4,H,W] or [3|4,H,W]
    in [0, 1] -> the image with its lines removed, of the same shape and channel count (alpha passed through unchanged).  The hull comes
    from `kpts` ([28,2] landmarks, one face: rmline.face_hull) or is given as `face_hull` [N,1,H,W] / [1,H,W]; with neither it is empty.
    Detector + generator + lerp: gen_depth + 1 launches, one call into the library.

    The 8-bit PIL round trips of the reference's image class (`I(img)...`) stay with the caller: an image read from an 8-bit file is a
    fixed point of them.  model_or_path: an RMLineGenerator, or the path of a Lightning checkpoint (RMLineGenerator.from_checkpoint)."""

    DOG = dict(ops.RMLINE_DOG)

    def __init__(self, model_or_path=None, dog=None):
        super().__init__()
        if model_or_path is None:
            model_or_path = RMLineGenerator()
        self.model = model_or_path if isinstance(model_or_path, RMLineGenerator) else RMLineGenerator.from_checkpoint(model_or_path)
        self.dog = ops.rmline_dog_params(dict(self.DOG, **(dog or {})))
        super().train(False)

    def train(self, mode=True):
        if mode:
            raise NotImplementedError("RMLineWrapper is inference only")
        return super().train(False)

    def forward(self, img, kpts=None, face_hull=None, fused=True, plan=0, return_more=False):
        if not isinstance(img, torch.Tensor) or img.ndim not in (3, 4) or img.shape[-3] not in (3, 4):
            raise ValueError("RMLineWrapper: an image tensor [N,3|4,H,W] or [3|4,H,W]")
        if img.dtype != torch.float32:
            raise RuntimeError(f"img must be torch.float32, got {img.dtype}")
        if torch.is_grad_enabled() and img.requires_grad:
            raise NotImplementedError("RMLineWrapper is inference only: detach the image or call it under torch.no_grad()")
        if kpts is not None and face_hull is not None:
            raise ValueError("RMLineWrapper: kpts or face_hull, not both")
        batched = img.ndim == 4
        x = (img if batched else img[None]).detach().contiguous()
        N, Cc, H, W = x.shape
        dev = self.model.generator[0].weight.device
        if kpts is not None:
            if N != 1:
                raise ValueError("RMLineWrapper: kpts describe one face: one image")
            hull = _face_hull(kpts, (H, W))
        elif face_hull is not None:
            hull = face_hull if face_hull.ndim == 4 else face_hull[None]
            if tuple(hull.shape) != (N, 1, H, W):
                raise ValueError(f"RMLineWrapper: face_hull {tuple(face_hull.shape)}, expected {(N, 1, H, W)}")
        else:
            hull = torch.zeros((N, 1, H, W), dtype=torch.float32)
        hull = hull.to(device=dev, dtype=torch.float32).contiguous()
        out, mask, image = self.model.run(x.to(dev), None, hull, dog=self.dog, pad=True, lerp=True, fused=fused, plan=plan)
        ans = torch.cat([out, x[:, 3:].to(dev)], dim=1) if Cc == 4 else out
        ans = ans if batched else ans[0]
        return (ans, {"line_mask": mask, "face_hull": hull, "image": image}) if return_more else ans
