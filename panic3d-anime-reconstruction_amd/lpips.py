"""LPIPS, the AlexNet perceptual distance, on the HIP operators of include/p3d_lpips.h.

The reference's trainer builds its perceptual model as `utorch.LPIPSLoss()` (training_loop_v0.py:168; _util/pytorch_v1.py:159-168):
`lpips.LPIPS(net='alex')` — version 0.1, lpips=True, spatial=False — followed by `.mean((1, 2, 3))`.  `LPIPS` and `LPIPSLoss` here have
that call surface; `StyleGAN2LossOrthoCondA(lpips_model=LPIPSLoss())` works as it is.

Neither the `lpips` package nor its weights were available where this was written.  The arithmetic is the one include/p3d_lpips.h
writes out; the parameter and buffer names below are the names the package uses AS FAR AS THEY ARE KNOWN HERE and could not be checked
against it: load a state dict of `lpips.LPIPS` with `strict=False` and look at what `load_state_dict` reports.  A freshly built model
holds random weights (He-scaled, drawn from torch's global generator): it is a distance, not THE distance, until the released
weights are loaded.
"""
import math

import torch

from . import memo, ops

ALEX_LAYERS = ((11, 4, 2, True), (5, 1, 2, True), (3, 1, 1, False), (3, 1, 1, False), (3, 1, 1, False))  # (k, stride, pad, pool after it)
ALEX_CHANNELS = (64, 192, 384, 256, 256)
ALEX_INDEX = (0, 3, 6, 8, 10)  # the convolutions' places in torchvision's alexnet().features, which the package's slices keep
SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)


class ScalingLayer(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer("shift", torch.tensor(SHIFT, dtype=torch.float32).view(1, 3, 1, 1))
        self.register_buffer("scale", torch.tensor(SCALE, dtype=torch.float32).view(1, 3, 1, 1))


class _Conv(torch.nn.Module):
    """The parameters of one convolution, in torch's layout: weight [Co,Ci,k,k], bias [Co]."""

    def __init__(self, Ci, Co, k):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.randn(Co, Ci, k, k) * math.sqrt(2.0 / (Ci * k * k)), requires_grad=False)
        self.bias = torch.nn.Parameter(torch.zeros(Co), requires_grad=False)


class _Lin(torch.nn.Module):
    """NetLinLayer's parameters: model.1.weight [1,C,1,1] (model.0 is the package's dropout: no parameters, off in eval)."""

    def __init__(self, C):
        super().__init__()
        self.model = torch.nn.Module()
        one = torch.nn.Module()
        one.weight = torch.nn.Parameter(torch.rand(1, C, 1, 1) / C, requires_grad=False)
        self.model.add_module("1", one)

    @property
    def weight(self):
        return getattr(self.model, "1").weight


class LPIPS(torch.nn.Module):
    """lpips.LPIPS(net='alex') on the HIP path.  forward(in0, in1, normalize=False) -> [N,1,1,1]; in0 may carry a gradient (first
    order), in1 is the target.  Images are [N,3,H,W] float32 in [-1, 1] (normalize=True: in [0, 1]), H, W >= 31.

    state_dict names (unchecked against the package, see the module's docstring): scaling_layer.shift / .scale [1,3,1,1];
    net.slice{1..5}.{0,3,6,8,10}.weight / .bias; lin{0..4}.model.1.weight [1,C,1,1].  Every parameter has requires_grad=False and never
    receives a gradient.  `channels` other than AlexNet's serve the tests."""

    def __init__(self, net="alex", channels=ALEX_CHANNELS, version="0.1", lpips=True, spatial=False, **package_options):
        """package_options: the package's remaining constructor options (pretrained, model_path, use_dropout, eval_mode, verbose, ...),
        accepted and ignored: nothing is downloaded or loaded here, and there is no dropout."""
        super().__init__()
        if (str(version), bool(lpips), bool(spatial)) != ("0.1", True, False):
            raise NotImplementedError("LPIPS: only version '0.1' with lpips=True, spatial=False (the reference's defaults) is implemented")
        if net != "alex":
            raise NotImplementedError(f"LPIPS(net={net!r}): the reference's trainer builds the default, 'alex' (training_loop_v0.py:168); "
                                      "the 'vgg' and 'squeeze' trunks are not ported")
        if len(channels) != len(ALEX_LAYERS):
            raise ValueError(f"channels: {len(ALEX_LAYERS)} widths")
        self.channels = tuple(int(c) for c in channels)
        self.scaling_layer = ScalingLayer()
        self.net = torch.nn.Module()
        Ci = 3
        for i, ((k, _, _, _), Co) in enumerate(zip(ALEX_LAYERS, self.channels)):
            s = torch.nn.Module()
            s.add_module(str(ALEX_INDEX[i]), _Conv(Ci, Co, k))
            self.net.add_module(f"slice{i + 1}", s)
            self.add_module(f"lin{i}", _Lin(Co))
            Ci = Co
        self._operands, self._operands_key = None, None

    def convs(self):
        return [getattr(getattr(self.net, f"slice{i + 1}"), str(ALEX_INDEX[i])) for i in range(len(ALEX_LAYERS))]

    def lins(self):
        return [getattr(self, f"lin{i}") for i in range(len(ALEX_LAYERS))]

    def load_torchvision_alexnet(self, state_dict):
        """Copy the trunk from a torchvision `alexnet()` state dict (`features.{0,3,6,8,10}.weight / .bias`); the lin layers and the
        scaling layer are not part of it.  Also accepts the package's own names, with or without the `net.` prefix."""
        for i, conv in enumerate(self.convs()):
            idx = ALEX_INDEX[i]
            for leaf in ("weight", "bias"):
                names = (f"features.{idx}.{leaf}", f"net.slice{i + 1}.{idx}.{leaf}", f"slice{i + 1}.{idx}.{leaf}")
                found = [n for n in names if n in state_dict]
                if not found:
                    raise KeyError(f"none of {names} in the state dict")
                with torch.no_grad():
                    getattr(conv, leaf).copy_(state_dict[found[0]])
        return self

    def operands(self):
        """The operators' operands, derived from the parameters: per layer wk [k*k,Ci,Co], bias, the backward's weights (flipped and
        transposed for a stride-1 layer; the stem's backward reads wk), lin [C]; shift, scale [3].  Cached under memo's convention —
        the identity and `_version` of every tensor they were derived from — so an in-place write (`copy_`, `load_state_dict`)
        re-derives them; memo.set_enabled(False) derives them on every call."""
        src = [self.scaling_layer.shift, self.scaling_layer.scale] + [t for c in self.convs() for t in (c.weight, c.bias)] + [l.weight for l in self.lins()]
        key = tuple((id(t), t._version, t.device) for t in src)
        if self._operands is None or self._operands_key != key or not memo.enabled():
            layers = []
            for (k, stride, pad, pool), conv, lin in zip(ALEX_LAYERS, self.convs(), self.lins()):
                w = conv.weight.detach().float()
                Co, Ci = w.shape[:2]
                wk = w.permute(2, 3, 1, 0).reshape(k * k, Ci, Co).contiguous()
                wkb = ops.lpips_backward_weights(wk) if stride == 1 else wk
                layers.append((wk, conv.bias.detach().float().contiguous(), wkb, lin.weight.detach().float().reshape(-1).contiguous(), k, stride, pad, pool))
            self._operands = dict(shift=self.scaling_layer.shift.detach().float().reshape(-1).contiguous(),
                                  scale=self.scaling_layer.scale.detach().float().reshape(-1).contiguous(), layers=layers)
            self._operands_key = key
        return self._operands

    def forward(self, in0, in1, normalize=False):
        if normalize:  # [0, 1] -> [-1, 1]
            in0, in1 = 2 * in0 - 1, 2 * in1 - 1
        return ops.lpips_distance(in0, in1, self.operands())


class LPIPSLoss(torch.nn.Module):
    """_util/pytorch_v1.py:159-168: `.model` is the LPIPS network, forward(preds, target) -> [N]."""

    def __init__(self, net_type="alex", **kwargs):
        super().__init__()
        self.net_type = net_type
        self.model = LPIPS(net=self.net_type, **kwargs)

    def forward(self, preds, target):
        return self.model(preds, target).mean((1, 2, 3))
