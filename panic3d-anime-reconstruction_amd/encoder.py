"""The conditioning encoder on the HIP operators of include/p3d_encoder.h: what the reference runs on every subject
before `G.f` (generate.py:68-92) to make `cond['resnet_chonk']`.

`ResnetFeatureExtractorPCA(fn_features, dim_out)` has the reference's constructor and call (katepca.py:9-30): the image is resized so
that its shorter side is 256, it and its mirror go through a ResNet-50 up to layer4 (katebackbone.py:103-121), and every pixel's 2048
features are projected by a fitted PCA, `pw @ (feat - mean)`: `[2, dim_out, h/32, w/32]`.  `ResNetEncoder` is that network: torchvision's
ResNet v1.5 bottleneck architecture under torchvision's `state_dict` names, in eval mode, its batch norms folded into the convolutions.
Inference only: the reference's trainer reads precomputed features and never differentiates the extractor.

Neither the tagger's checkpoint nor the fitted `pca.pkl` was available where this was written.  A freshly built model holds seeded
random weights: it is an encoder, not THE encoder, until `load_tagger` / `set_pca` (or `load_state_dict`) are given the real arrays.
Reading the real files (`fn_features` a path; `load_checkpoint`) is best-effort and UNCHECKED against them.
"""
import math

import torch

from . import memo, ops

STAGES = ("conv1", "layer1", "layer2", "layer3", "layer4")
MEAN = (0.485, 0.456, 0.406)  # katebackbone.py:31-34 (the tagger's resnet_preprocess is the same torchvision normalisation)
STD = (0.229, 0.224, 0.225)
BN_EPS = 1e-5


class _Conv(torch.nn.Module):
    def __init__(self, Ci, Co, k):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.randn(Co, Ci, k, k) * math.sqrt(2.0 / (Co * k * k)), requires_grad=False)  # (torchvision: fan_out)


class _BN(torch.nn.Module):
    def __init__(self, C):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.ones(C), requires_grad=False)
        self.bias = torch.nn.Parameter(torch.zeros(C), requires_grad=False)
        self.register_buffer("running_mean", torch.zeros(C))
        self.register_buffer("running_var", torch.ones(C))
        self.register_buffer("num_batches_tracked", torch.tensor(0, dtype=torch.long))


class _Linear(torch.nn.Module):
    def __init__(self, Ci, Co):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.randn(Co, Ci) / math.sqrt(Ci), requires_grad=False)
        self.bias = torch.nn.Parameter(torch.zeros(Co), requires_grad=False)


class Bottleneck(torch.nn.Module):
    """1 x 1 -> 3 x 3 (carries the stride: ResNet v1.5) -> 1 x 1, expansion 4; `downsample` = (1 x 1 convolution with the stride, BN)."""
    expansion = 4

    def __init__(self, Ci, width, stride, downsample):
        super().__init__()
        self.stride = stride
        self.conv1, self.bn1 = _Conv(Ci, width, 1), _BN(width)
        self.conv2, self.bn2 = _Conv(width, width, 3), _BN(width)
        self.conv3, self.bn3 = _Conv(width, width * 4, 1), _BN(width * 4)
        if downsample:
            self.downsample = torch.nn.Sequential(_Conv(Ci, width * 4, 1), _BN(width * 4))  # (containers of names only: never called)
        else:
            self.downsample = None


def fold_bn(conv_weight, bn, eps=BN_EPS):
    """Eval-mode batch norm folded into the convolution in float64, rounded once: (wk [k*k,Ci,Co], bias [Co]) in binary32 with
    wk = weight * gamma / sqrt(var + eps) (as weight.permute(2, 3, 1, 0)) and bias = beta - mean * gamma / sqrt(var + eps)."""
    w = conv_weight.detach().double()
    s = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + eps)
    Co, Ci, k, _ = w.shape
    wk = (w * s.view(-1, 1, 1, 1)).permute(2, 3, 1, 0).reshape(k * k, Ci, Co)
    b = bn.bias.detach().double() - bn.running_mean.detach().double() * s
    return wk.float().contiguous(), b.float().contiguous()


def fold_pca(components, mean):
    """pw @ (feat - mean) as a 1 x 1 convolution, in float64, rounded once: (wk [1,C,D], bias [D] = -pw mean)."""
    pw, m = components.detach().double(), mean.detach().double().reshape(-1)
    return pw.t().reshape(1, pw.shape[1], pw.shape[0]).float().contiguous(), (-(pw @ m)).float().contiguous()


class ResNetEncoder(torch.nn.Module):
    """torchvision's ResNet (v1.5 bottleneck) as a feature extractor on the HIP path.

    forward(x, size=256, features=('layer4',)) -> dict like the reference's `ans` (katebackbone.py:103-121): x [N,C>=3,H,W] float32 in
    [0, 1] is resized (shorter side `size`), normalised, and it and its mirror go through the network: every feature is [2N,C,h,w], rows
    N..2N-1 the mirrored image's.  Only the stages up to the last feature asked for are computed.  'pca' (after set_pca) is layer4
    projected.  fused=True walks the whole network in ONE call into the library; fused=False calls the operators layer by layer (the
    same kernels, the same bits).

    state_dict names are torchvision's: conv1.weight, bn1.*, layerL.B.conv{1,2,3}.weight, layerL.B.bn{1,2,3}.*,
    layerL.B.downsample.{0.weight,1.*}, and fc.* when num_classes is given (loaded, ignored by the feature path).  Every parameter has
    requires_grad=False.  Inference only."""

    def __init__(self, blocks=(3, 4, 6, 3), base_width=64, stem_width=64, num_classes=None):
        super().__init__()
        self.blocks, self.base_width, self.stem_width = tuple(int(b) for b in blocks), int(base_width), int(stem_width)
        if len(self.blocks) != 4 or min(self.blocks) < 1:
            raise ValueError("blocks: four positive counts")
        self.conv1, self.bn1 = _Conv(3, self.stem_width, 7), _BN(self.stem_width)
        Ci = self.stem_width
        for l, nb in enumerate(self.blocks):
            width, stride = self.base_width << l, 1 if l == 0 else 2
            layer = []
            for b in range(nb):
                s = stride if b == 0 else 1
                layer.append(Bottleneck(Ci, width, s, downsample=(b == 0 and (s != 1 or Ci != width * 4))))
                Ci = width * 4
            self.add_module(f"layer{l + 1}", torch.nn.Sequential(*layer))
        self.out_channels = Ci
        self.fc = _Linear(Ci, int(num_classes)) if num_classes is not None else None
        self.register_buffer("_mean", torch.tensor(MEAN, dtype=torch.float32), persistent=False)
        self.register_buffer("_std", torch.tensor(STD, dtype=torch.float32), persistent=False)
        self.register_parameter("pca_weights", None)
        self.register_parameter("pca_mean", None)
        self._folded, self._folded_key, self._programs = None, None, {}

    # ---- parameters ------------------------------------------------------------------------------------------------------------------
    def set_pca(self, components, mean):
        """components [D,C] (sklearn's pca.components_[:D]), mean [C] (pca.mean_): kept as the reference keeps them
        (katebackbone.py:78-79), pca_weights [1,D,C] and pca_mean [1,C]."""
        components, mean = torch.as_tensor(components, dtype=torch.float32), torch.as_tensor(mean, dtype=torch.float32)
        if components.ndim != 2 or components.shape[1] != self.out_channels or mean.numel() != self.out_channels:
            raise ValueError(f"set_pca: components [D,{self.out_channels}] and mean [{self.out_channels}]")
        dev = self.conv1.weight.device
        self.pca_weights = torch.nn.Parameter(components[None].to(dev).clone(), requires_grad=False)
        self.pca_mean = torch.nn.Parameter(mean.reshape(1, -1).to(dev).clone(), requires_grad=False)
        return self

    def blocks_of(self, l):
        return list(getattr(self, f"layer{l}"))

    def _sources(self):
        return [t for t in list(self.parameters()) + list(self.buffers()) if t.dtype.is_floating_point]

    def folded(self):
        """The operators' operands, derived from the parameters: per convolution (wk, bias) with the batch norm folded in float64 and
        rounded once; the PCA layer likewise.  Cached under memo's convention — identity and `_version` of every tensor they were derived
        from — so an in-place write (`copy_`, `load_state_dict`) re-derives them; memo.set_enabled(False) derives them on every call."""
        key = tuple((id(t), t._version, t.device) for t in self._sources())
        if self._folded is None or self._folded_key != key or not memo.enabled():
            f = {"conv1": fold_bn(self.conv1.weight, self.bn1)}
            for l in range(1, 5):
                for b, blk in enumerate(self.blocks_of(l)):
                    for j in (1, 2, 3):
                        f[f"layer{l}.{b}.conv{j}"] = fold_bn(getattr(blk, f"conv{j}").weight, getattr(blk, f"bn{j}"))
                    if blk.downsample is not None:
                        f[f"layer{l}.{b}.downsample"] = fold_bn(blk.downsample[0].weight, blk.downsample[1])
            if self.pca_weights is not None:
                f["pca"] = fold_pca(self.pca_weights[0], self.pca_mean)
            f["mean"], f["std"] = self._mean.detach().float().contiguous(), self._std.detach().float().contiguous()
            self._folded, self._folded_key, self._programs = f, key, {}
        return self._folded

    # ---- the network as a list of layer records ------------------------------------------------------------------------------------------
    def records(self, shape, size, features, plan=0):
        """(records, buf_len, outputs) for an input of `shape` = (N, C, H, W): the layer records of ops.EncoderProgram, the floats each
        arena buffer needs, and {feature: (buffer, shape)}.  Buffers: 0 the image, 1 the prepared batch, one per feature asked for,
        and five that the blocks rotate through (block input / output, the two inner activations, the downsampled identity)."""
        f = self.folded()
        N, C, H, W = (int(v) for v in shape)
        h, w = ops.enc_resize_hw(H, W, size)
        last = max(STAGES.index("layer4" if n == "pca" else n) for n in features)
        recs, buf_len, outputs = [], [N * C * H * W, 2 * N * 3 * h * w], {}

        def new_buf():
            buf_len.append(0)
            return len(buf_len) - 1
        feat_buf = {n: new_buf() for n in features}
        pool = [new_buf() for _ in range(5)]

        def emit(kind, src, dst, shape, out_shape, **kw):
            n_out = out_shape[0] * out_shape[1] * out_shape[2] * out_shape[3]
            buf_len[dst] = max(buf_len[dst], n_out)
            recs.append(dict(kind=kind, src=src, dst=dst, shape=tuple(shape), out_shape=tuple(out_shape), **kw))
            return out_shape

        def conv(name, src, dst, shape, k, stride, relu, res=None):
            wk, bias = f[name]
            Ho, Wo = ops._enc_out_hw(shape[2], shape[3], k, stride)
            return emit("conv", src, dst, shape, (shape[0], wk.shape[2], Ho, Wo), k=k, stride=stride, relu=relu, res=res, plan=plan, w=wk, b=bias, name=name)

        def free(*used):
            return next(b for b in pool if b not in used)
        cur_shape = emit("prepare", 0, 1, (N, C, H, W), (2 * N, 3, h, w), w=f["mean"], b=f["std"], name="prepare")
        cur = feat_buf.get("conv1", pool[0])
        cur_shape = conv("conv1", 1, cur, cur_shape, 7, 2, True)
        if "conv1" in features:
            outputs["conv1"] = (cur, cur_shape)
        if last >= 1:
            nxt = free(cur)
            cur_shape = emit("maxpool", cur, nxt, cur_shape, (cur_shape[0], cur_shape[1], (cur_shape[2] - 1) // 2 + 1, (cur_shape[3] - 1) // 2 + 1), name="maxpool")
            cur = nxt
        for l in range(1, last + 1):
            blks = self.blocks_of(l)
            for b, blk in enumerate(blks):
                pre = f"layer{l}.{b}"
                t1 = free(cur)
                s1 = conv(f"{pre}.conv1", cur, t1, cur_shape, 1, 1, True)
                t2 = free(cur, t1)
                s2 = conv(f"{pre}.conv2", t1, t2, s1, 3, blk.stride, True)
                idn = cur
                if blk.downsample is not None:
                    idn = free(cur, t1, t2)
                    conv(f"{pre}.downsample", cur, idn, cur_shape, 1, blk.stride, False)
                dst = feat_buf[f"layer{l}"] if (b == len(blks) - 1 and f"layer{l}" in features) else free(cur, t1, t2, idn)
                cur_shape = conv(f"{pre}.conv3", t2, dst, s2, 1, 1, True, res=idn)
                cur = dst
            if f"layer{l}" in features:
                outputs[f"layer{l}"] = (cur, cur_shape)
        if "pca" in features:
            outputs["pca"] = (feat_buf["pca"], conv("pca", cur, feat_buf["pca"], cur_shape, 1, 1, False))
        return recs, buf_len, outputs

    def program(self, shape, size=256, features=("layer4",), plan=0):
        """The ops.EncoderProgram of an input shape, cached with the folded operands."""
        f = self.folded()
        key = (tuple(int(v) for v in shape), int(size), tuple(features), int(plan), f["mean"].device)
        if key not in self._programs or not memo.enabled():
            recs, buf_len, outputs = self.records(shape, size, features, plan)
            self._programs[key] = (ops.EncoderProgram(recs, buf_len, f["mean"].device), outputs)
        return self._programs[key]

    def forward(self, x, size=256, features=("layer4",), fused=True, plan=0):
        if not isinstance(x, torch.Tensor) or x.ndim != 4 or x.shape[1] < 3:
            raise ValueError("ResNetEncoder: expected an image batch [N,C>=3,H,W]")
        if torch.is_grad_enabled() and x.requires_grad:
            raise NotImplementedError("ResNetEncoder is inference only (the reference never back-propagates into the extractor): "
                                      "detach the image or call it under torch.no_grad()")
        features = tuple(features)
        bad = [n for n in features if n not in STAGES + ("pca",)]
        if bad or not features:
            raise ValueError(f"features: some of {STAGES + ('pca',)}, got {features}")
        if "pca" in features and self.pca_weights is None:
            raise ValueError("features: 'pca' needs set_pca(components, mean) first")
        if x.dtype != torch.float32:
            raise RuntimeError(f"x must be torch.float32, got {x.dtype}")
        with torch.no_grad():
            x = x.detach().contiguous()
            if fused:
                prog, outputs = self.program(x.shape, size, features, plan)
                ops.encoder_forward(prog, x)
                return {n: prog.buffer(b, shp).clone() for n, (b, shp) in outputs.items()}
            recs, _, outputs = self.records(x.shape, size, features, plan)
            bufs = {0: x}
            for r in recs:
                src = bufs[r["src"]]
                if r["kind"] == "prepare":
                    y = ops._enc_prepare_impl(src, r["w"], r["b"], r["out_shape"][2], r["out_shape"][3])
                elif r["kind"] == "maxpool":
                    y = ops._enc_maxpool_impl(src)
                else:
                    y = ops._enc_conv_impl(src, r["w"], r["b"], r["k"], r["stride"], bufs[r["res"]] if r["res"] is not None else None, r["relu"], r["plan"])
                bufs[r["dst"]] = y
            return {n: bufs[b] for n, (b, _) in outputs.items()}


class ResnetFeatureExtractorPCA(torch.nn.Module):
    """katepca.py:9-30 on the HIP path.  forward(img) -> [2, dim_out, h/32, w/32] (row 0 the image, row 1 its mirror), what generate.py
    passes on as cond['resnet_chonk'] (`out[None, 0]`).  img: a [C,H,W] or [1,C,H,W] float32 tensor in [0, 1], or any object with
    `.bg('k').t()` (the reference's image class).  `rfe` is the ResNetEncoder; rfe.pca_weights [1,dim_out,2048] and rfe.pca_mean [1,2048]
    carry the reference's names.

    fn_features: None (set the arrays with set_pca), or the path of the pickled sklearn PCA — read best-effort with `pickle`, which was
    NOT checked against the real file (it was not available).  The projection is one more 1 x 1 convolution: weights pw, bias -pw mean,
    folded in float64."""

    def __init__(self, fn_features, dim_out, size=256, **encoder_options):
        super().__init__()
        self.fn_features, self.dim_out, self.size = fn_features, int(dim_out), int(size)
        self.rfe = ResNetEncoder(**encoder_options).eval()
        if fn_features is not None:
            import pickle
            with open(fn_features, "rb") as fh:  # unchecked: see the docstring
                pca = pickle.load(fh)
            self.set_pca(pca.components_, pca.mean_)

    def set_pca(self, components, mean):
        components = torch.as_tensor(components, dtype=torch.float32)
        if components.ndim != 2 or components.shape[0] < self.dim_out:
            raise ValueError(f"set_pca: at least {self.dim_out} components")
        self.rfe.set_pca(components[:self.dim_out], mean)
        return self

    def load_tagger(self, state_dict, prefix="resnet."):
        """Copy the network from the tagger's state dict (the Lightning checkpoint keeps it under `resnet.`, kate.py:25-26); other
        entries are ignored, missing ones raise.  Unchecked against the real checkpoint."""
        own = self.rfe.state_dict()
        sub = {k[len(prefix):]: v for k, v in state_dict.items() if k.startswith(prefix)}
        names = [k for k in own if not k.startswith("pca_")]
        missing = [k for k in names if k not in sub]
        if missing:
            raise KeyError(f"load_tagger: {len(missing)} entries missing under '{prefix}', the first: {missing[0]}")
        self.rfe.load_state_dict({k: sub[k] for k in names}, strict=False)
        return self

    def load_checkpoint(self, path):
        """The Lightning checkpoint's `state_dict` through load_tagger.  Best-effort and unchecked."""
        ck = torch.load(path, map_location="cpu")
        return self.load_tagger(ck.get("state_dict", ck))

    @staticmethod
    def _image(img):
        if not isinstance(img, torch.Tensor):
            img = img.bg("k").t()  # katepca.py:20
        if img.ndim == 3:
            img = img[None]
        if img.ndim != 4 or img.shape[0] != 1:
            raise ValueError("ResnetFeatureExtractorPCA: one image, [C,H,W] or [1,C,H,W]")
        return img

    def forward(self, img):
        if self.rfe.pca_weights is None:
            raise ValueError("ResnetFeatureExtractorPCA: no PCA yet: set_pca(components, mean)")
        img = self._image(img).to(self.rfe.pca_weights.device)
        return self.rfe(img, size=self.size, features=("pca",))["pca"]
