"""The dual discriminator of the adversarial phases (training/dual_discriminator.py: DualDiscriminator; training/networks_stylegan2.py:
Conv2dLayer :141-189, DiscriminatorBlock :759-840, MinibatchStdLayer :848-869, DiscriminatorEpilogue :877-930) on the HIP operators.

The classes keep the reference's names, constructor arguments, attribute names and state_dict keys, so `load_state_dict(...,
strict=True)` works in both directions and `c.D_kwargs.class_name` can name this module's DualDiscriminator.
Every convolution layer is ONE launch of ops.conv2d_act after its FIR (bias, lrelu, gain, clamp and the resnet block's residual add
in the convolution's store); the minibatch standard deviation is ops.minibatch_std; the two fully-connected layers of the epilogue
and the conditioning's mapping network are stylegan2.FullyConnectedLayer / MappingNetwork.  Under autograd each layer records a
first-order HIP backward; a double backward — the R1 penalty — raises, unless DualDiscriminator.set_r1_grad() has
switched on the recorded backward: then a backward under create_graph=True is differentiable once more, which is
what the loss's Dreg / Dboth phases need, and everything else — the forward, a plain backward — is unchanged.

Precision: `num_fp16_res`, `use_fp16` and `fp16_channels_last` are accepted and the network runs in binary32, as the reference does
on CPU and under force_fp32; `conv_clamp` is applied exactly as the reference applies it in fp32.
"""
import numpy as np
import torch

from . import memo, ops
from .stylegan2 import FullyConnectedLayer, MappingNetwork, _CacheFree


class Conv2dLayer(_CacheFree):
    def __init__(self, in_channels, out_channels, kernel_size, bias=True, activation="linear", up=1, down=1, resample_filter=[1, 3, 3, 1],
                 conv_clamp=None, channels_last=False, trainable=True):
        super().__init__()
        if up != 1 or down not in (1, 2) or kernel_size not in (1, 3):
            raise NotImplementedError("Conv2dLayer: the discriminator uses up=1, down 1 or 2 and 1x1 / 3x3 kernels (networks_stylegan2.py:797-808)")
        if activation not in ops._ACTS:
            raise NotImplementedError(f"activation {activation!r} is not used by the PAniC-3D discriminator")
        self.in_channels, self.out_channels, self.activation = in_channels, out_channels, activation
        self.up, self.down, self.conv_clamp = up, down, conv_clamp
        self.register_buffer("resample_filter", ops.setup_filter(resample_filter))
        self.padding = kernel_size // 2
        self.weight_gain = 1 / np.sqrt(in_channels * (kernel_size ** 2))
        self.act_gain = ops._ACTS[activation][2]
        weight = torch.randn([out_channels, in_channels, kernel_size, kernel_size])  # (channels_last: a memory format, binary32 runs contiguous)
        bias = torch.zeros([out_channels]) if bias else None
        if trainable:
            self.weight = torch.nn.Parameter(weight)
            self.bias = torch.nn.Parameter(bias) if bias is not None else None
        else:
            self.register_buffer("weight", weight)
            if bias is not None:
                self.register_buffer("bias", bias)
            else:
                self.bias = None
        self.r1_grad = False  # DualDiscriminator.set_r1_grad

    def _wk(self):
        """`weight * weight_gain` (networks_stylegan2.py:181) as the kernel's [taps][Ci][Co] operand.  No-grad: made once per parameter
        version, like FullyConnectedLayer._scaled.  Under autograd with a weight that requires grad: the same multiplication as a live
        op (same bits), so the raw parameter receives its gradient."""
        w = self.weight
        O, I, kh, kw = w.shape
        if torch.is_grad_enabled() and w.requires_grad:
            return (w * self.weight_gain).permute(2, 3, 1, 0).reshape(kh * kw, I, O).contiguous()
        key = (w.data_ptr(), w._version)
        if getattr(self, "_scaled_key", None) != key or not memo.enabled():
            self._scaled_wb = (w.detach() * self.weight_gain).permute(2, 3, 1, 0).reshape(kh * kw, I, O).contiguous()
            self._scaled_key = key
        return self._scaled_wb

    def forward(self, x, gain=1, res=None):
        """Conv2dLayer.forward (:180-189); `res` (not in the reference) is added to the result in the same launch: the `y.add_(x)` of
        the resnet block (:834).

        conv2d_resample.py's padding arithmetic for up = 1, restated: p = kernel_size // 2 on every side; with down = 2 and the 4-tap
        filter, p0 += (4 - 2 + 1) // 2 = 1 and p1 += (4 - 2) // 2 = 1.  3x3 (p = 2): upfirdn2d(x, f, padding 2) gives [H + 1]^2, then
        the correlation with stride 2 and no padding gives [H / 2]^2 (:"fast path: downsampling only").  1x1 (p = 1): upfirdn2d(x, f,
        down = 2, padding 1) gives [H / 2]^2, then the 1x1 correlation (:"fast path: 1x1 convolution with downsampling only").
        down = 1: the correlation with padding kernel_size // 2.  flip_weight is True (up == 1): the weights as they are."""
        k = self.weight.shape[-1]
        stride, pad = 1, self.padding
        if self.down == 2:
            f = self.resample_filter
            p = self.padding + (f.shape[-1] - self.down + 1) // 2, self.padding + (f.shape[-1] - self.down) // 2
            if k == 1:
                x = ops.fir(x, f, down=2, padding=[p[0], p[1], p[0], p[1]], r1=self.r1_grad)
            else:
                x = ops.fir(x, f, padding=[p[0], p[1], p[0], p[1]], r1=self.r1_grad)
                stride = 2
            pad = 0
        act_gain = self.act_gain * gain
        act_clamp = self.conv_clamp * gain if self.conv_clamp is not None else None
        return ops.conv2d_act(x, self._wk(), self.bias, act=self.activation, gain=act_gain, clamp=act_clamp, stride=stride, pad=pad, res=res,
                              r1=self.r1_grad)

    def extra_repr(self):
        return f"in_channels={self.in_channels:d}, out_channels={self.out_channels:d}, activation={self.activation:s}, up={self.up}, down={self.down}"


class DiscriminatorBlock(torch.nn.Module):
    def __init__(self, in_channels, tmp_channels, out_channels, resolution, img_channels, first_layer_idx, architecture="resnet",
                 activation="lrelu", resample_filter=[1, 3, 3, 1], conv_clamp=None, use_fp16=False, fp16_channels_last=False, freeze_layers=0):
        assert in_channels in [0, tmp_channels]
        assert architecture in ["orig", "skip", "resnet"]
        if architecture != "resnet":
            raise NotImplementedError(f"DiscriminatorBlock architecture {architecture!r} (networks_stylegan2.py:796-808, :822-837) is not "
                                      "used by PAniC-3D: only 'resnet' is implemented")
        super().__init__()
        self.in_channels, self.resolution, self.img_channels = in_channels, resolution, img_channels
        self.first_layer_idx, self.architecture = first_layer_idx, architecture
        self.use_fp16 = use_fp16  # accepted; the block runs in binary32 (module docstring)
        self.channels_last = (use_fp16 and fp16_channels_last)
        self.register_buffer("resample_filter", ops.setup_filter(resample_filter))
        self.num_layers = 0

        def trainable():  # networks_stylegan2.py:788-794
            layer_idx = self.first_layer_idx + self.num_layers
            self.num_layers += 1
            return layer_idx >= freeze_layers
        if in_channels == 0:
            self.fromrgb = Conv2dLayer(img_channels, tmp_channels, kernel_size=1, activation=activation, trainable=trainable(),
                                       conv_clamp=conv_clamp, channels_last=self.channels_last)
        self.conv0 = Conv2dLayer(tmp_channels, tmp_channels, kernel_size=3, activation=activation, trainable=trainable(),
                                 conv_clamp=conv_clamp, channels_last=self.channels_last)
        self.conv1 = Conv2dLayer(tmp_channels, out_channels, kernel_size=3, activation=activation, down=2, trainable=trainable(),
                                 resample_filter=resample_filter, conv_clamp=conv_clamp, channels_last=self.channels_last)
        self.skip = Conv2dLayer(tmp_channels, out_channels, kernel_size=1, bias=False, down=2, trainable=trainable(),
                                resample_filter=resample_filter, channels_last=self.channels_last)

    def forward(self, x, img, force_fp32=False):
        _ = force_fp32  # binary32 always
        if x is not None:
            assert tuple(x.shape[1:]) == (self.in_channels, self.resolution, self.resolution)
            x = x.to(torch.float32)
        if self.in_channels == 0:
            assert tuple(img.shape[1:]) == (self.img_channels, self.resolution, self.resolution)
            y = self.fromrgb(img.to(torch.float32))
            x = x + y if x is not None else y
            img = None
        y = self.skip(x, gain=np.sqrt(0.5))
        x = self.conv0(x)
        x = self.conv1(x, gain=np.sqrt(0.5), res=y)  # x = y.add_(x) (:834) in conv1's store
        return x, img

    def extra_repr(self):
        return f"resolution={self.resolution:d}, architecture={self.architecture:s}"


class MinibatchStdLayer(torch.nn.Module):
    def __init__(self, group_size, num_channels=1):
        super().__init__()
        self.group_size, self.num_channels = group_size, num_channels
        self.r1_grad = False  # DualDiscriminator.set_r1_grad

    def forward(self, x):
        return ops.minibatch_std(x, self.group_size, self.num_channels, r1=self.r1_grad)

    def extra_repr(self):
        return f"group_size={self.group_size}, num_channels={self.num_channels:d}"


class DiscriminatorEpilogue(torch.nn.Module):
    def __init__(self, in_channels, cmap_dim, resolution, img_channels, architecture="resnet", mbstd_group_size=4, mbstd_num_channels=1,
                 activation="lrelu", conv_clamp=None):
        assert architecture in ["orig", "skip", "resnet"]
        if architecture == "skip":
            raise NotImplementedError("DiscriminatorEpilogue architecture 'skip' (networks_stylegan2.py:897-898, :912-915) is not used by "
                                      "PAniC-3D: only 'resnet' is implemented")
        super().__init__()
        self.in_channels, self.cmap_dim, self.resolution = in_channels, cmap_dim, resolution
        self.img_channels, self.architecture = img_channels, architecture
        self.mbstd = MinibatchStdLayer(group_size=mbstd_group_size, num_channels=mbstd_num_channels) if mbstd_num_channels > 0 else None
        self.conv = Conv2dLayer(in_channels + mbstd_num_channels, in_channels, kernel_size=3, activation=activation, conv_clamp=conv_clamp)
        self.fc = FullyConnectedLayer(in_channels * (resolution ** 2), in_channels, activation=activation)
        self.out = FullyConnectedLayer(in_channels, 1 if cmap_dim == 0 else cmap_dim)

    def forward(self, x, img, cmap, force_fp32=False):
        _ = force_fp32, img
        assert tuple(x.shape[1:]) == (self.in_channels, self.resolution, self.resolution)
        x = x.to(torch.float32)
        if self.mbstd is not None:
            x = self.mbstd(x)
        x = self.conv(x)
        x = self.fc(x.flatten(1))
        x = self.out(x)
        if self.cmap_dim > 0:
            assert tuple(cmap.shape[1:]) == (self.cmap_dim,)
            x = (x * cmap).sum(dim=1, keepdim=True) * (1 / np.sqrt(self.cmap_dim))
        return x

    def extra_repr(self):
        return f"resolution={self.resolution:d}, architecture={self.architecture:s}"


def filtered_resizing(image_orig_tensor, size, f, filter_mode="antialiased", r1=False):
    """dual_discriminator.py:86-102.  The interpolations are torch's (plumbing); the 'classic' mode's two FIR passes are ops.fir (r1:
    differentiable to any order, DualDiscriminator.set_r1_grad)."""
    interp = torch.nn.functional.interpolate
    if filter_mode == "antialiased":
        return interp(image_orig_tensor, size=(size, size), mode="bilinear", align_corners=False, antialias=True)
    if filter_mode == "classic":
        fw = f.shape[-1]  # upsample2d (upfirdn2d.py:341-350): padding ((fw + 1) // 2, (fw - 2) // 2), gain 4
        y = ops.fir(image_orig_tensor, f, up=2, padding=[(fw + 1) // 2, (fw - 2) // 2] * 2, gain=4, r1=r1)
        y = interp(y, size=(size * 2 + 2, size * 2 + 2), mode="bilinear", align_corners=False)
        p = [-1 + (fw - 2 + 1) // 2, -1 + (fw - 2) // 2] * 2  # downsample2d (upfirdn2d.py:378-387) with padding -1
        return ops.fir(y.contiguous(), f, down=2, padding=p, flip_filter=True, r1=r1)
    if filter_mode == "none":
        return interp(image_orig_tensor, size=(size, size), mode="bilinear", align_corners=False)
    if type(filter_mode) == float:
        assert 0 < filter_mode < 1
        filtered = interp(image_orig_tensor, size=(size, size), mode="bilinear", align_corners=False, antialias=True)
        aliased = interp(image_orig_tensor, size=(size, size), mode="bilinear", align_corners=False, antialias=False)
        return (1 - filter_mode) * aliased + filter_mode * filtered
    raise ValueError(f"filter_mode {filter_mode!r}")


class DualDiscriminator(torch.nn.Module):
    def __init__(self, c_dim, img_resolution, img_channels, cond_mode, architecture="resnet", channel_base=32768, channel_max=512,
                 num_fp16_res=4, conv_clamp=256, cmap_dim=None, disc_c_noise=0, block_kwargs={}, mapping_kwargs={}, epilogue_kwargs={}):
        super().__init__()
        img_channels *= 2
        self.cond_mode, self.c_dim, self.img_resolution = cond_mode, c_dim, img_resolution
        self.img_resolution_log2 = int(np.log2(img_resolution))
        self.img_channels = img_channels
        self.block_resolutions = [2 ** i for i in range(self.img_resolution_log2, 2, -1)]
        channels_dict = {res: min(channel_base // res, channel_max) for res in self.block_resolutions + [4]}
        fp16_resolution = max(2 ** (self.img_resolution_log2 + 1 - num_fp16_res), 8)
        if cmap_dim is None:
            cmap_dim = channels_dict[4]
        if c_dim == 0:
            cmap_dim = 0
        common_kwargs = dict(img_channels=img_channels, architecture=architecture, conv_clamp=conv_clamp)
        cur_layer_idx = 0
        for res in self.block_resolutions:
            in_channels = channels_dict[res] if res < img_resolution else 0
            block = DiscriminatorBlock(in_channels, channels_dict[res], channels_dict[res // 2], resolution=res, first_layer_idx=cur_layer_idx,
                                       use_fp16=(res >= fp16_resolution), **block_kwargs, **common_kwargs)
            setattr(self, f"b{res}", block)
            cur_layer_idx += block.num_layers
        if c_dim > 0:
            self.mapping = MappingNetwork(z_dim=0, c_dim=c_dim, w_dim=cmap_dim, num_ws=None, w_avg_beta=None, cond_mode=cond_mode, **mapping_kwargs)
        self.b4 = DiscriminatorEpilogue(channels_dict[4], cmap_dim=cmap_dim, resolution=4, **epilogue_kwargs, **common_kwargs)
        self.register_buffer("resample_filter", ops.setup_filter([1, 3, 3, 1]))
        self.disc_c_noise = disc_c_noise
        self.r1_grad = False

    def set_r1_grad(self, state=True):
        """Opt-in: let a backward that autograd records (torch.autograd.grad(..., create_graph=True), the R1 penalty of the loss's Dreg /
        Dboth phases) be differentiated once more.  With the switch on, every convolution layer, the minibatch standard
        deviation, the FIR passes and the epilogue's activated fully-connected layer record their first backward through Functions
        whose own backward is HIP (include/p3d_r1.h); the gradients of that first backward are the plain backward's bits.  The forward
        and a plain backward are today's in either state.  Off (the default): such a backward raises ops.R1_MESSAGE."""
        state = bool(state)
        self.r1_grad = state
        for m in self.modules():
            if isinstance(m, (Conv2dLayer, MinibatchStdLayer)):
                m.r1_grad = state
        self.b4.fc.r1_grad = state
        return state

    def forward(self, img, c, cond, update_emas=False, **block_kwargs):
        image_raw = filtered_resizing(img["image_raw"], size=img["image"].shape[-1], f=self.resample_filter, r1=self.r1_grad)
        img = torch.cat([img["image"], image_raw], 1)
        _ = update_emas  # unused (dual_discriminator.py:162)
        x = None
        for res in self.block_resolutions:
            x, img = getattr(self, f"b{res}")(x, img, **block_kwargs)
        cmap = None
        if self.c_dim > 0:
            if self.disc_c_noise > 0:
                c += torch.randn_like(c) * c.std(0) * self.disc_c_noise  # in place, as the reference does (:170)
            cmap = self.mapping(None, c, cond)
        return self.b4(x, img, cmap)

    def extra_repr(self):
        return f"c_dim={self.c_dim:d}, img_resolution={self.img_resolution:d}, img_channels={self.img_channels:d}"
