"""The augmentation pipe of "Training Generative Adversarial Networks with Limited Data" as the reference's trainer uses it
(training/augment.py:123-439, training_loop_v0.py:193-202, :399-402): AugmentPipe with the reference's constructor, buffers and
forward(images, debug_percentile=None), and the ADA controller (ada_update, AdaStats).  DESIGN.md §4.22.

The parameters of a call are drawn on the HOST with the reference's own torch calls, shapes and dtypes in the reference's order, and
composed there in float64 (AugmentPipe.draw); the image runs through two HIP operators, ops.augment_apply (geometry and colour, §4.20)
and ops.augment_tail (filter, noise, cutout).  Nothing is read back from the device in the steady state: the reference reads its
margins back on every call; here they are computed where the matrices are.
"""
import collections

import numpy as np
import torch

from . import ops

SIGNS_REAL = "Loss/signs/real"

AugmentDraw = collections.namedtuple("AugmentDraw", "G_inv margins C taps sigma rect")
AugmentDraw.__doc__ = """One call's parameters, all on the host: G_inv [N, 3, 3] float32 or None, margins (mx0, my0, mx1, my1) (zeros
without G_inv), C [N, 4, 4] float32 or None, taps [N, 43] float32 or None, sigma [N] float32 or None, rect [N, 4] int32
= (x0, x1, y0, y1) or None."""


def fbank():
    """Hz_fbank [4, 43] float64, derived (augment.py:177-186 without scipy): the order-2 Daubechies low-pass in closed form, then the
    reference's construction with np.convolve per row.  Equal to the reference's buffer to the bit on every tap that is not
    mathematically zero; those hold float64 cancellation residue (below 1e-12) in both."""
    s3 = np.sqrt(3.0)
    lo = (np.array([1 + s3, 3 + s3, 3 - s3, 1 - s3]) / (4 * np.sqrt(2.0)))[::-1]
    hi = lo * ((-1) ** np.arange(lo.size))
    lo2, hi2 = np.convolve(lo, lo[::-1]) / 2, np.convolve(hi, hi[::-1]) / 2
    bank = np.eye(4, 1)
    for i in range(1, bank.shape[0]):
        bank = np.dstack([bank, np.zeros_like(bank)]).reshape(bank.shape[0], -1)[:, :-1]
        bank = np.stack([np.convolve(row, lo2) for row in bank])
        bank[i, (bank.shape[1] - hi2.size) // 2: (bank.shape[1] + hi2.size) // 2] += hi2
    return bank


def _translate2d(tx, ty):
    M = np.tile(np.eye(3), (len(tx), 1, 1))
    M[:, 0, 2], M[:, 1, 2] = tx, ty
    return M


def _scale2d(sx, sy):
    M = np.tile(np.eye(3), (len(sx), 1, 1))
    M[:, 0, 0], M[:, 1, 1] = sx, sy
    return M


def _rotate2d(theta):
    M = np.tile(np.eye(3), (len(theta), 1, 1))
    M[:, 0, 0], M[:, 0, 1], M[:, 1, 0], M[:, 1, 1] = np.cos(theta), np.sin(-theta), np.sin(theta), np.cos(theta)
    return M


def _rotate3d(v, theta):
    vx, vy, vz = v[:3]
    s, c = np.sin(theta), np.cos(theta)
    cc = 1 - c
    M = np.tile(np.eye(4), (len(theta), 1, 1))
    M[:, 0, :3] = np.stack([vx * vx * cc + c, vx * vy * cc - vz * s, vx * vz * cc + vy * s], axis=-1)
    M[:, 1, :3] = np.stack([vy * vx * cc + vz * s, vy * vy * cc + c, vy * vz * cc - vx * s], axis=-1)
    M[:, 2, :3] = np.stack([vz * vx * cc - vy * s, vz * vy * cc + vx * s, vz * vz * cc + c], axis=-1)
    return M


def _matrix32(*rows):
    """[N, rows, cols] float32 from rows of [N] tensors and constants: the reference's own float32 matrices, for the margins."""
    ref = [x for row in rows for x in row if isinstance(x, torch.Tensor)][0]
    elems = [x if isinstance(x, torch.Tensor) else torch.full_like(ref, float(x)) for row in rows for x in row]
    return torch.stack(elems, dim=-1).reshape(ref.shape + (len(rows), -1))


def _scale32(sx, sy):
    return _matrix32([sx, 0, 0], [0, sy, 0], [0, 0, 1])


def _rotate32(theta):
    return _matrix32([torch.cos(theta), torch.sin(-theta), 0], [torch.sin(theta), torch.cos(theta), 0], [0, 0, 1])


def _translate32(tx, ty):
    return _matrix32([1, 0, tx], [0, 1, ty], [0, 0, 1])


def _f64(t):
    return t.reshape(t.shape[0], -1).numpy().astype(np.float64)


class AugmentPipe(torch.nn.Module):
    """The reference's AugmentPipe: all augmentations are disabled by default; each is enabled by its probability multiplier.

    One stream cannot follow the reference's: the noise field is drawn on the device (torch.randn(images.shape, device=...,
    generator=noise_generator)), where the reference on a CPU device draws it from the host stream between the noise's and the
    cutout's parameters.  With noise > 0 the cutout draws that follow therefore differ from the reference's under the same seed;
    every other parameter equals the reference's own CPU run after torch.manual_seed(s)."""

    def __init__(self,
                 xflip=0, rotate90=0, xint=0, xint_max=0.125,
                 scale=0, rotate=0, aniso=0, xfrac=0, scale_std=0.2, rotate_max=1, aniso_std=0.2, xfrac_std=0.125,
                 brightness=0, contrast=0, lumaflip=0, hue=0, saturation=0, brightness_std=0.2, contrast_std=0.5, hue_max=1, saturation_std=1,
                 imgfilter=0, imgfilter_bands=[1, 1, 1, 1], imgfilter_std=1,
                 noise=0, cutout=0, noise_std=0.1, cutout_size=0.5):
        super().__init__()
        self.register_buffer("p", torch.ones([]))  # overall multiplier for augmentation probability
        self.xflip, self.rotate90, self.xint, self.xint_max = float(xflip), float(rotate90), float(xint), float(xint_max)
        self.scale, self.rotate, self.aniso, self.xfrac = float(scale), float(rotate), float(aniso), float(xfrac)
        self.scale_std, self.rotate_max, self.aniso_std, self.xfrac_std = float(scale_std), float(rotate_max), float(aniso_std), float(xfrac_std)
        self.brightness, self.contrast, self.lumaflip, self.hue, self.saturation = float(brightness), float(contrast), float(lumaflip), float(hue), float(saturation)
        self.brightness_std, self.contrast_std, self.hue_max, self.saturation_std = float(brightness_std), float(contrast_std), float(hue_max), float(saturation_std)
        self.imgfilter, self.imgfilter_bands, self.imgfilter_std = float(imgfilter), list(imgfilter_bands), float(imgfilter_std)
        self.noise, self.cutout, self.noise_std, self.cutout_size = float(noise), float(cutout), float(noise_std), float(cutout_size)
        self.register_buffer("Hz_geom", torch.from_numpy(ops.augment_filter_tables()[0].copy()))
        self.register_buffer("Hz_fbank", torch.as_tensor(fbank(), dtype=torch.float32))
        self._fbank_host = self.Hz_fbank.numpy().astype(np.float64)  # what draw() multiplies by: the buffer's float32 values
        self._p_host, self._p_ref, self._p_version = None, None, None
        self.noise_generator = None  # an optional device generator for the noise field

    # ---- p: a buffer (the training loop writes augment_pipe.p.copy_(...)) with a host mirror -----------------------------------------------
    def _read_p(self):
        """The only place that reads p's value: one device-to-host copy, after which the mirror holds while p is the same tensor with
        the same version counter."""
        self._p_host, self._p_ref, self._p_version = float(self.p.detach().cpu()), self.p, self.p._version
        return self._p_host

    def p_host(self):
        if self._p_ref is not self.p or self._p_version != self.p._version:
            self._read_p()
        return self._p_host

    def set_p(self, value):
        """Writes the buffer and the mirror together (ada_update)."""
        value = float(np.float32(value))
        self.p.fill_(value)
        self._p_host, self._p_ref, self._p_version = value, self.p, self.p._version

    # ---- the draws --------------------------------------------------------------------------------------------------------------------------
    def draw(self, batch, num_channels, height, width, debug_percentile=None, generator=None):
        """-> AugmentDraw.  Every random number is formed as the reference forms it on a CPU device (the same torch calls, shapes and
        float32 comparisons, in its order); the matrices, margins, band gains and filter rows are composed in float64 from those
        float32 parameters and rounded once."""
        N = int(batch)
        p = torch.tensor(self.p_host(), dtype=torch.float32)
        rand = lambda *shape: torch.rand(list(shape), generator=generator)
        randn = lambda *shape: torch.randn(list(shape), generator=generator)
        q = None if debug_percentile is None else torch.as_tensor(debug_percentile, dtype=torch.float32, device="cpu")
        enabled_geo = any(v > 0 for v in (self.xflip, self.rotate90, self.xint, self.scale, self.rotate, self.aniso, self.xfrac))
        G = np.tile(np.eye(3), (N, 1, 1))
        G32 = torch.eye(3)  # the same chain as the reference forms it, in float32: only the margins are taken from it (a ceil)
        if self.xflip > 0:
            i = torch.floor(rand(N) * 2)
            i = torch.where(rand(N) < self.xflip * p, i, torch.zeros_like(i))
            if q is not None:
                i = torch.full_like(i, torch.floor(q * 2))
            G = G @ _scale2d(1 / _f64(1 - 2 * i)[:, 0], np.ones(N))
            G32 = G32 @ _scale32(1 / (1 - 2 * i), 1.0)
        if self.rotate90 > 0:
            i = torch.floor(rand(N) * 4)
            i = torch.where(rand(N) < self.rotate90 * p, i, torch.zeros_like(i))
            if q is not None:
                i = torch.full_like(i, torch.floor(q * 4))
            G = G @ _rotate2d(-_f64(-np.pi / 2 * i)[:, 0])
            G32 = G32 @ _rotate32(-(-np.pi / 2 * i))
        if self.xint > 0:
            t = (rand(N, 2) * 2 - 1) * self.xint_max
            t = torch.where(rand(N, 1) < self.xint * p, t, torch.zeros_like(t))
            if q is not None:
                t = torch.full_like(t, (q * 2 - 1) * self.xint_max)
            G = G @ _translate2d(-_f64(torch.round(t[:, 0] * width))[:, 0], -_f64(torch.round(t[:, 1] * height))[:, 0])
            G32 = G32 @ _translate32(-torch.round(t[:, 0] * width), -torch.round(t[:, 1] * height))
        if self.scale > 0:
            s = torch.exp2(randn(N) * self.scale_std)
            s = torch.where(rand(N) < self.scale * p, s, torch.ones_like(s))
            if q is not None:
                s = torch.full_like(s, torch.exp2(torch.erfinv(q * 2 - 1) * self.scale_std))
            G32 = G32 @ _scale32(1 / s, 1 / s)
            s = _f64(s)[:, 0]
            G = G @ _scale2d(1 / s, 1 / s)
        p_rot = 1 - torch.sqrt((1 - self.rotate * p).clamp(0, 1))  # P(pre OR post) = p
        if self.rotate > 0:
            theta = (rand(N) * 2 - 1) * np.pi * self.rotate_max
            theta = torch.where(rand(N) < p_rot, theta, torch.zeros_like(theta))
            if q is not None:
                theta = torch.full_like(theta, (q * 2 - 1) * np.pi * self.rotate_max)
            G = G @ _rotate2d(-_f64(-theta)[:, 0])  # before anisotropic scaling
            G32 = G32 @ _rotate32(-(-theta))
        if self.aniso > 0:
            s = torch.exp2(randn(N) * self.aniso_std)
            s = torch.where(rand(N) < self.aniso * p, s, torch.ones_like(s))
            if q is not None:
                s = torch.full_like(s, torch.exp2(torch.erfinv(q * 2 - 1) * self.aniso_std))
            G32 = G32 @ _scale32(1 / s, 1 / (1 / s))
            s = _f64(s)[:, 0]
            G = G @ _scale2d(1 / s, s)
        if self.rotate > 0:
            theta = (rand(N) * 2 - 1) * np.pi * self.rotate_max
            theta = torch.where(rand(N) < p_rot, theta, torch.zeros_like(theta))
            if q is not None:
                theta = torch.zeros_like(theta)
            G = G @ _rotate2d(-_f64(-theta)[:, 0])  # after anisotropic scaling
            G32 = G32 @ _rotate32(-(-theta))
        if self.xfrac > 0:
            t = randn(N, 2) * self.xfrac_std
            t = torch.where(rand(N, 1) < self.xfrac * p, t, torch.zeros_like(t))
            if q is not None:
                t = torch.full_like(t, torch.erfinv(q * 2 - 1) * self.xfrac_std)
            G = G @ _translate2d(-_f64(t[:, 0] * width)[:, 0], -_f64(t[:, 1] * height)[:, 0])
            G32 = G32 @ _translate32(-(t[:, 0] * width), -(t[:, 1] * height))
        G_inv, margins = None, (0, 0, 0, 0)
        if enabled_geo:
            # the margins are a ceil: taken from the float32 chain with the reference's own operations (augment.py:280-290), so that
            # they equal the reference's where a lattice transform puts the corner reach on an integer up to float32 rounding
            cx, cy = (width - 1) / 2, (height - 1) / 2
            const = lambda v: torch.as_tensor(np.asarray(v), dtype=torch.float32)
            cp = G32 @ const([[-cx, -cy, 1], [cx, -cy, 1], [cx, cy, 1], [-cx, cy, 1]]).t()  # [batch, xyz, idx]
            hz_pad = self.Hz_geom.shape[0] // 4
            m = cp[:, :2, :].permute(1, 0, 2).flatten(1)
            m = torch.cat([-m, m]).max(dim=1).values  # x0, y0, x1, y1
            m = m + const([hz_pad * 2 - cx, hz_pad * 2 - cy] * 2)
            m = m.max(const([0, 0] * 2)).min(const([width - 1, height - 1] * 2))
            margins = tuple(int(v) for v in m.ceil().to(torch.int32))
            G_inv = G.astype(np.float32)

        # colour
        enabled_col = any(v > 0 for v in (self.brightness, self.contrast, self.lumaflip)) or (num_channels > 1 and (self.hue > 0 or self.saturation > 0))
        Cm = np.tile(np.eye(4), (N, 1, 1))
        v = np.array([1, 1, 1, 0]) / np.sqrt(3)  # the luma axis
        vv = np.outer(v, v)
        if self.brightness > 0:
            b = randn(N) * self.brightness_std
            b = torch.where(rand(N) < self.brightness * p, b, torch.zeros_like(b))
            if q is not None:
                b = torch.full_like(b, torch.erfinv(q * 2 - 1) * self.brightness_std)
            T = np.tile(np.eye(4), (N, 1, 1))
            T[:, :3, 3] = _f64(b)
            Cm = T @ Cm
        if self.contrast > 0:
            c = torch.exp2(randn(N) * self.contrast_std)
            c = torch.where(rand(N) < self.contrast * p, c, torch.ones_like(c))
            if q is not None:
                c = torch.full_like(c, torch.exp2(torch.erfinv(q * 2 - 1) * self.contrast_std))
            S = np.tile(np.eye(4), (N, 1, 1))
            S[:, 0, 0] = S[:, 1, 1] = S[:, 2, 2] = _f64(c)[:, 0]
            Cm = S @ Cm
        if self.lumaflip > 0:
            i = torch.floor(rand(N, 1, 1) * 2)
            i = torch.where(rand(N, 1, 1) < self.lumaflip * p, i, torch.zeros_like(i))
            if q is not None:
                i = torch.full_like(i, torch.floor(q * 2))
            Cm = (np.eye(4) - 2 * vv * _f64(i)[:, :, None]) @ Cm  # Householder reflection
        if self.hue > 0 and num_channels > 1:
            theta = (rand(N) * 2 - 1) * np.pi * self.hue_max
            theta = torch.where(rand(N) < self.hue * p, theta, torch.zeros_like(theta))
            if q is not None:
                theta = torch.full_like(theta, (q * 2 - 1) * np.pi * self.hue_max)
            Cm = _rotate3d(v, _f64(theta)[:, 0]) @ Cm
        if self.saturation > 0 and num_channels > 1:
            s = torch.exp2(randn(N, 1, 1) * self.saturation_std)
            s = torch.where(rand(N, 1, 1) < self.saturation * p, s, torch.ones_like(s))
            if q is not None:
                s = torch.full_like(s, torch.exp2(torch.erfinv(q * 2 - 1) * self.saturation_std))
            Cm = (vv + (np.eye(4) - vv) * _f64(s)[:, :, None]) @ Cm
        if enabled_col and num_channels not in (1, 3, 6):
            raise ValueError("Image must be RGB (3 channels) or L (1 channel)")
        C = Cm.astype(np.float32) if enabled_col else None

        # filter
        taps = None
        if self.imgfilter > 0:
            num_bands = self._fbank_host.shape[0]
            assert len(self.imgfilter_bands) == num_bands
            expected_power = np.array([10, 1, 1, 1]) / 13  # expected power spectrum (1/f)
            g = np.ones((N, num_bands))
            for i, band_strength in enumerate(self.imgfilter_bands):
                t_i = torch.exp2(randn(N) * self.imgfilter_std)
                t_i = torch.where(rand(N) < self.imgfilter * p * band_strength, t_i, torch.ones_like(t_i))
                if q is not None:
                    t_i = torch.full_like(t_i, torch.exp2(torch.erfinv(q * 2 - 1) * self.imgfilter_std)) if band_strength > 0 else torch.ones_like(t_i)
                t = np.ones((N, num_bands))
                t[:, i] = _f64(t_i)[:, 0]
                g = g * (t / np.sqrt((expected_power * t ** 2).sum(axis=-1, keepdims=True)))
            taps = (g @ self._fbank_host).astype(np.float32)

        # noise
        sigma = None
        if self.noise > 0:
            sg = randn(N, 1, 1, 1).abs() * self.noise_std
            sg = torch.where(rand(N, 1, 1, 1) < self.noise * p, sg, torch.zeros_like(sg))
            if q is not None:
                sg = torch.full_like(sg, torch.erfinv(q) * self.noise_std)
            sigma = sg.reshape(N).numpy().copy()

        # cutout: the reference's float32 expression decides every pixel here; the kernel gets the integer rectangle
        rect = None
        if self.cutout > 0:
            size = torch.full([N, 2, 1, 1, 1], self.cutout_size)
            size = torch.where(rand(N, 1, 1, 1, 1) < self.cutout * p, size, torch.zeros_like(size))
            center = rand(N, 2, 1, 1, 1)
            if q is not None:
                size = torch.full_like(size, self.cutout_size)
                center = torch.full_like(center, q)
            coord_x = torch.arange(width).reshape([1, 1, 1, -1])
            coord_y = torch.arange(height).reshape([1, 1, -1, 1])
            keep_x = (((coord_x + 0.5) / width - center[:, 0]).abs() >= size[:, 0] / 2).reshape(N, width).numpy()
            keep_y = (((coord_y + 0.5) / height - center[:, 1]).abs() >= size[:, 1] / 2).reshape(N, height).numpy()
            rect = np.zeros((N, 4), dtype=np.int32)
            for n in range(N):
                for col, keep in ((0, keep_x[n]), (2, keep_y[n])):
                    cut = np.flatnonzero(~keep)
                    if cut.size:
                        assert cut[-1] - cut[0] + 1 == cut.size, "the cut pixels of an axis are an interval"
                        rect[n, col], rect[n, col + 1] = cut[0], cut[-1] + 1
        return AugmentDraw(G_inv, margins, C, taps, sigma, rect)

    # ---- the call ---------------------------------------------------------------------------------------------------------------------------
    def apply_draw(self, images, d, z=None):
        """The two operators on one call's parameters (draw()); z is the noise field when d.sigma is not None."""
        dev = images.device
        if d.G_inv is not None or d.C is not None:
            C = torch.from_numpy(d.C).to(dev, non_blocking=True) if d.C is not None else None
            images = ops.augment_apply(images, d.G_inv, d.margins, C)
        if d.taps is not None or d.sigma is not None or d.rect is not None:
            up = lambda a: torch.from_numpy(a).to(dev, non_blocking=True) if a is not None else None
            images = ops.augment_tail(images, up(d.taps), z if d.sigma is not None else None, up(d.sigma), up(d.rect))
        return images

    def forward(self, images, debug_percentile=None):
        assert isinstance(images, torch.Tensor) and images.ndim == 4
        N, ch, H, W = images.shape
        d = self.draw(N, ch, H, W, debug_percentile)
        z = torch.randn(images.shape, device=images.device, generator=self.noise_generator) if d.sigma is not None else None
        return self.apply_draw(images, d, z)


# ---- the ADA controller (training_loop_v0.py:399-402) -------------------------------------------------------------------------------------
def ada_update(pipe, sign_mean, batch_size, ada_interval, ada_kimg, ada_target):
    """p <- max(p + sign(sign_mean - ada_target) * batch_size * ada_interval / (ada_kimg * 1000), 0), in float32 as the reference's
    tensor arithmetic; writes the buffer and its host mirror.  Returns the new p."""
    adjust = np.sign(sign_mean - ada_target) * (batch_size * ada_interval) / (ada_kimg * 1000)
    new = max(np.float32(pipe.p_host()) + np.float32(adjust), np.float32(0))
    pipe.set_p(new)
    return float(new)


class AdaStats:
    """Collects what ADA needs from the loss's reports: the sum and the count of "Loss/signs/real", added into a device accumulator
    with no synchronisation.  report(name, value) has the signature of loss.report and passes every call on to `previous` (the
    collector it replaces); mean_and_reset() does the one read per ada_interval.

        stats = AdaStats(device, previous=loss.report); loss.report = stats.report"""

    def __init__(self, device, previous=None):
        self.acc = torch.zeros(2, dtype=torch.float64, device=device)  # sum of signs, count
        self.previous = previous

    def report(self, name, value):
        if name == SIGNS_REAL:
            v = torch.as_tensor(value).detach()
            self.acc[0] += v.sum().to(self.acc)
            self.acc[1] += v.numel()
        if self.previous is not None:
            self.previous(name, value)

    def mean_and_reset(self):
        """The mean sign since the last reset (0.0 when nothing was reported): one device-to-host read."""
        total, count = self.acc.tolist()
        self.acc.zero_()
        return total / count if count else 0.0
