"""Shared by tests/test_augment_pipe_cpu.py, tests/test_hip_augment_pipe.py and tests/golden/make_golden_augment_pipe.py: the cases of
the augmentation pipe's module and of its tail operator, a float64 restatement of the tail of include/p3d_augment_tail.h (forward,
adjoint, the sum of the absolute terms for the gate), seeded faults of that restatement, and the whole pipe in float64 from one call's
parameters (augment_cases.Restated, then the tail).

Inputs come from augment_cases.images / cotangent and are not stored.
"""
import os

import numpy as np

import augment_cases as AC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "augment_pipe_module.npz")
EPS = AC.EPS

# The tail family: the reference's pipe at debug percentiles (0.5 is the identity filter), each pipe on its shape.  22 is the smallest
# side the reference accepts (reflect pad 21): there every interior pixel has two mirror images.
TAIL_PERCENTILES = [0.1, 0.37, 0.8, 0.95]
TAIL_PIPES = [dict(imgfilter=1, cutout=1), dict(imgfilter=1, imgfilter_bands=[1, 0, 1, 1]), dict(**AC.BGC, imgfilter=1, cutout=1)]
TAIL_SHAPES = [(2, 3, 22, 23), (1, 1, 22, 22), (2, 6, 24, 40)]
TAIL_SEED = 20  # augment_cases.images(shape, TAIL_SEED + index)

# Random mode: AugmentPipe(**RANDOM_PIPE) with p set, after torch.manual_seed(seed).
RANDOM_PIPE = dict(**AC.BGC, imgfilter=1, cutout=1)
RANDOM_P = [0.6, 1.0]
RANDOM_SEEDS = [0, 1, 2]
RANDOM_SHAPES = [(4, 6, 24, 40), (3, 3, 22, 23)]
RANDOM_SEED = 40

FAULTS = ["edge_repeat", "filter_flipped", "rect_off_by_one", "no_mirror_images", "noise_after_cutout"]
# Not a fault: the two passes act on different axes with the same taps, so "columns before rows" is the same operator (Fc (x) Fr in
# either order) up to rounding.  The restatement can run it (fault="columns_first") and the test shows it equal.
NOT_A_FAULT = "columns_first"


def tail_key(kind, pipe_index, q):
    return f"tail_{kind}_p{pipe_index}_{q}"


def random_key(kind, shape_index, p, seed):
    return f"random_{kind}_s{shape_index}_p{p}_seed{seed}"


def terms_forward(K):
    """the longest rounding chain of a forward output (include/p3d_augment_tail.h): two passes of K taps and the noise's fma"""
    return 2 * max(K, 1) + 1


def terms_adjoint(K):
    """two passes, each a chain of K taps and the two adds of the mirror images"""
    return 2 * (max(K, 1) + 2)


def _reflect(q, n, edge_repeat=False):
    if edge_repeat:
        return -q - 1 if q < 0 else (2 * n - 1 - q if q >= n else q)
    return -q if q < 0 else (2 * (n - 1) - q if q >= n else q)


def _axis_matrix(h, n, edge_repeat=False):
    """[n, n]: out[j] = sum_k h[k] in[refl(j + k - R)]"""
    K = len(h)
    R = K // 2
    assert R < n
    F = np.zeros((n, n))
    for j in range(n):
        for k in range(K):
            F[j, _reflect(j + k - R, n, edge_repeat)] += h[k]
    return F


def _axis_matrix_no_images(h, n):
    """the transposed correlation WITHOUT the fold: only the pixel itself (the fault)"""
    K = len(h)
    R = K // 2
    F = np.zeros((n, n))
    for j in range(n):
        for k in range(K):
            if 0 <= j + k - R < n:
                F[j, j + k - R] += h[k]
    return F


class TailRestated:
    """The tail for one call's parameters, in float64: .forward(x), .adjoint(g), .bound(x), .adjoint_bound(g).
    taps [N, K] or None, z [N, C, H, W] and sigma [N] or None, rect [N, 4] = (x0, x1, y0, y1) or None."""

    def __init__(self, shape, taps=None, z=None, sigma=None, rect=None, fault=None):
        self.N, self.C, self.H, self.W = shape
        self.fault = fault
        self.taps = None if taps is None else np.asarray(taps, dtype=np.float64)
        self.K = 0 if taps is None else self.taps.shape[1]
        self.noise = None if sigma is None else np.asarray(sigma, dtype=np.float64)[:, None, None, None] * np.asarray(z, dtype=np.float64)
        self.keep = np.ones((self.N, 1, self.H, self.W))
        if rect is not None:
            for n, (x0, x1, y0, y1) in enumerate(np.asarray(rect, dtype=np.int64)):
                if fault == "rect_off_by_one" and x1 > x0 and y1 > y0:
                    x0, x1 = x0 + 1, x1 + 1
                self.keep[n, 0, max(y0, 0):max(y1, 0), max(x0, 0):max(x1, 0)] = 0
        self.Fr = self.Fc = None
        if self.taps is not None:
            h = self.taps[:, ::-1] if fault == "filter_flipped" else self.taps
            er = fault == "edge_repeat"
            self.Fr = np.stack([_axis_matrix(hn, self.W, er) for hn in h])
            self.Fc = np.stack([_axis_matrix(hn, self.H, er) for hn in h])

    def _filter(self, x, Fr, Fc):
        if Fr is None:
            return x
        if self.fault == "columns_first":
            return np.einsum("nqw,nchw->nchq", Fr, np.einsum("nrh,nchw->ncrw", Fc, x))
        return np.einsum("nrh,nchw->ncrw", Fc, np.einsum("nqw,nchw->nchq", Fr, x))

    def forward(self, x):
        f = self._filter(np.asarray(x, dtype=np.float64), self.Fr, self.Fc)
        if self.fault == "noise_after_cutout":
            return f * self.keep + (self.noise if self.noise is not None else 0)
        if self.noise is not None:
            f = f + self.noise
        return f * self.keep

    def bound(self, x):
        """the gate of the forward: 8 sqrt(K) 2^-24 sum|terms|, K the length of the longest rounding chain"""
        total = self._filter(np.abs(np.asarray(x, dtype=np.float64)), None if self.Fr is None else np.abs(self.Fr), None if self.Fc is None else np.abs(self.Fc))
        if self.noise is not None:
            total = total + np.abs(self.noise)
        return 8 * np.sqrt(terms_forward(self.K)) * EPS * total * self.keep

    def adjoint(self, g, absolute=False):
        g = np.asarray(g, dtype=np.float64)
        a = np.abs if absolute else (lambda v: v)
        m = a(g) * self.keep
        if self.Fr is None:
            return m
        Fr, Fc = self.Fr, self.Fc
        if self.fault == "no_mirror_images":
            Fr = np.stack([_axis_matrix_no_images(hn, self.W) for hn in self.taps])
            Fc = np.stack([_axis_matrix_no_images(hn, self.H) for hn in self.taps])
        return np.einsum("nqw,nchq->nchw", a(Fr), np.einsum("nrh,ncrw->nchw", a(Fc), m))

    def adjoint_bound(self, g):
        return 8 * np.sqrt(terms_adjoint(self.K)) * EPS * self.adjoint(g, absolute=True)


class PipeRestated:
    """The whole pipe for one call's parameters in float64: augment_cases.Restated (geometry and colour), then the tail.
    M (float64 [N, 2, 3], e.g. from a recorded theta) replaces G_inv when given."""

    def __init__(self, hz, shape, G_inv, margins, C, taps, rect, z=None, sigma=None, M=None):
        self.head = AC.Restated(hz, shape, G_inv, margins, C, M=M) if (G_inv is not None or M is not None or C is not None) else None
        self.tail = TailRestated(shape, taps, z, sigma, rect)

    def forward(self, x):
        return self.tail.forward(self.head.forward(x) if self.head is not None else x)

    def adjoint(self, g):
        g = self.tail.adjoint(g)
        return self.head.adjoint(g) if self.head is not None else g


def tail_inputs(index):
    shape = TAIL_SHAPES[index]
    return AC.images(shape, TAIL_SEED + index), AC.cotangent(shape, TAIL_SEED + index)


def random_inputs(index):
    return AC.images(RANDOM_SHAPES[index], RANDOM_SEED + index)


def explicit_tail(shape, K, seed, filt=True, noise=True, cutout=True, symmetric=False, rect_kind="inner"):
    """One tail case on explicit parameters: (x, g, taps, z, sigma, rect).  The taps are non-symmetric unless asked: a low-pass bump
    plus noise, normalised to sum 1 per sample."""
    N, C, H, W = shape
    g = np.random.default_rng(seed + 77)
    taps = z = sigma = rect = None
    if filt:
        k = np.arange(K) - K // 2
        taps = np.exp(-0.5 * (k / max(K / 6, 0.5)) ** 2)[None] + 0.2 * g.standard_normal((N, K))
        if symmetric:
            taps = (taps + taps[:, ::-1]) / 2
        taps = (taps / taps.sum(axis=1, keepdims=True)).astype(np.float32)
    if noise:
        z, sigma = g.standard_normal(shape).astype(np.float32), np.abs(g.standard_normal(N)).astype(np.float32) * 0.3
    if cutout:
        rect = np.zeros((N, 4), dtype=np.int32)
        for n in range(N):
            if rect_kind == "inner":
                rect[n] = [W // 4 + n, W // 4 + n + max(W // 2, 1), H // 3, H // 3 + max(H // 2 - n, 1)]
            elif rect_kind == "all":
                rect[n] = [-3, W + 5, 0, H]
            # "empty": zeros
    return AC.images(shape, seed), AC.cotangent(shape, seed), taps, z, sigma, rect


# ---- a torch stand-in of the tail and of the whole pipe (any device, any float dtype) -----------------------------------------------------
def torch_tail(x, taps=None, z=None, sigma=None, rect=None):
    """ops.augment_tail's semantics from torch's own operators: F.pad reflect, the two grouped F.conv2d, add, multiply."""
    import torch
    F = torch.nn.functional
    N, C, H, W = x.shape
    if taps is not None:
        K = taps.shape[1]
        w = taps.to(x).unsqueeze(1).repeat(1, C, 1).reshape(N * C, 1, K)
        y = F.pad(x.reshape(1, N * C, H, W), [K // 2] * 4, mode="reflect")
        y = F.conv2d(y, w.unsqueeze(2), groups=N * C)
        x = F.conv2d(y, w.unsqueeze(3), groups=N * C).reshape(N, C, H, W)
    if sigma is not None:
        x = x + z.to(x) * sigma.to(x).reshape(N, 1, 1, 1)
    if rect is not None:
        jj, ii = torch.arange(W, device=x.device).view(1, 1, 1, W), torch.arange(H, device=x.device).view(1, 1, H, 1)
        r = rect.to(x.device).long().view(N, 4, 1, 1, 1)
        x = x * (~((jj >= r[:, 0]) & (jj < r[:, 1]) & (ii >= r[:, 2]) & (ii < r[:, 3]))).to(x)
    return x


def linear_twice(fn):
    """fn: an affine map of a tensor onto one of the same shape, from torch operators that have no double backward (grid_sample) ->
    the same map, differentiable to any order: its backward is its own vector-Jacobian product, and that one's backward the linear part."""
    import torch

    class Fn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, adjoint):
            ctx.adjoint = adjoint
            if not adjoint:
                with torch.no_grad():
                    return fn(x)
            with torch.enable_grad():
                x0 = torch.zeros_like(x).requires_grad_(True)
                return torch.autograd.grad(fn(x0), x0, x)[0]

        @staticmethod
        def backward(ctx, g):
            if ctx.adjoint:
                with torch.no_grad():
                    return Fn.apply(g, False) - fn(torch.zeros_like(g)), None
            return Fn.apply(g, True), None
    return lambda x: Fn.apply(x, False)


def torch_pipe(hz, d, z=None):
    """One call's parameters (AugmentPipe.draw) -> the pipe from torch's operators (augment_cases.torch_operator, then torch_tail)."""
    import torch
    op = AC.torch_operator(hz)
    up = lambda a, dev: None if a is None else torch.from_numpy(np.asarray(a)).to(dev)

    def fn(x):
        if d.G_inv is not None or d.C is not None:
            x = op(x, d.G_inv, d.margins, up(d.C, x.device))
        return torch_tail(x, up(d.taps, x.device), z, up(d.sigma, x.device), up(d.rect, x.device))
    return linear_twice(fn)


def debug_taps64(pipe_kwargs, q, fbank32, N):
    """The filter rows of a debug-percentile call in exact arithmetic from its float32 parameter (float64, unrounded): the band gain
    t = exp2(erfinv(2 q - 1) * std) as float32, then augment.py:385-400 in float64 on the buffer's float32 values.  Neither the
    reference's float32 products nor the module's single rounding is in it."""
    import torch
    std, bands = pipe_kwargs.get("imgfilter_std", 1), pipe_kwargs.get("imgfilter_bands", [1, 1, 1, 1])
    t_q = float(torch.exp2(torch.erfinv(torch.as_tensor(q, dtype=torch.float32) * 2 - 1) * float(std)))
    power = np.array([10, 1, 1, 1]) / 13
    g = np.ones(4)
    for i, strength in enumerate(bands):
        t = np.ones(4)
        t[i] = t_q if strength > 0 else 1.0
        g = g * (t / np.sqrt((power * t ** 2).sum()))
    return np.tile(g @ np.asarray(fbank32, dtype=np.float64), (N, 1))
