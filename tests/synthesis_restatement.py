"""A plain-torch restatement of the triplane backbone's SynthesisNetwork (networks_stylegan2.py:299-487 and the PAniC-3D conditioning
'ortho_front.add_shuffle2_4.inj_6b_4' of :551-694), written from the formulas and independent of stylegan2.py's host code: no
StylePlan, no caches, no fused operators.  It runs in any dtype on any device, so torch autograd differentiates it — in float64 on
CPU as the yardstick of tests/test_hip_synthesis_grad.py, and in float32 on the GPU as the baseline of tools/bench_synthesis_grad.py."""
import numpy as np
import torch
import torch.nn.functional as F

SUPPORTED_COND = ("none", "ortho_front.add_shuffle2_4.inj_6b_4", "ortho_front.add_shuffle2_4.inj_6b_4.resnetcond_8")


def _fir(f, dtype, device):
    f = f.to(dtype=dtype, device=device)
    return (f * 4.0).flip([0, 1])


def _upfirdn_up2(x, f):
    """upsample2d(x, f): zero-insert, pad [2,1,2,1], FIR with f * 4 (upfirdn2d.py:315-350)."""
    N, C, H, W = x.shape
    xu = torch.zeros((N, C, 2 * H, 2 * W), dtype=x.dtype, device=x.device)
    xu[:, :, ::2, ::2] = x
    k = _fir(f, x.dtype, x.device)[None, None].repeat(C, 1, 1, 1)
    return F.conv2d(F.pad(xu, [2, 1, 2, 1]), k, groups=C)


def _affine(p, name, w):
    A, b = p[name + ".affine.weight"], p[name + ".affine.bias"]
    return w @ (A * (1.0 / np.sqrt(A.shape[1]))).t() + b  # FullyConnectedLayer, lr_multiplier 1 (bias_gain 1)


def _layer(p, name, x, w, up, f, clamp, keep, branch=None, outputs=None):
    y = _layer_impl(p, name, x, w, up, f, clamp, keep, branch)
    if outputs is not None:
        outputs.append(y.detach())
    return y


def _layer_impl(p, name, x, w, up, f, clamp, keep, branch):
    W = p[name + ".weight"]
    s = _affine(p, name, w)
    d = ((W.square().sum(dim=(2, 3))[None] * s.square()[:, None, :]).sum(dim=2) + 1e-8).rsqrt()
    xm = x * s[:, :, None, None]
    if up == 1:
        y = F.conv2d(xm, W, padding=1)
    else:  # conv2d_resample.py:114-128: transposed conv (stride 2), then the FIR with pad [1,1,1,1], gain 4
        y = F.conv_transpose2d(xm, W.transpose(0, 1), stride=2)
        k = _fir(f, y.dtype, y.device)[None, None].repeat(y.shape[1], 1, 1, 1)
        y = F.conv2d(F.pad(y, [1, 1, 1, 1]), k, groups=y.shape[1])
    noise = p[name + ".noise_const"] * p[name + ".noise_strength"]
    if keep is not None and noise.requires_grad:  # (the noise input's own gradient, for the conditioning of the strength's sum)
        noise.retain_grad()
        keep[name] = noise
    y = y * d[:, :, None, None] + noise + p[name + ".bias"][None, :, None, None]
    if branch is None:
        y = F.leaky_relu(y, 0.2) * np.sqrt(2)
        return y.clamp(-clamp, clamp) if clamp is not None else y
    # the lrelu slope and the clamp decided by another evaluation's output (the same kinks on both sides of a comparison)
    branch = branch.to(dtype=y.dtype, device=y.device)
    y = torch.where(branch > 0, y, y * 0.2) * np.sqrt(2)
    return torch.where(branch.abs() < clamp, y, y.detach().clamp(-clamp, clamp)) if clamp is not None else y


def _torgb(p, name, x, w, clamp):
    W = p[name + ".weight"]
    s = _affine(p, name, w) * (1.0 / np.sqrt(W.shape[1]))
    y = F.conv2d(x * s[:, :, None, None], W) + p[name + ".bias"][None, :, None, None]
    return y.clamp(-clamp, clamp) if clamp is not None else y


def _unshuffle(t, f):
    b, ch, H, W = t.shape
    t = t.reshape(b, ch, H // f, f, W // f, f).permute(0, 3, 5, 1, 2, 4)
    return t.reshape(b, f * f * ch, H // f, W // f)


def synthesis(p, ws, cond, cond_mode, resolutions, filt, conv_clamp, keep=None, branches=None, outputs=None):
    """p: {parameter / buffer name of a SynthesisNetwork: tensor}; ws [N, num_ws, w_dim]; cond {'image_ortho_front': [N,3,S,S]} (or
    unused for cond_mode 'none'); constant noise.  Returns the output image [N, C, R, R].  keep: a dict that receives each layer's
    noise input (noise_const * strength, gradient retained).  branches: the layers' outputs of another evaluation, in execution order —
    each layer's lrelu slope and clamp are then taken from them (torch autograd differentiates the same branch at every kink).
    outputs: a list that receives every layer's output (detached), in execution order."""
    nxt = (lambda: next(branches)) if branches is not None else (lambda: None)
    assert cond_mode in SUPPORTED_COND
    conditioned = cond_mode != "none"
    interp = F.interpolate
    cimg = cond["image_ortho_front"].flip(dims=(-2,)) * 2 - 1 if conditioned else None
    x = img = None
    wi = 0
    for lvl, res in enumerate(resolutions):
        b = f"b{res}"
        if res == 4:
            x = p[b + ".const"][None].expand(ws.shape[0], -1, -1, -1)
            x = _layer(p, b + ".conv1", x, ws[:, wi], 1, filt, conv_clamp, keep, nxt(), outputs)
            img = _torgb(p, b + ".torgb", x, ws[:, wi + 1], conv_clamp)
            wi += 1
        else:
            x = _layer(p, b + ".conv0", x, ws[:, wi], 2, filt, conv_clamp, keep, nxt(), outputs)
            x = _layer(p, b + ".conv1", x, ws[:, wi + 1], 1, filt, conv_clamp, keep, nxt(), outputs)
            img = _upfirdn_up2(img, filt) + _torgb(p, b + ".torgb", x, ws[:, wi + 2], conv_clamp)
            wi += 2
        if conditioned:  # add_shuffle2_4 at every level, inj_6b_4 at the last
            if lvl < len(resolutions) - 2:
                t = interp(cimg, size=x.shape[-2:], mode="bilinear")
            else:
                t = _unshuffle(cimg, cimg.shape[-1] // x.shape[-1])
            t = t.repeat(1, int((x.shape[1] / 4) // t.shape[1]), 1, 1)
            k = t.shape[1]
            x = torch.cat([x[:, :x.shape[1] - k], x[:, x.shape[1] - k:] + t], dim=1)
            if res == resolutions[-1]:
                front = cond["image_ortho_front"]
                ti = interp((front.flip(dims=(-2,)) * 2 - 1) * 4, size=img.shape[-2:], mode="bilinear")
                img = torch.cat([img[:, :ti.shape[1]] + ti, img[:, ti.shape[1]:]], dim=1)
    return img
