"""Float64 references of the synthesis backward's C ABI (include/p3d_synthesis_grad.h), written from the header's formulas and not
from the kernels, and the element-wise error gate every kernel-level test of it applies.

Each GEMM-like reference also returns the same sum taken over absolute values (|g|·|w|, |x·g|, ...): the scale of an fp32 result's
rounding error element by element.  The gate: |ours - ref| <= GATE_C · sqrt(K) · 2^-24 · absref (K = the length of the sum), plus
relative L2 <= REL_L2 per tensor.  tests/test_synthesis_grad_ref_cpu.py checks the references against torch autograd and shows that
the gate fails a float32 result with one chunk, tile, tap, slab or sample wrong; tests/test_hip_synthesis_grad_edges.py applies it
to the kernels."""
import math

import numpy as np
import torch
import torch.nn.functional as F

EPS32 = 2.0 ** -24
GATE_C = 8.0    # one constant for every gated tensor
REL_L2 = 1e-5
ULP_MAX = 2     # element-wise results (bias_act's g_out): within 2 ulp of the float64 value


def f32(v):
    """The float32 value the C ABI receives for a Python float."""
    return float(np.float32(v))


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double().ravel(), torch.as_tensor(b).double().ravel()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


# ---- the gate ---------------------------------------------------------------------------------------------------------------
def gate_ratio(ours, ref, absref, K):
    """max over elements of |ours - ref| / (sqrt(K) · 2^-24 · absref); an element with absref == 0 must be exact (else inf)."""
    d = (torch.as_tensor(ours).double().cpu() - ref.double()).abs()
    scale = math.sqrt(max(K, 1)) * EPS32 * absref.double()
    r = torch.where(scale > 0, d / scale.clamp_min(1e-300), torch.where(d > 0, math.inf, 0.0))
    return float(r.max()) if r.numel() else 0.0


def gate_passes(ours, ref, absref, K):
    return gate_ratio(ours, ref, absref, K) <= GATE_C and rel_l2(torch.as_tensor(ours).cpu(), ref) <= REL_L2


def gate(name, ours, ref, absref, K):
    """Assert the gate for one tensor; prints the worst ratio (against GATE_C) so that a drift toward the gate shows in the log."""
    r = gate_ratio(ours, ref, absref, K)
    e = rel_l2(torch.as_tensor(ours).cpu(), ref)
    print(f"gate {name}: worst {r:.3f} (c = {GATE_C:g}, K = {K}), rel-L2 {e:.2e}")
    assert r <= GATE_C and e <= REL_L2, (name, r, e)
    return r


def ulp_distance(ours, ref):
    """max |ours - ref| in units of the ulp of fp32(ref), ref the float64 value (an exact zero must be matched exactly)."""
    r64 = ref.double().cpu().numpy()
    o = torch.as_tensor(ours).float().cpu().numpy()
    sp = np.spacing(np.abs(r64.astype(np.float32))).astype(np.float64)
    d = np.abs(o.astype(np.float64) - r64)
    return float(np.max(np.where(d == 0, 0.0, d / sp))) if d.size else 0.0


# ---- bias_act backward --------------------------------------------------------------------------------------------------------
def bias_act_masks(y, act, clamp):
    """The header's rule on the float32 output y: (keep = clamp < 0 or |y| < clamp, lrelu slope taken = act == 1 and y <= 0)."""
    keep = torch.ones_like(y, dtype=torch.bool) if clamp is None or clamp < 0 else y.abs() < f32(clamp)
    neg = (y <= 0) if act == 1 else torch.zeros_like(y, dtype=torch.bool)
    return keep, neg


def bias_act_backward_ref(y, g_y, act, alpha, gain, clamp, dscale=None, dtype=torch.float64):
    """g_z = g_y · gain · keep · (neg ? alpha : 1); (g_z, g_out = g_z · dscale[n,c], g_bias [N,C], g_noise [N,HW], |.| sums of both)."""
    N, C = y.shape[0], y.shape[1]
    keep, neg = bias_act_masks(y, act, clamp)
    gz = g_y.to(dtype) * f32(gain)
    gz = torch.where(neg, gz * f32(alpha), gz)
    gz = torch.where(keep, gz, torch.zeros_like(gz)).reshape(N, C, -1)
    out = gz if dscale is None else gz * dscale.to(dtype).reshape(N, C, 1)
    return dict(g_z=gz.reshape(y.shape), g_out=out.reshape(y.shape), g_bias=gz.sum(2), abs_bias=gz.abs().sum(2), g_noise=gz.sum(1),
                abs_noise=gz.abs().sum(1))


# ---- data gradient --------------------------------------------------------------------------------------------------------------
def _tap_windows(t, stride, step, pad, taps, Ho, Wo):
    """t [N,C,H,W] read at (stride·oy + step·ty - pad, stride·ox + step·tx - pad), zero outside: [taps][N,C,Ho,Wo] views."""
    H, W = t.shape[-2:]
    kt = 3 if taps == 9 else 1
    need_h = stride * (Ho - 1) + step * (kt - 1) + 1  # rows of the padded map the windows span
    need_w = stride * (Wo - 1) + step * (kt - 1) + 1
    tp = F.pad(t, [pad, max(0, need_w - W - pad), pad, max(0, need_h - H - pad)])
    out = []
    for k in range(taps):
        ty, tx = (k // 3, k % 3) if taps == 9 else (0, 0)
        y0, x0 = step * ty, step * tx
        out.append(tp[:, :, y0:y0 + stride * (Ho - 1) + 1:stride, x0:x0 + stride * (Wo - 1) + 1:stride])
    return out


def conv_dgrad_ref(g, wk, Co, Ho, Wo, stride, pad, dtype=torch.float64):
    """out[n,co,oy,ox] = sum_{ci,t} g[n,ci,stride·oy + ty - pad, stride·ox + tx - pad] · wk[t,ci,co]: (out, sum of |.| terms)."""
    g, wk = g.to(dtype), wk.to(dtype)
    taps = wk.shape[0]
    assert wk.shape[2] == Co
    out = torch.zeros(g.shape[0], Co, Ho, Wo, dtype=dtype)
    absout = torch.zeros_like(out)
    for t, win in enumerate(_tap_windows(g, stride, 1, pad, taps, Ho, Wo)):
        out += torch.einsum("nchw,cd->ndhw", win, wk[t])
        absout += torch.einsum("nchw,cd->ndhw", win.abs(), wk[t].abs())
    return out, absout


# ---- modulation backward ------------------------------------------------------------------------------------------------------
def mod_backward_ref(x, s, g, dtype=torch.float64):
    """(g_s [N,C] = sum over pixels of x · g, its |.| sum, g · s)."""
    N, C = x.shape[0], x.shape[1]
    shape = g.shape
    x, g, s = x.to(dtype).reshape(N, C, -1), g.to(dtype).reshape(N, C, -1), s.to(dtype).reshape(N, C, 1)
    return (x * g).sum(2), (x * g).abs().sum(2), (g * s).reshape(shape)


# ---- weight gradient ----------------------------------------------------------------------------------------------------------
def wgrad_operands(g, gmap, x, s, xmap, taps, domain, dtype=torch.float64):
    """The header's two index maps over the domain: (G [N,taps,O,P], X·s [N,taps,I,P]), P = Hd·Wd in row-major order."""
    Hd, Wd = domain
    N = g.shape[0]
    G = torch.stack(_tap_windows(g.to(dtype), gmap[0], gmap[1], gmap[2], taps, Hd, Wd), 1).reshape(N, taps, g.shape[1], Hd * Wd)
    xs = x.to(dtype)
    if s is not None:
        xs = xs * s.to(dtype)[:, :, None, None]
    X = torch.stack(_tap_windows(xs, xmap[0], xmap[1], xmap[2], taps, Hd, Wd), 1).reshape(N, taps, x.shape[1], Hd * Wd)
    return G, X


def conv_wgrad_ref(g, gmap, x, s, xmap, taps, domain, wk=None, dscale=None, dtype=torch.float64):
    """dw [taps,O,I] = sum over n and the domain of G · X·s, and with wk [taps,O,I], dscale [N,O]: g_d[n,o] = sum_{t,i} wk · dw_n / dscale.
    Returns dict(dw, abs_dw, dw_n, abs_dw_n[, g_d, abs_g_d])."""
    G, X = wgrad_operands(g, gmap, x, s, xmap, taps, domain, dtype)
    dwn = torch.einsum("ntop,ntip->ntoi", G, X)
    adwn = torch.einsum("ntop,ntip->ntoi", G.abs(), X.abs())
    r = dict(dw=dwn.sum(0), abs_dw=adwn.sum(0), dw_n=dwn, abs_dw_n=adwn)
    if wk is not None:
        wk, d = wk.to(dtype), dscale.to(dtype)
        r["g_d"] = torch.einsum("toi,ntoi->no", wk, dwn) / d
        r["abs_g_d"] = torch.einsum("toi,ntoi->no", wk.abs(), adwn) / d.abs()
    return r


def sg_split(N, O, I, taps, Hd, Wd):
    """(slabs, pixels per slab) of p3d_conv_wgrad_f32's split of each sample's pixels — mirrored only to assert that the test
    matrix has several slabs with a ragged last one, and for the sensitivity checks."""
    P = Hd * Wd
    tiles = taps * -(-O // 64) * -(-I // 64)
    want = min(-(-2048 // (tiles * N)), -(-P // 256))
    want = max(want, 1)
    K = -(-P // want)
    K = -(-K // 16) * 16
    return -(-P // K), K


# ---- layers -------------------------------------------------------------------------------------------------------------------
def act_masked(z, y_ours, alpha, gain, clamp, act="lrelu"):
    """clamp(act(z) · gain) whose branch decisions (lrelu slope, clamp) are those of the kernel's fp32 output y_ours: both sides
    differentiate the same branch at every kink."""
    a = torch.where(y_ours > 0, z, z * alpha) if act == "lrelu" else z
    a = a * gain
    if clamp is not None:
        keep = y_ours.abs() < clamp
        a = torch.where(keep, a, a.detach().clamp(-clamp, clamp))
    return a


def fir_ref(f, gain=4.0):
    """The 2-D filter as upfirdn2d applies it (flipped for a convolution, times gain), float64."""
    return (f.double() * gain).flip([0, 1])


def upsample2d_ref(x, f, up=2, padding=0):
    """upfirdn2d.upsample2d restated: zero-insert, pad (upsample2d's own padding plus the caller's), FIR with gain up^2."""
    if isinstance(padding, int):
        padding = [padding] * 4
    elif len(padding) == 2:
        padding = [padding[0], padding[0], padding[1], padding[1]]
    px0, px1, py0, py1 = padding
    N, C, H, W = x.shape
    fh, fw = f.shape
    z = torch.zeros(N, C, H * up, W * up, dtype=x.dtype)
    z[:, :, ::up, ::up] = x
    z = F.pad(z, [px0 + (fw + up - 1) // 2, px1 + (fw - up) // 2, py0 + (fh + up - 1) // 2, py1 + (fh - up) // 2])
    k = fir_ref(f, up * up).to(x.dtype)[None, None].repeat(C, 1, 1, 1)
    return F.conv2d(z, k, groups=C)
