"""Shared cases of the synthesis-network gradient tests (tests/test_synthesis_grad_cpu.py on CPU with the torch restatements of the
operators, tests/test_hip_synthesis_grad.py on the HIP kernels): the generators of syn_generator_{none,cond}.npz differentiated
against the reference's own fp32 autograd (tests/golden/make_golden_synthesis_grad.py -> syn_grad_{none,cond}.npz)."""
import numpy as np
import torch

import p3d_testing as T

GEN_KW = dict(z_dim=64, c_dim=25, w_dim=64, img_resolution=32, img_channels=96, mapping_kwargs={"num_layers": 2},
              channel_base=2048, channel_max=64, num_fp16_res=0, conv_clamp=None, fused_modconv_default="inference_only")
COND_GRAD = ("image_ortho_front", "resnet_chonk")
THIN = 3  # make_golden_synthesis_grad.thin


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def thin(a):
    a = np.asarray(a)
    return a.reshape(-1)[::THIN] if a.size > 4096 else a


def build(P, tag, device):
    """(generator, ws leaf, cond with the COND_GRAD leaves, injections, cotangent, stop level, fixture) for one case."""
    g = T.load_golden(f"syn_grad_{tag}.npz")
    gen = T.load_golden(f"syn_generator_{tag}.npz")
    G = P.stylegan2.Generator(cond_mode=str(gen["cond_mode"]), **GEN_KW)
    G.load_state_dict({k[3:].replace("__", "."): torch.from_numpy(v) for k, v in gen.items() if k.startswith("sd_")}, strict=True)
    G = G.eval().to(device)
    cond = {k[5:]: torch.from_numpy(np.ascontiguousarray(v)).to(device) for k, v in gen.items() if k.startswith("cond_") and k != "cond_mode"}
    for k in COND_GRAD:
        cond[k].requires_grad_(True)
    ws = torch.from_numpy(gen["ws"]).to(device).requires_grad_(True)
    net = G.synthesis
    gg = torch.Generator().manual_seed(93)  # the fixture script's draws, in its order
    ch = lambda res: min(GEN_KW["channel_base"] // res, GEN_KW["channel_max"])
    N = ws.shape[0]
    da0 = torch.randn((N, ch(4), 4, 4), generator=gg) * 0.3
    db1 = torch.randn((N, GEN_KW["img_channels"], 8, 8), generator=gg) * 0.3
    g_out = torch.randn((N, GEN_KW["img_channels"], 32, 32), generator=gg)
    chk = float(g_out.double().sum() + da0.double().sum() + db1.double().sum())
    assert abs(chk - float(g["draw_checksum"][0])) < 1e-6 * max(1.0, abs(chk)), "the fixture's draws could not be reproduced"
    inj = {"da_0": da0.to(device).requires_grad_(True), "db_1": db1.to(device).requires_grad_(True)}
    sl = int(g["stop_level"])
    return G, net, ws, cond, inj, g_out.to(device), (None if sl < 0 else sl), g


def check_against_fixture(net, ws, cond, inj, g, tol=1e-4):
    """Every recorded gradient within relative L2 `tol`; parameters the fixture has no gradient for get none (or zeros)."""
    bad = []

    def cmp(name, ours, ref):
        if ours is None:
            bad.append((name, "missing"))
            return
        e = rel_l2(thin(ours.detach().cpu().numpy()) if ref.ndim == 1 and ours.numel() > 4096 else ours.detach().cpu().numpy(), ref)
        if not e <= tol:
            bad.append((name, e))
    cmp("ws", ws.grad, g["g_ws"])
    for k, v in inj.items():
        if "g_inj_" + k in g:
            cmp(k, v.grad, g["g_inj_" + k])
        elif v.grad is not None and torch.count_nonzero(v.grad) > 0:
            bad.append((k, "non-zero gradient where the reference has none"))
    for k in COND_GRAD:
        if "g_cond_" + k in g:
            cmp(k, cond[k].grad, g["g_cond_" + k])
        elif cond[k].grad is not None and torch.count_nonzero(cond[k].grad) > 0:
            bad.append((k, "non-zero gradient where the reference has none"))
    for n, p in net.named_parameters():
        key = "g_" + n.replace(".", "__")
        if key in g:
            cmp(n, p.grad, g[key])
        elif p.grad is not None and torch.count_nonzero(p.grad) > 0:
            bad.append((n, "non-zero gradient where the reference has none"))
    assert not bad, bad
