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


# ---- the kernel-level matrix of tests/test_hip_synthesis_grad_edges.py ------------------------------------------------------------
# A designed covering list, not a product: every tail of the 64 x 64 GEMM tiles and 16-wide K chunks (1, 15/17, 63/65, 130), maps
# that are non-square with pixel counts off multiples of 16 and 64, and every (taps, stride, pad) / index map the ABI documents.
# tests/test_synthesis_grad_ref_cpu.py checks the gate at the largest K of each list.
def _dgrad_cases():
    """(N, Ci, Co, Hi, Wi, Ho, Wo, taps, stride, pad): Ci is the K-chunk tail, Co the row-tile tail."""
    CI, CO = (1, 15, 16, 17, 33, 130), (1, 3, 63, 64, 65, 130)
    MAPS = ((1, 1), (7, 13), (5, 67), (33, 33), (13, 7), (4, 9))
    out, i = [], 0
    for taps in (1, 9):
        for stride in (1, 2):
            for pad in (0, 1, 2):
                for _ in range(3):
                    Ho, Wo = MAPS[(i + i // 6) % 6]
                    kt = 3 if taps == 9 else 1
                    Hi = max(1, stride * (Ho - 1) + kt - 2 * pad + i % 3 - 1)
                    Wi = max(1, stride * (Wo - 1) + kt - 2 * pad + (i + 1) % 3 - 1)
                    out.append((3 if (i // 2) % 2 else 1, CI[i % 6], CO[(i + i // 6) % 6], Hi, Wi, Ho, Wo, taps, stride, pad))
                    i += 1
    # the product layers at 4^2 and 8^2: plain (flipped weights), up (stride 2 after the FIR adjoint), 1x1
    out += [(1, 512, 512, 4, 4, 4, 4, 9, 1, 1), (3, 512, 512, 8, 8, 8, 8, 9, 1, 1), (1, 512, 512, 9, 9, 4, 4, 9, 2, 0),
            (3, 512, 256, 17, 17, 8, 8, 9, 2, 0), (1, 96, 256, 8, 8, 8, 8, 1, 1, 0)]
    return out


DGRAD_CASES = _dgrad_cases()

# index maps of p3d_conv_wgrad_f32: kind -> (taps, (sg, ag, pg), (sx, ax, px0), g map size, x map size) for a domain (Hd, Wd)
WGRAD_MAPS = {
    "plain": (9, (1, 0, 0), (1, 1, 1), lambda h, w: (h, w), lambda h, w: (h, w)),
    "up": (9, (2, 1, 0), (1, 0, 0), lambda h, w: (2 * h + 1, 2 * w + 1), lambda h, w: (h, w)),
    "1x1": (1, (1, 0, 0), (1, 0, 0), lambda h, w: (h, w), lambda h, w: (h, w)),
    "pad2": (9, (1, 1, 2), (2, 1, 2), lambda h, w: (h + 1, w + 2), lambda h, w: (2 * h, 2 * w + 1)),  # not a product map
    "step0": (9, (2, 0, 1), (1, 1, 0), lambda h, w: (2 * h, 2 * w), lambda h, w: (h + 2, w + 1)),
}
# (kind, N, O, I, Hd, Wd): O is the row-tile tail, I the column-tile tail, the domain the K of one sample (P < 16, P % 16 != 0,
# several slabs with a ragged last one where O·I is small and the map large)
_WG = [("plain", 1, 1, 1, 1, 1), ("plain", 3, 3, 17, 7, 13), ("plain", 1, 64, 64, 5, 67), ("plain", 3, 65, 63, 7, 13),
       ("plain", 1, 130, 15, 16, 16), ("plain", 3, 17, 3, 63, 61), ("plain", 2, 1, 130, 33, 33), ("plain", 3, 15, 65, 3, 5),
       ("up", 1, 3, 1, 2, 7), ("up", 3, 17, 64, 7, 13), ("up", 1, 63, 130, 4, 4), ("up", 3, 64, 17, 8, 8), ("up", 1, 3, 3, 33, 31),
       ("up", 3, 130, 65, 5, 6),
       ("1x1", 1, 1, 1, 1, 1), ("1x1", 3, 3, 96, 7, 13), ("1x1", 1, 96, 130, 5, 67), ("1x1", 3, 17, 15, 63, 61),
       ("1x1", 1, 130, 130, 16, 16), ("1x1", 2, 65, 1, 3, 5), ("1x1", 1, 3, 17, 61, 67),
       ("pad2", 1, 3, 17, 7, 13), ("pad2", 3, 64, 65, 5, 6), ("pad2", 1, 15, 1, 33, 33),
       ("step0", 3, 17, 3, 7, 13), ("step0", 1, 65, 64, 4, 9), ("step0", 1, 1, 15, 63, 61),
       # the product layers at 4^2 and 8^2
       ("plain", 1, 512, 512, 4, 4), ("plain", 3, 512, 512, 8, 8), ("up", 1, 512, 512, 4, 4), ("up", 3, 256, 256, 8, 8)]
# (case, with s, with g_d): s on two of every three, g_d on every sample-3 case and every other one besides
WGRAD_CASES = [(c, i % 3 != 2, c[1] == 3 or i % 2 == 0) for i, c in enumerate(_WG)]

# (N, C, HW)
MOD_CASES = [(1, 1, 1), (3, 3, 7), (1, 17, 255), (3, 130, 256), (1, 15, 257), (3, 17, 4099), (1, 1, 4099), (3, 130, 1), (2, 65, 7),
             (1, 512, 64)]

# (N, C, HW, act, alpha, gain, clamp, dscale, g_out aliases g_y, want_noise)
BIAS_ACT_CASES = [(1, 1, 1, 1, 0.2, float(np.sqrt(2)), None, False, False, True),
                  (3, 15, 7, 1, 0.3, 1.7, None, True, False, True),
                  (2, 17, 255, 0, 0.2, 1.0, 0.5, False, True, True),
                  (3, 96, 257, 1, 0.1, 0.9, 0.75, True, True, True),
                  (1, 96, 16, 1, 0.2, float(np.sqrt(2)), 256.0, True, False, True),
                  (3, 1, 300, 0, 0.0, 2.5, 1.0, True, False, True),
                  (1, 17, 4099, 1, 0.05, 1.3, 1.0, False, False, True),
                  (3, 16, 5, 1, 0.25, 1.0, None, False, True, False),
                  (1, 130, 33, 0, 0.0, 1.0, None, True, False, True),
                  (3, 64, 64, 1, 0.2, float(np.sqrt(2)), 0.0, True, False, True)]
