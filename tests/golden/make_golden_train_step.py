#!/usr/bin/env python3
"""Golden vectors for training through the mapping network and the front-view paste, produced by the REFERENCE ITSELF on CPU (its
source tree imported unmodified from the directory P3D_REFERENCE_DIR names).  Writes only arrays: tests/golden/mapping_grad.npz and
tests/golden/train_step.npz.

    P3D_REFERENCE_DIR=<checkout of the reference> python tests/golden/make_golden_train_step.py [mapping] [paste]

kornia is not installed where this runs: `kornia.filters.sobel` is stood in by this package's paste.sobel_magnitude (kornia 0.6.5
semantics), exactly as make_golden_synthesis.py does, so train_step.npz pins the paste GLUE and its autograd, not kornia.
"""
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("P3D_REFERENCE_DIR")
if not REF:
    sys.exit("set P3D_REFERENCE_DIR to a checkout of the reference")
os.environ.setdefault("PROJECT_DN", REF)
os.environ.setdefault("PROJECT_NAME", "x")
sys.path[:0] = [REF]
sys.path.append(os.path.join(REF, "_train", "eg3dc", "src"))
sys.path.append(os.path.dirname(HERE))  # tests/: the case definitions the tests share with this script
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))  # the package (paste.sobel_magnitude)
sys.modules.setdefault("kornia", types.ModuleType("kornia"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import train_step_cases as TC  # noqa: E402


def save(name, **arrs):
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **arrs)
    print(f"{name}: {os.path.getsize(path) / 1024:.0f} KiB")
    assert os.path.getsize(path) < 1 << 20


def mapping_case():
    """TriPlaneGenerator.mapping_zplus of the reference under autograd: cond_mode resnetcond_8, c_dim 25, 2 and 8 mapping layers,
    batch 3, one z per w slot; truncation 0.7 with a cutoff, and two update_emas calls.  Parameters, inputs and the cotangent are
    re-drawn by the test from the same seeds (train_step_cases); the fixture stores the reference's ws, w_avg and gradients (the big
    weight gradients as every 8th row and column, next to their full L2 norm)."""
    from training.triplane import TriPlaneGenerator
    out = {}
    for L in TC.MAPPING_LAYERS:
        G = TC.fill_mapping(TriPlaneGenerator(**TC.mapping_kw(L)).eval(), 100 + L)
        inp = TC.mapping_inputs(G.backbone.num_ws, 200 + L)
        leaves = {k: v.clone().requires_grad_(True) for k, v in inp.items() if k in ("zs", "feats")}
        ws = G.mapping_zplus(leaves["zs"], inp["c"], {"resnet_feats": leaves["feats"]}, truncation_psi=TC.PSI, truncation_cutoff=TC.CUTOFF)
        (ws * inp["g_ws"]).sum().backward()
        p = f"L{L}_"
        out[p + "ws"] = ws.detach().numpy()
        out[p + "g_zs"], out[p + "g_feats"] = leaves["zs"].grad.numpy(), leaves["feats"].grad.numpy()
        for n, q in G.backbone.mapping.named_parameters():
            out[p + "g_" + n.replace(".", "__")] = TC.sub(q.grad).numpy()
            out[p + "n_" + n.replace(".", "__")] = np.float64(q.grad.double().norm())
        out[p + "checksum"] = np.float64(TC.checksum(G, inp))
        G.zero_grad()
        for i in range(2):  # two training-style calls: w_avg moves twice
            inp2 = TC.mapping_inputs(G.backbone.num_ws, 300 + L + i)
            z2 = {k: inp2[k].clone().requires_grad_(True) for k in ("zs", "feats")}
            ws2 = G.mapping_zplus(z2["zs"], inp2["c"], {"resnet_feats": z2["feats"]}, update_emas=True)
        (ws2 * inp2["g_ws"]).sum().backward()
        out[p + "emas_ws"], out[p + "emas_w_avg"] = ws2.detach().numpy(), G.backbone.mapping.w_avg.numpy().copy()
        out[p + "emas_g_zs"] = z2["zs"].grad.numpy()
        out[p + "emas_g_fc0_weight"] = TC.sub(G.backbone.mapping.fc0.weight.grad).numpy()
    save("mapping_grad.npz", **out)


def paste_case():
    """The reference's G.f on the generator of syn_triplane_f.npz, an orthographic and a perspective view, then the reference's
    paste_front under autograd at the paste's inputs (grad_sample on) with the loss of train_step_cases.paste_loss.  The pre-paste
    image handed to the paste is the 4x bilinear up-sampling of every 4th pixel of the reference's super-resolved image: the test
    rebuilds it bit for bit from 1/16 of the data (a 512^2 x 2 image does not fit a fixture)."""
    from training import triplane as rt
    import panic3d_amd.paste as my_paste
    import kornia
    kornia.filters = types.SimpleNamespace(sobel=my_paste.sobel_magnitude)
    g = dict(np.load(os.path.join(HERE, "syn_triplane_f.npz")))
    G = rt.TriPlaneGenerator(**TC.TRI_KW).eval()
    G.load_state_dict({k[3:].replace("__", "."): torch.from_numpy(v) for k, v in g.items() if k.startswith("sd_")}, strict=True)
    G.set_force_sigmoid(True)
    draws = []
    o_rl, o_r = torch.rand_like, torch.rand

    def rand_like(t, *a, **k):
        r = o_rl(t, *a, **k); draws.append(r.clone()); return r

    def rand(*a, **k):
        r = o_r(*a, **k); draws.append(r.clone()); return r

    x = TC.paste_x(torch.device("cpu"))
    torch.rand_like, torch.rand = rand_like, rand
    try:
        torch.manual_seed(10)
        with torch.no_grad():
            out = G.f(x)
        sub4 = out["image"][..., ::4, ::4].contiguous()
        ret = {"image": TC.prepaste_from_sub4(sub4).requires_grad_(True), "image_xyz": out["image_xyz"].clone().requires_grad_(True),
               "image_weights": out["image_weights"].clone().requires_grad_(True), "normalize_images": out["normalize_images"]}
        occ = {}
        real_occ = rt.get_front_occlusion
        rt.get_front_occlusion = lambda *a, **k: occ.setdefault("occ", real_occ(*a, **k))
        try:
            paste = rt.paste_front(G, x, ret, **TC.PASTE_PARAMS)
        finally:
            rt.get_front_occlusion = real_occ
    finally:
        torch.rand_like, torch.rand = o_rl, o_r
    assert len(draws) == 4
    TC.paste_loss(paste["image"], ret["image_weights"], ret["image_xyz"]).backward()
    m = paste["mask"]
    print("train_step fixture: mask mean %.3f per view %s, weights mean %.3f" % (float(m.mean()), [round(float(v.mean()), 3) for v in m],
                                                                                   float(out["image_weights"].mean())))
    arrs = dict(image_sub4=sub4.numpy(), image_xyz=out["image_xyz"].numpy(), image_weights=out["image_weights"].numpy(),
                ray_origins=x["force_rays"]["ray_origins"].numpy(), ray_directions=x["force_rays"]["ray_directions"].numpy(),
                ws=x["ws"].numpy(), occ=occ["occ"].numpy(), mask=m.numpy(), paste_sub4=paste["paste"].detach()[..., ::4, ::4].contiguous().numpy(),
                out_sub4=paste["image"].detach()[..., ::4, ::4].contiguous().numpy(),
                g_prepaste_sub4=ret["image"].grad[..., ::4, ::4].contiguous().numpy(), g_prepaste_norm=np.float64(ret["image"].grad.double().norm()),
                g_xyz=ret["image_xyz"].grad.numpy(), g_weights=ret["image_weights"].grad.numpy())
    for i, dr in enumerate(draws):
        arrs[f"draw{i}"] = dr.numpy()
    save("train_step.npz", **arrs)


if __name__ == "__main__":
    torch.set_num_threads(8)
    which = sys.argv[1:] or ["mapping", "paste"]
    if "mapping" in which:
        mapping_case()
    if "paste" in which:
        paste_case()
