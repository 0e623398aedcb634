#!/usr/bin/env python3
"""Wave-step statistics of k_render's early-outs on the bench view, from the CPU oracle alone (no GPU).

    python tools/oracle_step_stats.py [--scene surface] [--stride 4] [--sc 48 --sf 48]

Renders every `stride`-th 8x4 tile of the 512^2 bench view with oracle.render(..., dumps=True), the rays of a tile in the
kernel's Morton lane order, and counts decode steps per wave the way the kernel takes them:

* a coarse step runs if any lane of the wave is neither cropped (by position) nor dead (transmittance < 1e-60);
* the final pass runs max over the lanes of the merged samples that are alive and not known-masked (cropped, or a coarse
  sample that decoded to the masked density).

It also prints the final pass's lane occupancy (decodes / (steps x 32)) and what perfect packing of a wave's decodes would
give, i.e. the ceiling of any scheme that regroups lanes; and the final wave-steps that carry at least one live unmasked lane
(the steps whose colour part runs), the colour samples per wave and their lane occupancy: what a shortcut that needs all 32
lanes of a step to agree can hope for.  Stride 4 on the surface scene at 48+48: 23.0 coarse + 48.5 final
wave-steps of 144 = 0.497 (the kernel's own counter, decode_steps_executed_frac: 0.498), occupancy 0.85, packed 41.6.
"""
import argparse
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import p3d_testing as T  # noqa: E402
from oracle import oracle  # noqa: E402


def tile_steps(scene="surface", stride=4, Sc=48, Sf=48, res=512, azim=20.0):
    """The view's tiles (tx, ty) with tx % stride == ty % stride == 0, each rendered as one wave: returns (ty, tx, coarse wave-steps,
    final wave-steps, decodes of the final pass, fraction of the coarse samples cropped, per-tile colour statistics of the final pass:
    colour_steps, colour_samples, coarse_again), arrays over those tiles in row-major order."""
    spec = importlib.util.spec_from_file_location("p3d_cameras", os.path.join(ROOT, "panic3d-anime-reconstruction_amd", "cameras.py"))
    cams = importlib.util.module_from_spec(spec)  # (the cameras alone: the package itself would load the HIP library)
    spec.loader.exec_module(cams)
    planes, raw = T.make_bench_scene(scene)
    o, d = cams.rays_from_label(cams.camera_label(0.0, azim, 1.0, 30.0)[None], res)
    o, d = o.reshape(res, res, 3).numpy(), d.reshape(res, res, 3).numpy()
    idx, tys, txs = [], [], []
    for ty in range(0, res // 4, stride):
        for tx in range(0, res // 8, stride):
            tys.append(ty)
            txs.append(tx)
            for j in range(32):  # k_render's lane order inside an 8x4 tile
                lx, ly = (j & 1) | ((j >> 1) & 6), ((j >> 1) & 1) | ((j >> 3) & 2)
                idx.append((ty * 4 + ly, tx * 8 + lx))
    idx = np.array(idx)
    oo = np.ascontiguousarray(o[idx[:, 0], idx[:, 1]][None])
    dd = np.ascontiguousarray(d[idx[:, 0], idx[:, 1]][None])
    NR, W = oo.shape[1], oo.shape[1] // 32
    rng = np.random.default_rng(0)
    jit, u = rng.random((1, NR, Sc), dtype=np.float32), rng.random((NR, Sf), dtype=np.float32)
    opts = oracle.make_opts(T.bench_rendering_kwargs(Sc, Sf), **T.BENCH_KW)
    D = oracle.render(planes, oo, dd, jit, u, oracle.prescale_mlp(*raw), opts, dumps=True)[4]
    tc, sc, tf, sf, perm = D["depths_coarse"], D["sigma_coarse"], D["depths_fine"], D["sigma_fine"], D["perm"]

    def cropped(t):
        px, pz = oo[0, :, None, 0] + t * dd[0, :, None, 0], oo[0, :, None, 2] + t * dd[0, :, None, 2]
        return (np.abs(px) > opts.crop_limit) | (np.abs(pz) > opts.crop_limit)

    def transmittance_before(t, s):  # of every sample: the marcher of ray_marcher.py in binary64
        dens = np.logaddexp(0, ((s[:, :-1] + s[:, 1:]) * 0.5).astype(np.float64) - 1)
        alpha = 1 - np.exp(-dens * (t[:, 1:] - t[:, :-1]))
        return np.concatenate([np.ones((t.shape[0], 1)), np.cumprod(1 - alpha + 1e-10, axis=1)], axis=1)

    live_c = ~(cropped(tc) | (transmittance_before(tc, sc) < 1e-60))
    steps_c = live_c.reshape(W, 32, Sc).any(axis=1).sum(axis=1)
    tm = np.take_along_axis(np.concatenate([tc, tf], axis=1), perm, axis=1)
    sm = np.take_along_axis(np.concatenate([sc, sf], axis=1), perm, axis=1)
    known = cropped(tm) | ((perm < Sc) & (sm <= -999))
    need = (transmittance_before(tm, sm) >= 1e-60) & ~known
    n_l = need.sum(axis=1).reshape(W, 32)
    # the colour part of a final step runs if a lane that decodes in it finds its sample unmasked.  A lane's k-th needed sample is
    # decoded in the wave's k-th final step: bring every ray's needed samples to the front, in merged order
    order = np.argsort(~need, axis=1, kind="stable")
    colour = np.take_along_axis(need & (sm > -999), order, axis=1)  # [ray, step]: the lane decodes an unmasked sample in this step
    again = np.take_along_axis(need & (sm > -999) & (perm < Sc), order, axis=1)  # ... which the coarse pass had decoded already
    colour_w = colour.reshape(W, 32, -1)
    stats = dict(colour_steps=colour_w.any(axis=1).sum(axis=1), colour_samples=colour_w.sum(axis=(1, 2)),
                 coarse_again=again.reshape(W, -1).sum(axis=1))
    return np.array(tys), np.array(txs), steps_c, n_l.max(axis=1), n_l.sum(axis=1), float(cropped(tc).mean()), stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="surface")
    ap.add_argument("--stride", type=int, default=4)
    ap.add_argument("--sc", type=int, default=48)
    ap.add_argument("--sf", type=int, default=48)
    a = ap.parse_args()
    Sc, Sf = a.sc, a.sf
    _, _, steps_c, mx, tot, crop, st = tile_steps(a.scene, a.stride, Sc, Sf)
    W, S = len(mx), Sc + Sf
    print(f"{a.scene} {Sc}+{Sf}, {W} waves ({W * 32} rays): coarse samples cropped {crop:.3f}")
    print(f"coarse wave-steps {steps_c.mean():.1f} of {Sc}; final wave-steps {mx.mean():.1f} of {S}; "
          f"total {(steps_c + mx).mean():.1f} of {Sc + S} = {(steps_c + mx).mean() / (Sc + S):.4f}")
    print(f"final pass: lane occupancy {tot.sum() / (mx.sum() * 32):.3f}; perfectly packed {np.ceil(tot / 32).mean():.1f} wave-steps")
    # what a wave-uniform shortcut of the walk can hope for: the final steps in which NO lane holds a live, unmasked sample
    cs, cn = st["colour_steps"], st["colour_samples"]
    print(f"final wave-steps with at least one live unmasked lane (the colour part runs) {cs.mean():.1f} of {mx.mean():.1f}; "
          f"colour samples per wave {cn.mean():.0f}, lane occupancy {cn.sum() / (cs.sum() * 32):.3f}; "
          f"{st['coarse_again'].mean():.0f} of them coarse samples decoded a second time")


if __name__ == "__main__":
    main()
