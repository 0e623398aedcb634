#!/usr/bin/env python3
"""Timing of the point-to-mesh distance (include/p3d_metrics.h) at the evaluation's size: 10 000 sample points against
the marching-cubes mesh of a 512^3 volume, both directions; prints one JSON line and writes it to profiles/metrics_bench.json.

The two meshes are extracted on the device from an analytic density (a sphere with lobes, two phases), so no checkpoint is needed and
the face count is of the real order.  Per direction: the median (and the spread) over --repeats windows of --calls calls, timed with
HIP events after a warm-up, ours with culling off and with culling on (the Morton sort and the un-permute included), and the yardstick
— a chunked torch composition of the same formulas (torch_point_mesh_d2 below) on the same GPU — the three alternating
window by window.  The composition moves every intermediate through memory and takes seconds per direction, so it is timed on the
first --yardstick-faces faces and reported as pairs per second; its time for the whole mesh is that rate extrapolated.

Reported: milliseconds, (point, face) pairs per second, and — without culling, where every pair is computed — the fraction of the
157.3 TFLOP/s fp32 vector peak at FLOPS_PER_PAIR flops per pair (the contract's operations with the face term always counted, an fma
as two).  geometry_metrics is timed end to end
(sampling, both directions, the reductions) with the default culling.

    python tools/bench_metrics.py [--repeats 7] [--calls 3] [--resolution 512] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

PEAK_FLOPS = 157.3e12
# 18 subtractions (ab, bc, ca, ap, bp, cp); per segment: two dots of 5, a division, two clamps, three fmas, = 19; the face term: three
# cross + dot of 9 + 5, n.ap 5, h*h/nn 2; three minimums
FLOPS_PER_PAIR = 18 + 3 * 19 + 3 * 14 + 7 + 3
BOX = 0.7


def torch_point_mesh_d2(points, verts, faces, chunk=2048):
    """The contract's formulas (include/p3d_metrics.h) as a chunked torch composition (float32, plain * and +, no fused kernels): dist2
    [Q] and face [Q] of points against the mesh, `chunk` faces at a time.  Same formulas, not the same bits (no fma)."""
    dot = lambda u, v: (u * v).sum(-1)
    best = torch.full((points.shape[0],), float("inf"), device=points.device)
    arg = torch.zeros((points.shape[0],), dtype=torch.long, device=points.device)
    p = points[:, None, :]
    for lo in range(0, faces.shape[0], chunk):
        tri = verts[faces[lo:lo + chunk].long()]
        a, b, c = tri[None, :, 0], tri[None, :, 1], tri[None, :, 2]

        def seg(a, b):
            ab, ap = b - a, p - a
            den = dot(ab, ab)
            t = torch.where(den > 0, (dot(ab, ap) / den).clamp(0, 1), torch.zeros_like(den))
            r = ap - t[..., None] * ab
            return dot(r, r)
        ab, ac, bc, ca = b - a, c - a, c - b, a - c
        n = torch.linalg.cross(ab, ac)
        nn = dot(n, n)
        ap = p - a
        inside = (nn > 0) & (dot(torch.linalg.cross(ab.expand_as(ap), ap), n) > 0) & (dot(torch.linalg.cross(bc.expand_as(ap), p - b), n) > 0) \
            & (dot(torch.linalg.cross(ca.expand_as(ap), p - c), n) > 0)
        h = dot(n, ap)
        face = torch.where(inside, h * h / nn, torch.full_like(h, float("inf")))
        d = torch.minimum(torch.minimum(seg(a, b), seg(b, c)), torch.minimum(seg(c, a), face))
        m, i = d.min(1)
        better = m < best
        best = torch.where(better, m, best)
        arg = torch.where(better, i + lo, arg)
    return best, arg


def window_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def lobed_density(n, phase, dev):
    """0.5 on a sphere of radius 0.31 n voxels whose radius swings by 6 % with the direction; one slab at a time."""
    i = torch.arange(n, device=dev, dtype=torch.float32) - (n - 1) / 2
    vol = torch.empty((n, n, n), device=dev)
    for x in range(n):
        y, z = i[:, None], i[None, :]
        r = (i[x] ** 2 + y ** 2 + z ** 2).sqrt().clamp_min(1e-3)
        ux, uy, uz = i[x] / r, y / r, z / r
        R = 0.31 * n * (1 + 0.06 * torch.sin(9 * ux + phase) * torch.sin(7 * uy + 2 * phase) * torch.cos(8 * uz))
        vol[x] = 0.5 + (R - r) * 0.25
    return vol


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--points", type=int, default=10000)
    ap.add_argument("--yardstick-faces", type=int, default=65536)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_metrics.py needs a GPU"
    import panic3d_amd as P
    P._lib.lib()
    dev = torch.device("cuda")
    M = P.metrics
    meshes = [P.volume.marching_cubes(lobed_density(a.resolution, ph, dev), None, BOX, as_tensors=True) for ph in (0.0, 1.0)]
    gen = torch.Generator(device=dev).manual_seed(0)
    points = [M.sample_points_on_mesh(m["verts"], m["faces"], a.points, gen)[0] for m in meshes]
    res = {"size": {"resolution": a.resolution, "points": a.points, "faces": [int(m["faces"].shape[0]) for m in meshes],
                    "verts": [int(m["verts"].shape[0]) for m in meshes]},
           "repeats": a.repeats, "calls_per_window": a.calls, "flops_per_pair": FLOPS_PER_PAIR, "peak_tflops": PEAK_FLOPS / 1e12,
           "yardstick_faces": a.yardstick_faces, "device": torch.cuda.get_device_name(0),
           "plan": P.ops.point_mesh_plan(a.points, int(meshes[1]["faces"].shape[0]))}
    for name, pts, mesh in (("pred_to_gt", points[0], meshes[1]), ("gt_to_pred", points[1], meshes[0])):
        v, f = mesh["verts"], mesh["faces"]
        fy = f[:a.yardstick_faces].contiguous()
        runs = {"cull_off": lambda: M.point_mesh_squared_distance(pts, v, f, cull=False),
                "cull_on": lambda: M.point_mesh_squared_distance(pts, v, f, cull=True),
                "torch": lambda: torch_point_mesh_d2(pts, v, fy)}
        off, on = runs["cull_off"](), runs["cull_on"]()
        assert all(torch.equal(x, y) for x, y in zip(off, on)), "culling changed a bit"
        d_y, i_y = runs["torch"]()
        d_o = M.point_mesh_squared_distance(pts, v, fy, cull=False)[0]
        for fn in runs.values():
            fn()
        torch.cuda.synchronize()
        t = {k: [] for k in runs}
        for _ in range(a.repeats):  # alternating, so that a disturbance from outside meets all three
            for k, fn in runs.items():
                t[k].append(window_ms(fn, a.calls if k != "torch" else 1))
        med = {k: statistics.median(x) for k, x in t.items()}
        pairs, pairs_y = a.points * f.shape[0], a.points * fy.shape[0]
        row = {"faces": int(f.shape[0]), "max_abs_diff_vs_torch_on_yardstick_faces": float((d_o - d_y).abs().max())}
        for k in ("cull_off", "cull_on"):
            row[k] = {"ms": round(med[k], 4), "min_max_ms": [round(min(t[k]), 4), round(max(t[k]), 4)]}
        row["cull_off"].update(pairs_per_s=round(pairs / med["cull_off"] * 1e3, -6),
                               fraction_of_peak=round(pairs / med["cull_off"] * 1e3 * FLOPS_PER_PAIR / PEAK_FLOPS, 4))
        row["cull_on"]["effective_pairs_per_s"] = round(pairs / med["cull_on"] * 1e3, -6)  # every pair counted, the skipped ones included
        rate_y = pairs_y / med["torch"] * 1e3
        row["torch"] = {"ms_on_yardstick_faces": round(med["torch"], 4), "min_max_ms": [round(min(t["torch"]), 4), round(max(t["torch"]), 4)],
                        "pairs_per_s": round(rate_y, -6), "ms_extrapolated_to_all_faces": round(pairs / rate_y * 1e3, 2)}
        row["ours_over_torch"] = {k: round(med[k] / (pairs / rate_y * 1e3), 4) for k in ("cull_off", "cull_on")}
        res[name] = row

    def e2e():
        return M.geometry_metrics(meshes[0], meshes[1], n_sample=a.points, generator=gen)
    out = e2e()
    torch.cuda.synchronize()
    t = [window_ms(e2e, 1) for _ in range(a.repeats)]
    res["geometry_metrics_end_to_end"] = {"ms": round(statistics.median(t), 3), "min_max_ms": [round(min(t), 3), round(max(t), 3)],
                                          "default_cull": bool(M.DEFAULT_CULL), "cd": float(out["cd"]), "cd_in_voxels": float(out["cd"]) / (BOX / a.resolution),
                                          "f1_005": float(out["f1_005"]), "f1_010": float(out["f1_010"])}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
