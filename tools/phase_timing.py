#!/usr/bin/env python3
"""Per-section clock table of k_render (csrc/p3d_phase_timing.hpp: the -DP3D_PHASE_TIMING measurement build).

    python tools/phase_timing.py --build            # no GPU needed: compiles build/lib_phase.so (48+48 kernels only)
    python tools/phase_timing.py --build --parent-order   # ... build/lib_phase_parent.so with -DP3D_TILE_ORDER_PARENT (the round-5 tile order)
    python tools/phase_timing.py [-o profiles/X.txt]  # on the GPU: runs the bench view and prints one table per variant
    python tools/phase_timing.py --xcd [-o profiles/X.txt]  # on the GPU: when the last wave of each XCD ends (exact, early-outs on)

P3D_LIB names another measurement library (a build with -DP3D_TILE_ORDER_PARENT, say).

The measurement build is a library of its own; the product library never holds a stamp.  Shares are of the summed wave
lifetimes; "ticks/wave" are shader cycles per wave WITH the stamps' own cost (~10 %), so compare shares and ratios, not
milliseconds.
"""
import argparse
import ctypes
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
LIB = os.path.join(ROOT, "build", "lib_phase.so")
SECTIONS = ["weights->LDS", "stratified", "coarse loop", "cdf", "draws", "sort", "merge pre-pass", "final: select/skip", "final: decode",
            "final: march+composite", "outputs"]
N_SLOTS = len(SECTIONS) + 2  # + waves, lifetime


def build(parent_order=False):
    """The render unit compiled with the switch (one fine-depth capacity: P3D_ONLY_NF=48), linked with the product's other objects."""
    import importlib
    B = importlib.import_module("panic3d_amd")._build
    objs = [o for o in B._compile_objects() if not os.path.basename(o).startswith("p3d_kernels.hip.")]
    flags = [f for f in B.HIPCC_FLAGS if f != "-shared"] + ["-DP3D_PHASE_TIMING", "-DP3D_ONLY_NF=48"] + (["-DP3D_TILE_ORDER_PARENT"] if parent_order else [])
    lib = LIB.replace(".so", "_parent.so") if parent_order else LIB
    obj = os.path.join(ROOT, "build", "p3d_kernels_phase_parent.o" if parent_order else "p3d_kernels_phase.o")
    subprocess.check_call([B._hipcc()] + flags + ["-c", os.path.join(B.CSRC, "p3d_kernels.hip"), "-o", obj])
    subprocess.check_call([B._hipcc(), "--offload-arch=gfx950", "-fPIC", "-shared"] + objs + [obj, "-o", lib])
    print("built", lib)


def run(out):
    os.environ.setdefault("P3D_LIB", LIB)
    import numpy as np
    import torch
    import panic3d_amd as P
    import p3d_testing as T
    from panic3d_amd import ops
    L = P._lib.lib()
    L.p3d_phase_read.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int, ctypes.c_int]
    dev = torch.device("cuda")
    res, Sc, Sf = 512, 48, 48
    R = res * res
    ro = T.bench_rendering_kwargs(Sc, Sf)
    lines = ["# k_render section table, 512^2 rays x (48+48), library " + L.p3d_build_info().decode()]
    for scene in ("surface", "canonical"):
        planes_np, raw = T.make_bench_scene(scene)
        nhwc = ops.planes_to_nhwc(torch.from_numpy(planes_np).to(dev))
        mlp = ops.prescale_mlp(*(torch.from_numpy(x).to(dev) for x in raw), 1 / np.sqrt(32), 1.0, 1 / np.sqrt(64), 1.0)
        o, d = P.cameras.rays_from_label(P.cameras.camera_label(0.0, 20.0, 1.0, 30.0)[None], res)
        o, d = o.to(dev), d.to(dev)
        g = torch.Generator(device=dev).manual_seed(5)
        jit = torch.rand((1, R, Sc, 1), device=dev, generator=g)
        u = torch.rand((R, Sf), device=dev, generator=g)
        for fast in (False, True):
            for early in (True, False):
                opts = ops.make_opts(ro, early_out=early, fast_color=fast, **T.BENCH_KW)
                for _ in range(2):
                    ops.render(nhwc, o, d, jit, u, mlp, opts, ray_tile_w=res)
                buf = (ctypes.c_ulonglong * N_SLOTS)()
                assert L.p3d_phase_read(buf, N_SLOTS, 1) == N_SLOTS
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                ops.render(nhwc, o, d, jit, u, mlp, opts, ray_tile_w=res)
                e1.record()
                torch.cuda.synchronize()
                assert L.p3d_phase_read(buf, N_SLOTS, 1) == N_SLOTS
                b = list(buf)
                waves, life = max(b[-2], 1), max(b[-1], 1)
                lines.append(f"\n{scene} {'tolerance' if fast else 'exact'} early_out={early}: {e0.elapsed_time(e1):.2f} ms with stamps, "
                             f"{waves} waves, {life / waves:.0f} ticks/wave")
                for name, v in zip(SECTIONS, b):
                    lines.append(f"  {name:24s} {v / waves:10.0f} ticks/wave  {v / life:6.3f}")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if out:
        with open(out, "w") as f:
            f.write(text)


def run_xcd(out, launches=3):
    """Per XCD (blockIdx.x % 8): when its last wave ended, from the launch's first wave start, on the device-wide 100 MHz clock."""
    os.environ.setdefault("P3D_LIB", LIB)
    import numpy as np
    import torch
    import panic3d_amd as P
    import p3d_testing as T
    from panic3d_amd import ops
    L = P._lib.lib()
    L.p3d_phase_read_waves.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int]
    dev = torch.device("cuda")
    res, Sc, Sf = 512, 48, 48
    R = res * res
    nwaves = R // 32
    ro = T.bench_rendering_kwargs(Sc, Sf)
    lines = ["# k_render per-XCD finish times, 512^2 rays x (48+48), exact, early-outs on, library " + L.p3d_build_info().decode()
             + " (" + os.path.basename(os.environ["P3D_LIB"]) + ")",
             "# finish: last wave end of the XCD's blocks (b % 8) after the launch's first wave start, us, WITH the stamps' cost;",
             "# busy: summed wave lifetimes of the XCD over the 256 wave slots it has (32 CUs x 8), us"]
    for scene in ("surface", "canonical"):
        planes_np, raw = T.make_bench_scene(scene)
        nhwc = ops.planes_to_nhwc(torch.from_numpy(planes_np).to(dev))
        mlp = ops.prescale_mlp(*(torch.from_numpy(x).to(dev) for x in raw), 1 / np.sqrt(32), 1.0, 1 / np.sqrt(64), 1.0)
        o, d = P.cameras.rays_from_label(P.cameras.camera_label(0.0, 20.0, 1.0, 30.0)[None], res)
        o, d = o.to(dev), d.to(dev)
        g = torch.Generator(device=dev).manual_seed(5)
        jit = torch.rand((1, R, Sc, 1), device=dev, generator=g)
        u = torch.rand((R, Sf), device=dev, generator=g)
        opts = ops.make_opts(ro, early_out=True, fast_color=False, **T.BENCH_KW)
        for _ in range(2):
            ops.render(nhwc, o, d, jit, u, mlp, opts, ray_tile_w=res)
        ratios = []
        for it in range(launches):
            ops.render(nhwc, o, d, jit, u, mlp, opts, ray_tile_w=res)
            torch.cuda.synchronize()
            buf = (ctypes.c_ulonglong * (4 * nwaves))()
            assert L.p3d_phase_read_waves(buf, nwaves) == nwaves
            w = np.frombuffer(buf, dtype=np.uint64).reshape(nwaves, 4).astype(np.int64)
            t0, t1, x, xcc = w[:, 0], w[:, 1], w[:, 2] % 8, w[:, 3]
            start = t0.min()
            fin = np.array([(t1[x == k].max() - start) / 100.0 for k in range(8)])
            busy = np.array([(t1[x == k] - t0[x == k]).sum() / 100.0 / 256 for k in range(8)])
            ids = [sorted(set(xcc[x == k].tolist())) for k in range(8)]
            ratios.append(fin.max() / fin.mean())
            lines.append(f"\n{scene} launch {it}: finish max/mean {fin.max() / fin.mean():.4f}  (max {fin.max():.1f} us, mean {fin.mean():.1f} us, "
                         f"min {fin.min():.1f} us);  busy max/mean {busy.max() / busy.mean():.4f}")
            lines.append("  b % 8        " + " ".join(f"{k:8d}" for k in range(8)))
            lines.append("  finish us    " + " ".join(f"{v:8.1f}" for v in fin))
            lines.append("  busy us      " + " ".join(f"{v:8.1f}" for v in busy))
            lines.append("  XCC_ID seen  " + " ".join(f"{','.join(map(str, i)):>8s}" for i in ids))
        lines.append(f"{scene}: finish max/mean over {launches} launches: median {sorted(ratios)[len(ratios) // 2]:.4f}")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if out:
        with open(out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--build", action="store_true")
    ap.add_argument("--parent-order", action="store_true")
    ap.add_argument("--xcd", action="store_true")
    ap.add_argument("-o", "--out")
    a = ap.parse_args()
    build(a.parent_order) if a.build else run_xcd(a.out) if a.xcd else run(a.out)
