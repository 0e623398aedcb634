#!/usr/bin/env python3
"""Modelled load of the eight XCDs under k_render's tile orders, from the CPU oracle alone (no GPU).

    python tools/xcd_load_model.py [--scene surface] [--azim 20] [--res 512] [--views 1] [--rules 16,8,1,0 16,8,7,0]
    python tools/xcd_load_model.py --sweep [-o profiles/X.txt]

Hardware places block b on XCD b % 8 and the launch ends when the slowest XCD ends.  The model prices a tile (= one wave) as

    cycles = fixed + coarse wave-steps x (coarse loop / mean coarse steps) + final wave-steps x (final decode / mean final steps)

with the wave-steps counted from the oracle the way tools/oracle_step_stats.py counts them (every `stride`-th tile in x and y;
a tile in between takes the count of the sampled tile of its stride x stride cell) and the three constants read from the
"<scene> exact early_out=True" table of a section-table file (tools/phase_timing.py), calibrated on the bench view (azimuth 20,
512^2), whose mean steps the same oracle run gives.  Which tile an XCD gets comes from tests/tile_order_host.cpp, i.e. from the
functions the kernel itself calls (csrc/p3d_render_plan.hpp): the round-5 order ("parent"), the plan's choice, and any --rules.

--sweep: both bench scenes at azimuths 0, 30 ... 330 at 512^2, then the surface scene as 4 views of 256^2 (c2's launch shape, views at
azimuths 0 / 30 / 60 / 90; bench.py's c2 renders a random backbone's planes, which only the GPU has) and at 1024^2.
Everything this prints is MODELLED; the measured counterpart is tools/phase_timing.py --xcd.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
from host_build import compile_host  # noqa: E402
import oracle_step_stats as O  # noqa: E402

PHASE_FILE = os.path.join(ROOT, "profiles", "r11_phase_branch.txt")
SC, SF = 48, 48
_steps, _orders, _exe = {}, {}, []


def section_table(path, scene):
    """{section: ticks/wave} of the '<scene> exact early_out=True' table."""
    tab, on = {}, False
    with open(path) as f:
        for line in f:
            if not line.startswith(" "):
                on = line.startswith(f"{scene} exact early_out=True")
            elif on:
                m = re.match(r"\s+(.*?)\s+(\d+) ticks/wave", line)
                tab[m.group(1)] = float(m.group(2))
    assert "coarse loop" in tab and "final: decode" in tab, (path, scene)
    return tab


def steps(scene, azim, res, stride):
    key = (scene, azim, res, stride)
    if key not in _steps:
        _steps[key] = O.tile_steps(scene, stride, SC, SF, res, azim)[:4]
    return _steps[key]


def costs(scene, phase_file, stride):
    """(fixed, per coarse step, per final step) in shader cycles, calibrated on the bench view."""
    tab = section_table(phase_file, scene)
    _, _, sc, sf = steps(scene, 20.0, 512, stride)
    fixed = sum(v for k, v in tab.items() if k not in ("coarse loop", "final: decode"))
    return fixed, tab["coarse loop"] / sc.mean(), tab["final: decode"] / sf.mean()


def tile_order(N, res, parent, rule):
    """(the order's parameters, block, view, tx, ty of every wave), from the host program."""
    key = (N, res, parent, rule)
    if key in _orders:
        return _orders[key]
    if not _exe:
        import pathlib
        _exe.append(compile_host(pathlib.Path(tempfile.mkdtemp(prefix="tile_order")), "tile_order_host.cpp"))
    pw, ph, xa, xs = rule if rule else (0, 0, 0, 0)
    req = f"m {N} {res * res} {res} {SC} {SF} 0 0 {int(parent)} {pw} {ph} {xa} {xs}\n"
    out = subprocess.run([_exe[0]], input=req, capture_output=True, text=True, check=True).stdout
    first, rest = out.split("\n", 1)
    head = first.split()
    assert head[0] == "order", first
    w = np.array(rest.split(), dtype=np.int64).reshape(-1, 6)
    _orders[key] = dict(zip(("swz", "blocked", "pieces", "pw", "ph", "xa", "xs"), map(int, head[1:8]))), w[:, 0], w[:, 3], w[:, 4], w[:, 5]
    return _orders[key]


def tile_cost_maps(scene, azims, res, stride, phase_file):
    """[view] -> array [tiles_y, tiles_x] of modelled cycles per tile."""
    fixed, cc, cf = costs(scene, phase_file, stride)
    maps = []
    for az in azims:
        ty, tx, sc, sf = steps(scene, az, res, stride)
        m = np.zeros((res // 4 // stride, res // 8 // stride))
        m[ty // stride, tx // stride] = fixed + cc * sc + cf * sf
        maps.append(np.kron(m, np.ones((stride, stride))))
    return maps


def xcd_loads(maps, N, res, parent, rule):
    head, blk, n, tx, ty = tile_order(N, res, parent, rule)
    cost = np.stack(maps)[n, ty, tx]
    return head, np.bincount(blk % 8, weights=cost, minlength=8) / np.bincount(blk % 8, minlength=8)


def report(scene, azims, res, rules, stride, phase_file, verbose=True):
    """One line per order: name, max/mean of the eight XCD loads (and the loads in k cycles per wave when verbose)."""
    maps = tile_cost_maps(scene, azims, res, stride, phase_file)
    rows = []
    for name, parent, rule in [("parent", True, None), ("plan", False, None)] + [(",".join(map(str, r)), False, r) for r in rules]:
        head, loads = xcd_loads(maps, len(azims), res, parent, rule)
        if name == "plan":
            name = "plan({pw},{ph},{xa},{xs})".format(**head) if head["pieces"] else "plan(=parent)"
        elif not parent and not head["pieces"]:
            name += "(=parent)"
        rows.append((name, loads.max() / loads.mean(), loads))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="surface")
    ap.add_argument("--azim", type=float, default=20.0)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--views", type=int, default=1, help="views of one launch, at azimuths azim, azim + 30, ...")
    ap.add_argument("--stride", type=int, default=4)
    ap.add_argument("--rules", nargs="*", default=[], help="pw,ph,a,s: pieces of pw x ph tiles, piece (column c, row r) dealt to XCD (a * c + r + s * (r // 8)) % 8")
    ap.add_argument("--phase-file", default=PHASE_FILE)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("-o", "--out")
    a = ap.parse_args()
    rules = [tuple(int(v) for v in r.split(",")) for r in a.rules]
    lines = [f"# MODELLED per-XCD loads of k_render (tools/xcd_load_model.py): oracle wave-steps of every {a.stride}th tile x the section costs of",
             f"# {os.path.relpath(a.phase_file, ROOT)}; max/mean of the eight XCD sums per tile order; rules pw,ph,a,s = pw x ph-tile pieces dealt by (a * column + row + s * (row // 8)) % 8"]
    if not a.sweep:
        azims = [a.azim + 30.0 * v for v in range(a.views)]
        fixed, cc, cf = costs(a.scene, a.phase_file, a.stride)
        lines.append(f"# {a.scene}: cycles/wave = {fixed:.0f} + {cc:.0f} x coarse steps + {cf:.0f} x final steps")
        for name, ratio, loads in report(a.scene, azims, a.res, rules, a.stride, a.phase_file):
            lines.append(f"{a.scene} {a.views} x {a.res}^2 azimuth {a.azim:g}  {name:14s} max/mean {ratio:.4f}   k cycles/wave per XCD: "
                         + " ".join(f"{v / 1e3:.0f}" for v in loads))
    else:
        cases = [(s, [float(az)], 512) for s in ("surface", "canonical") for az in range(0, 360, 30)]
        cases += [("surface", [0.0, 30.0, 60.0, 90.0], 256), ("surface", [20.0], 1024)]
        names, table = None, []
        for scene, azims, res in cases:
            rows = report(scene, azims, res, rules, a.stride, a.phase_file)
            names = names or [r[0] for r in rows]
            table.append([r[1] for r in rows])
            lines.append(f"{scene:9s} {len(azims)} x {res:4d}^2 azimuth {azims[0]:5g}  " + "  ".join(f"{r[0]} {r[1]:.4f}" for r in rows))
            print(lines[-1], flush=True)
        t = np.array(table)
        lines.append("mean over the views             " + "  ".join(f"{n} {v:.4f}" for n, v in zip(names, t.mean(axis=0))))
        lines.append("worst view                      " + "  ".join(f"{n} {v:.4f}" for n, v in zip(names, t.max(axis=0))))
        lines.append("views worse than the parent     " + "  ".join(f"{n} {int((t[:, i] > t[:, 0] + 1e-9).sum())}" for i, n in enumerate(names)))
    text = "\n".join(lines) + "\n"
    if not a.sweep:
        sys.stdout.write(text)
    else:
        sys.stdout.write("\n".join(lines[-3:]) + "\n")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
