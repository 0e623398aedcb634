#!/usr/bin/env python3
"""Writes tests/golden/torgb_plans.json: the launch of every p3d_torgb_f32 call of a sweep of (N, I, O, H, W), by the rule the launcher
held in its own body before csrc/p3d_torgb_plan.hpp existed, restated here in Python (integer arithmetic only).  The rows were first
recorded from that rule and the plan header must reproduce them (tests/test_torgb_cases_cpu.py); run this again to extend the sweep —
an existing row that changes means this restatement, not the header, has drifted.

A row: N, I, O, H, W, then the P3D_E_* code, or the instantiation, grid x, y, z and the dynamic LDS bytes.  Of the rows that a
non-positive size refuses (P3D_E_ARG) every sixteenth is kept."""
import json
import os

E_ARG, E_RANGE, KC = -1, -2, 64


def launch(N, I, O, H, W):
    if min(N, I, O, H, W) <= 0:
        return [E_ARG]
    if O > 96 or I > 1024 or I * H * W * 4 >= 1 << 31:
        return [E_RANGE]
    HW, MT = H * W, 1 if O <= 32 else 3
    ks = N * ((HW + 127) // 128) < 512
    ms = ks and MT == 3 and N * ((HW + 31) // 32) * 3 <= 1024
    pre = ms and I <= 8 * KC
    lds = (2 * KC * 32 * (1 if ms else MT) + (8 * KC if pre else (I + 63) // 64 * 64)) * 4
    if lds > 64 * 1024:
        return [E_RANGE]
    b = lambda v: "true" if v else "false"  # noqa: E731
    name = f"k_torgb<1,{b(ks)}>" if MT == 1 else "k_torgb<1,true,true,true>" if pre else "k_torgb<1,true,true>" if ms else f"k_torgb<3,{b(ks)}>"
    return [name, (HW + 31) // 32 if ks else (HW + 127) // 128, N, 3 if ms else 1, lds]


def sweep():
    Ns, Is, Os = (0, 1, 2, 3, 4, 8, 16), (0, 1, 63, 64, 65, 129, 512, 513, 1024, 1025), (0, 1, 3, 32, 33, 96, 97)
    HWs = ((0, 4), (4, 0), (1, 1), (4, 4), (6, 10), (16, 16), (32, 32), (33, 31), (58, 62), (59, 62), (64, 64), (90, 91), (90, 92), (128, 128),
           (181, 181), (256, 256), (255, 257), (512, 512), (724, 724), (1024, 1024))
    shapes = [(N, I, O, H, W) for N in Ns for I in Is for O in Os for H, W in HWs]
    # the dispatch edges: PX tiles 511 / 512, 3 * KS tiles 1023 / 1026, and their neighbours
    for O in (3, 40):
        for I in (10, 515):
            shapes += [(1, I, O, 1, hw) for hw in range(128 * 510, 128 * 513 + 1, 64)]
            shapes += [(n, I, O, 90, 91) for n in range(1, 10)]
            for t in range(339, 345):
                shapes += [(1, I, O, 1, 32 * t), (1, I, O, 1, 32 * t - 31)]
            for n in range(1, 5):
                shapes += [(n, I, O, 58, 62), (n, I, O, 59, 62)]
    rows, nth = [], 0
    for s in shapes:
        r = launch(*s)
        if r == [E_ARG]:
            nth += 1
            if nth % 16:
                continue
        rows.append(list(s) + r)
    return rows


if __name__ == "__main__":
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "torgb_plans.json")
    with open(out, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in sweep()) + "\n]\n")
    print(out)
