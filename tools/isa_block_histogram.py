#!/usr/bin/env python3
"""Opcode histograms of the MFMA-carrying basic blocks of one kernel in a kept gfx950 `.s` (tools/resource_usage.py --keep DIR).

    python tools/isa_block_histogram.py DIR/p3d_kernels-hip-amdgcn-amd-amdhsa-gfx950.s 'k_render<48, false, false, true, false>' [OTHER.s]

A decode step is straight-line code, so each of its parts is one basic block: a block with 32 f32 MFMAs and ~1500 vector instructions
is a density decode (gather + fold + transpose + layer 1 + softplus + sigma row), one with 32 MFMAs and ~450 the colour part (layer 2 +
sigmoids).  Prints, per block with at least `--min-mfma` MFMAs: its label, the VALU / MFMA / SALU / VMEM / LDS counts and the opcodes
(encoding suffixes _e32 / _e64 stripped, _dpp and _sdwa kept).  With a second file the same kernel's blocks of both are printed side
by side, matched in program order, with the difference per opcode (`--other-kernel NAME`: under another name there).
"""
import argparse
import collections
import re
import subprocess


def kernel_blocks(path, kernel):
    """[(label, Counter of opcodes)] of `kernel` (demangled name without arguments), in program order."""
    lines = open(path, errors="replace").read().split("\n")
    starts = [(i, m.group(1)) for i, l in enumerate(lines) for m in [re.match(r"^(_Z\w+|k_\w+):", l)] if m]
    names = subprocess.run(["c++filt"], input="\n".join(n for _, n in starts), capture_output=True, text=True).stdout.split("\n")
    want = [i for (i, _), d in zip(starts, names) if re.sub(r"\(.*", "", d.replace("void ", "")) == kernel]
    if not want:
        raise SystemExit(f"{kernel} not in {path}")
    blocks, label, cur = [], "entry", collections.Counter()
    for l in lines[want[0] + 1:]:
        t = l.split(";")[0].strip()
        if t.startswith(".Lfunc_end"):
            break
        m = re.match(r"^([.\w$]+):", t)
        if m:
            blocks.append((label, cur))
            label, cur = m.group(1), collections.Counter()
            continue
        if not t or t.startswith((".", "//")):
            continue
        op = re.sub(r"_e(32|64)(?=$|_)", "", t.split()[0])
        cur[op] += 1
        if op.startswith(("s_cbranch", "s_branch", "s_endpgm")):
            blocks.append((label, cur))
            label, cur = label + "+", collections.Counter()
    blocks.append((label, cur))
    return [(lb, c) for lb, c in blocks if c]


def classes(c):
    def n(p):
        return sum(v for k, v in c.items() if p(k))
    return dict(VALU=n(lambda k: k.startswith("v_") and not k.startswith("v_mfma")), MFMA=n(lambda k: k.startswith("v_mfma")),
                SALU=n(lambda k: k.startswith("s_")), VMEM=n(lambda k: k.startswith(("buffer_", "global_", "flat_", "scratch_"))),
                LDS=n(lambda k: k.startswith("ds_")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("isa")
    ap.add_argument("kernel")
    ap.add_argument("other", nargs="?")
    ap.add_argument("--min-mfma", type=int, default=16)
    ap.add_argument("--other-kernel", help="the kernel's name in OTHER.s where it differs (a template parameter added or chosen differently)")
    ap.add_argument("-o", "--out")
    a = ap.parse_args()
    files = [(a.isa, a.kernel), (a.other, a.other_kernel or a.kernel)] if a.other else [(a.isa, a.kernel)]
    sides = [[b for b in kernel_blocks(p, k) if classes(b[1])["MFMA"] >= a.min_mfma] for p, k in files]
    out = [f"# {a.kernel}: basic blocks with >= {a.min_mfma} MFMAs, in program order" +
           (f"; left {a.isa}, right {a.other}" + (f" ({a.other_kernel})" if a.other_kernel else "") if a.other else "")]
    if a.other and len(sides[0]) != len(sides[1]):
        out.append(f"# block counts differ ({len(sides[0])} / {len(sides[1])}): matched in order as far as they go")
    for i in range(max(len(s) for s in sides)):
        row = [s[i] if i < len(s) else ("-", collections.Counter()) for s in sides]
        out.append("")
        out.append(f"block {i}: " + " | ".join(f"{lb} " + " ".join(f"{k}={v}" for k, v in classes(c).items()) for lb, c in row))
        for op in sorted(set().union(*(c for _, c in row))):
            cnt = [c.get(op, 0) for _, c in row]
            out.append("  %-28s" % op + " ".join("%6d" % x for x in cnt) + ("  %+d" % (cnt[1] - cnt[0]) if a.other and cnt[1] != cnt[0] else ""))
    text = "\n".join(out) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
