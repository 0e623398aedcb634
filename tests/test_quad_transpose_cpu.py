"""CPU: the two cross-lane routes of the quad-cooperative gather (csrc/p3d_decode.hpp, P3D_QUAD_EXCHANGE), emulated in numpy over the four
lanes of a quad from the instruction tables of the header itself:

* p3d_quad_transpose — the two-stage exchange of v_cndmask_b32_dpp (D = vcc ? src1 : src0, src0 read from the lane that quad_perm
  names, the lane mask in VCC) over all 16 registers: out[lane i][4 p + d] == in[lane p][4 i + d] for every i, p, d;
* p3d_fmac_quad16 — v_fmac_f32_dpp with the bilinear weight as its DPP source: folded over the 12 taps in the contract's order and
  transposed, it equals the per-lane fold (each lane its own sample, its own weight) bit for bit;
* the wait states that the compiler does not pad inside an asm statement: no register is read through DPP within two instructions of
  its write, and a statement whose inputs may be fresh opens with s_nop 1.

The statements are read from the header (macro calls, VCC masks, operand lists, the transpose's result list), so an edit of the routing
there is an edit of what runs here.
"""
import os
import re

import numpy as np
import pytest

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "panic3d-anime-reconstruction_amd", "csrc", "p3d_decode.hpp")
PERMS = {"P3D_X1": (1, 0, 3, 2), "P3D_X2": (2, 3, 0, 1)}


def _function(name):
    """the text of the first definition of `name` in the header, up to the brace that closes it at column 0"""
    src = open(HEADER).read()
    m = re.search(r"^P3D_DEV [\w ]+ " + name + r"\(.*?^}", src, re.S | re.M)
    assert m, name
    return m.group(0)


def _statements(text):
    """[(instructions, operands)] of every asm statement: instructions are ('nop',), ('mask_lo' | 'mask_hi', bits), ('sel', D, OWN, PARTNER, perm) or
    ('fmac', F, V, lane), in program order; operands the C++ expressions bound to %0, %1, ..."""
    out = []
    for body in re.findall(r"asm\((.*?)\);", text, re.S):
        code, _, tail = re.sub(r"//[^\n]*", "", body).partition(":")
        ins = []
        for m in re.finditer(r'"s_nop 1|P3D_QMASK\("0x([0-9a-f]{8})"\)|P3D_QSEL\((\d+), (\d+), (\d+), (\w+)\)|P3D_FMAC_Q\((\d+), (\d+), (\d)\)', code):
            if m.group(0).startswith('"s_nop'):
                ins.append(("nop",))
            elif m.group(1):
                ins += [("mask_lo", int(m.group(1), 16)), ("mask_hi", int(m.group(1), 16))]
            elif m.group(2):
                ins.append(("sel", int(m.group(2)), int(m.group(3)), int(m.group(4)), PERMS[m.group(5)]))
            else:
                ins.append(("fmac", int(m.group(6)), int(m.group(7)), int(m.group(8))))
        out.append((ins, re.findall(r'"[+=&]*v"\(([\w.]+)\)', tail)))
    return out


def _reg(expr):
    """'x.sa' -> ('x', 10); 't4' -> ('t4', 0)"""
    m = re.fullmatch(r"(\w+)\.s([0-9a-f])", expr)
    return (m.group(1), int(m.group(2), 16)) if m else (expr, 0)


def fma32(a, b, c):
    """one fp32 fused multiply-add per element (the product is exact in float64; both sides of every comparison go through here)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def run(statement, regs):
    """Execute one asm statement on `regs`: {(name, index): float32[4 lanes]}.  Returns the least distance, in instructions, from a
    write of a register to a DPP read of it inside the statement (None: no such pair), and whether it opens with s_nop 1."""
    ins, ops = statement
    ops = [_reg(e) for e in ops]
    lane = np.arange(4)
    vcc = [0, 0]
    written, least = {}, None
    for n, i in enumerate(ins):
        dpp = None
        if i[0] in ("mask_lo", "mask_hi"):
            vcc[i[0] == "mask_hi"] = i[1]
        elif i[0] == "sel":
            _, d, own, partner, perm = i
            assert vcc[0] == vcc[1] and all((vcc[0] >> (4 * q)) & 0xf == vcc[0] & 0xf for q in range(8)), "the emulation is of ONE quad: every quad of the wave must see the same mask"
            cond = ((vcc[0] >> lane) & 1).astype(bool)
            regs[ops[d]] = np.where(cond, regs[ops[own]], regs[ops[partner]][list(perm)])
            dpp, dst = ops[partner], ops[d]
        elif i[0] == "fmac":
            _, f, v, r = i
            w = ops[-1]
            regs[ops[f]] = fma32(regs[w][[r] * 4], regs[ops[v]], regs[ops[f]])
            dpp, dst = w, ops[f]
        if dpp is not None:
            if dpp in written:
                least = n - written[dpp] if least is None else min(least, n - written[dpp])
            written[dst] = n
    return least, ins[0] == ("nop",)


@pytest.fixture(scope="module")
def transpose():
    text = _function("p3d_quad_transpose")
    (st,) = _statements(text)
    result = re.search(r"return \(f32x16\)\{([^}]*)\}", text).group(1)
    return st, [_reg(e.strip()) for e in result.split(",")]


@pytest.fixture(scope="module")
def fmac():
    sts = _statements(_function("p3d_fmac_quad16"))
    assert len(sts) == 2
    return sts


def quad_transpose(transpose, x):
    """x: float32[4 lanes][16] -> [4 lanes][16], by the header's statement"""
    st, result = transpose
    regs = {("x", c): x[:, c].copy() for c in range(16)}
    for k in range(8):
        regs[(f"t{k}", 0)] = np.full(4, np.nan, np.float32)  # (a temporary read before its write would show)
    hazard = run(st, regs)
    return np.stack([regs[r] for r in result], axis=1), hazard


def test_transpose_is_32_selects_on_constant_masks(transpose):
    (ins, ops), result = transpose
    assert sum(i[0] == "sel" for i in ins) == 32 and len(ops) == 24 and len(result) == 16
    assert [i[1] for i in ins if i[0] == "mask_lo"] == [0x55555555, 0xaaaaaaaa, 0x33333333, 0xcccccccc]
    assert ins[-1] == ("nop",)  # its outputs are MFMA operands


def test_transpose_every_lane_row_and_channel(transpose):
    # a value that names its (lane, register): exact in float32
    x = (100.0 * np.arange(4)[:, None] + np.arange(16)[None, :]).astype(np.float32)
    out, _ = quad_transpose(transpose, x)
    for i in range(4):
        for p in range(4):
            for d in range(4):
                assert out[i, 4 * p + d] == x[p, 4 * i + d], (i, p, d)
    rng = np.random.default_rng(11)
    y = rng.standard_normal((4, 16)).astype(np.float32)
    out, _ = quad_transpose(transpose, y)
    assert np.array_equal(out.reshape(4, 4, 4), y.reshape(4, 4, 4).transpose(1, 0, 2))


def test_wait_states_inside_the_statements(transpose, fmac):
    _, (least, opens_with_nop) = quad_transpose(transpose, np.zeros((4, 16), np.float32))
    assert opens_with_nop and least is not None and least > 2, least  # two wait states: at least two instructions in between
    for st in fmac:
        regs = {_reg(e): np.zeros(4, np.float32) for e in st[1]}
        least, opens_with_nop = run(st, regs)
        assert opens_with_nop and least is None  # the weight is never written inside; it may be fresh from outside


@pytest.mark.parametrize("seed", range(4))
def test_dpp_weighted_fold_equals_the_per_lane_fold(transpose, fmac, seed):
    """12 taps of 4 samples x 16 channels with their weights (some exactly zero, as for a tap outside the plane), folded in the
    contract's order: nw, ne, sw, se per plane; plane 0 + plane 1, + plane 2, x 1/3."""
    rng = np.random.default_rng(seed)
    taps = rng.standard_normal((12, 4, 16)).astype(np.float32)  # [tap][sample][channel of this lane half]
    wgt = rng.uniform(0, 1, (12, 4)).astype(np.float32)
    wgt[rng.integers(0, 12, 5), rng.integers(0, 4, 5)] = 0.0
    third = np.float32(1.0 / 3.0)

    def fold(first, rest):
        X = None
        for k in range(12):
            f = first(k) if k % 4 == 0 else rest(k, f)
            if k == 3:
                X = f
            elif k == 7:
                X = X + f
            elif k == 11:
                X = (X + f) * third
        return X

    # per lane: lane = sample, 16 channels, its own weight
    want = fold(lambda k: wgt[k][:, None] * taps[k], lambda k, f: fma32(np.broadcast_to(wgt[k][:, None], (4, 16)), taps[k], f))

    # quad layout: register 4 r + d of lane i = channel 4 i + d of sample r; the weight of sample r sits in lane r
    def quad(k):
        return np.ascontiguousarray(taps[k].reshape(4, 4, 4).transpose(1, 0, 2).reshape(4, 16))  # [lane i][4 r + d]

    def rest(k, f):
        v = quad(k)
        regs = {("f", c): f[:, c].copy() for c in range(16)}
        regs.update({("v", c): v[:, c] for c in range(16)})
        regs[("w", 0)] = wgt[k]  # lane r holds the weight of sample r
        for st in fmac:
            run(st, regs)
        return np.stack([regs[("f", c)] for c in range(16)], axis=1)

    got_quad = fold(lambda k: np.repeat(wgt[k], 4)[None, :] * quad(k), rest)  # (the first tap: v_mul_f32_dpp, by the compiler)
    got, _ = quad_transpose(transpose, got_quad)
    assert np.array_equal(got, want)
    assert want.dtype == np.float32 and got.dtype == np.float32
