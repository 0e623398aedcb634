"""CPU: the host-side plan of a modulated convolution (csrc/p3d_conv_plan.hpp).  (1) The shape queries of the library answer
what they answered before the plan existed (values recorded from that build in tests/golden/conv_queries.json).  (2) A host
program compiled from the plan header alone, with no device code, checks over the same sweep that every plan under every operand
mode, input / output kind and forcing switch fits the workspace the library asks for, and prints the default plan of the
generator's layers: that is the documented dispatch below."""
import ctypes as C
import json
import os
import subprocess

import pytest

import conv_plan_cases as K
from host_build import compile_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X2 = 2  # P3D_CONV_MMA_F16X2


@pytest.fixture(scope="module")
def L():
    import panic3d_amd
    panic3d_amd.build()
    lib = panic3d_amd._lib.lib()
    lib.p3d_modconv2d_workspace_bytes.restype = C.c_size_t
    return lib


def test_shape_queries_answer_the_recorded_values(L):
    with open(os.path.join(ROOT, "tests", "golden", "conv_queries.json")) as f:
        rows = json.load(f)
    assert [tuple(r[:6]) for r in rows] == K.all_cases()
    for r in rows:
        N, I, O, H, W, up = r[:6]
        got = [L.p3d_modconv2d_workspace_bytes(N, I, O, H, W, up), L.p3d_conv_weight_layout(I, O, W, up), L.p3d_conv_takes_image(I, O, W, up)]
        got += [L.p3d_conv_fuses_torgb(N, I, O, H, W, rgb) for rgb in (0, 1, 3, 4, 5)]
        assert got == r[6:], (N, I, O, H, W, up)


# The generator's calls (stylegan2.SynthesisBlock, default switches): a block's up-sampling conv0 reads the image conv1 of the block
# before it wrote and writes an image where its own conv1 takes one (maps >= 32^2), fp32 below; conv1 reads an image from 32^2 up and
# writes y plus the next conv0's image; the super-resolution's conv1 layers take their ToRGB layer along.  Each call: two-term
# operands, lrelu.  The table was checked once against a kernel trace of an eager backbone + super-resolution pass on the GPU.
# What each of these plans COMPUTES is pinned elsewhere: tests/modconv_cases.py reaches every kernel, reduction and tail the plan can name
# (tests/test_modconv_cases_cpu.py checks that against this header) and tests/test_hip_modconv_edges.py runs every case on the GPU
# against the float64 reference and gate of tests/modconv_ref.py.
def _calls():
    out = []
    for name, I, O, r, up in K.BACKBONE + K.SUPERRES:
        sr = name.startswith("sr.")
        if up == 2:
            x_img, y_img, rgb = not name.startswith("sr.b0"), 2 * r >= 32, False
        else:
            x_img, y_img, rgb = r >= 32, not name.endswith("b1.conv1") and name != "b256.conv1", sr
        out.append((name, I, O, r, up, x_img, y_img, rgb))
    return out


DISPATCH = {  # (name, N): main kernel, split-K depth, reduction, last pass, k_act_to_image of the fp32 input first
    ('b4.conv1', 1): ('k_modconv_h<0,true>', 32, 'k_splitk_reduce_img', '-', False),
    ('b8.conv0', 1): ('k_modconv_up3<false>', 16, 'k_splitk_reduce', 'k_fir4x4_tiled', False),
    ('b8.conv1', 1): ('k_modconv_h<0,true>', 32, 'k_splitk_reduce_img', '-', False),
    ('b16.conv0', 1): ('k_modconv_up3<false>', 8, '-', 'k_fir4x4_tiled', False),
    ('b16.conv1', 1): ('k_modconv_h<0,true>', 16, 'k_splitk_reduce_img', '-', False),
    ('b32.conv0', 1): ('k_modconv_up3<false>', 8, '-', 'k_fir4x4_img2<8>', False),
    ('b32.conv1', 1): ('k_modconv_w3<false>', 8, 'k_splitk_reduce_img', '-', False),
    ('b64.conv0', 1): ('k_modconv_up5', 2, '-', 'k_fir4x4_img<true,2,3>', False),
    ('b64.conv1', 1): ('k_modconv_w3<false>', 2, 'k_splitk_reduce_img', '-', False),
    ('b128.conv0', 1): ('k_modconv_up5', 2, '-', 'k_fir4x4_img<true,2,3>', False),
    ('b128.conv1', 1): ('k_modconv_w3<false>', 1, '-', '-', False),
    ('b256.conv0', 1): ('k_modconv_up4<4,2,2>', 1, '-', '-', False),
    ('b256.conv1', 1): ('k_modconv_w3<false>', 1, '-', '-', False),
    ('sr.b0.conv0', 1): ('k_modconv_up3<true>', 1, '-', '-', True),
    ('sr.b0.conv1', 1): ('k_modconv_w3<true>', 1, '-', '-', False),
    ('sr.b1.conv0', 1): ('k_modconv_up4<8,2,3>', 1, '-', '-', False),
    ('sr.b1.conv1', 1): ('k_modconv_w3<true>', 1, '-', '-', False),
    ('b4.conv1', 4): ('k_modconv_h<0,true>', 8, 'k_splitk_reduce_img', '-', False),
    ('b8.conv0', 4): ('k_modconv_up5', 4, '-', 'k_fir4x4_tiled', False),
    ('b8.conv1', 4): ('k_modconv_h<0,true>', 8, 'k_splitk_reduce_img', '-', False),
    ('b16.conv0', 4): ('k_modconv_up5', 2, '-', 'k_fir4x4_tiled', False),
    ('b16.conv1', 4): ('k_modconv_h<0,true>', 4, 'k_splitk_reduce_img', '-', False),
    ('b32.conv0', 4): ('k_modconv_up5', 2, '-', 'k_fir4x4_img<true,2,3>', False),
    ('b32.conv1', 4): ('k_modconv_w3<false>', 2, 'k_splitk_reduce_img', '-', False),
    ('b64.conv0', 4): ('k_modconv_up4<4,2,2>', 1, '-', '-', False),
    ('b64.conv1', 4): ('k_modconv_w3<false>', 1, '-', '-', False),
    ('b128.conv0', 4): ('k_modconv_up4<4,2,2>', 1, '-', '-', False),
    ('b128.conv1', 4): ('k_modconv_w3<false>', 1, '-', '-', False),
    ('b256.conv0', 4): ('k_modconv_up4<8,2,3>', 1, '-', '-', False),
    ('b256.conv1', 4): ('k_modconv_w3<false>', 1, '-', '-', False),
    ('sr.b0.conv0', 4): ('k_modconv_up3<true>', 1, '-', '-', True),
    ('sr.b0.conv1', 4): ('k_modconv_w3<true>', 1, '-', '-', False),
    ('sr.b1.conv0', 4): ('k_modconv_up4<8,2,3>', 1, '-', '-', False),
    ('sr.b1.conv1', 4): ('k_modconv_w3<true>', 1, '-', '-', False),
}


def test_plans_fit_the_workspace_and_follow_the_dispatch_table(tmp_path):
    exe = compile_host(tmp_path, "conv_plan_host.cpp")
    lines = ["s %d %d %d %d %d %d" % c for c in K.all_cases()]
    calls = [(name, n, I, O, r, up, x_img, y_img, rgb) for n in (1, 4) for name, I, O, r, up, x_img, y_img, rgb in _calls()]
    for name, n, I, O, r, up, x_img, y_img, rgb in calls:
        lines.append("p %d %d %d %d %d 3 %d %d %d %d %d 1 0.2" % (n, I, O, r, r, up, X2, x_img, y_img, rgb))
    res = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-4000:]
    out = res.stdout.splitlines()
    sweeps = [int(s.split()[1]) for s in out if s.startswith("s ")]
    assert len(sweeps) == len(K.all_cases()) and sum(sweeps) > 100000
    plans = [s.split(" ", 1)[1] for s in out if s.startswith("p ")]
    got = {}
    for (name, n, *_), p in zip(calls, plans):
        main, ks, red, tail = p.split()[:4]
        got[(name, n)] = (main, int(ks), red, tail, p.endswith("(input image first)"))
    assert got == DISPATCH
