"""CPU (-m "not gpu"): the backward passes' C ABI — include/p3d_render_grad.h, _lib.GRAD_SIGNATURES and the library's exports agree,
and argument errors are reported before any launch (no GPU needed)."""
import ctypes as C
import os
import re

import pytest

import p3d_testing as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def P():
    import panic3d_amd
    panic3d_amd.build()
    return panic3d_amd


def test_grad_header_table_and_exports_agree(P):
    hdr = open(os.path.join(ROOT, "include", "p3d_render_grad.h")).read()
    declared = set(re.findall(r"\b(p3d_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(P._lib.GRAD_SIGNATURES), "include/p3d_render_grad.h and _lib.GRAD_SIGNATURES disagree"
    assert not declared & set(P._lib.SIGNATURES), "the backward table must stay separate from panic3d_hip.h's"
    L = P._lib.lib()
    for name in declared:
        assert hasattr(L, name)
    assert "p3d_render_grad.hip" in P._build.SOURCES
    assert os.path.join("..", "..", "include", "p3d_render_grad.h") in P._build.HEADERS


def test_grad_workspace_sizes(P):
    L = P._lib.lib()
    assert L.p3d_render_backward_workspace_bytes(0, 16, 48, 48) == 0
    assert L.p3d_render_backward_workspace_bytes(1, 16, 1, 0) == 0
    small = L.p3d_render_backward_workspace_bytes(1, 1024, 48, 48)
    assert small >= 1024 * 96 * 17 and small % 256 == 0
    assert L.p3d_render_backward_workspace_bytes(4, 1024, 48, 48) > small
    assert L.p3d_triplane_decode_backward_workspace_bytes(1, 0) == 0
    assert L.p3d_triplane_decode_backward_workspace_bytes(1, 64) >= 256 + 4 * 4257


def test_grad_argument_errors_without_gpu(P):
    L = P._lib.lib()
    o = P.ops.make_opts(T.RENDERING_KWARGS)
    fake = C.c_void_p(256)  # never dereferenced: the checks come first
    wsb = L.p3d_render_backward_workspace_bytes(1, 16, 48, 48)
    args = [fake, 1, 8, 8, fake, fake, 16, fake, fake, fake, fake, fake, C.byref(o), None, None, None, None, fake, fake, fake, fake, fake,
            fake, wsb, None]

    def call(**kw):
        a = list(args)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return L.p3d_render_backward_f32(*a)
    assert call(a0=None) == -1          # planes
    assert call(a7=None) == -1          # merged depths
    assert call(a18=None) == -1         # d_w0
    assert call(a22=None) == -1         # workspace
    assert call(a1=0) == -1             # N
    assert call(a6=0) == -1             # R
    assert call(a2=5000) == -2          # H: per-image offsets are 32-bit
    assert call(a23=wsb - 1) == -3      # workspace too small
    assert call(a22=C.c_void_p(264)) == -1  # workspace not 256-byte aligned
    o2 = P.ops.make_opts(dict(T.RENDERING_KWARGS, depth_resolution_importance=200))
    args[12] = C.byref(o2)
    assert call() == -2                 # Sf beyond P3D_MAX_S
    wsp = L.p3d_triplane_decode_backward_workspace_bytes(1, 16)
    dec = [fake, 1, 8, 8, fake, 16, fake, fake, fake, fake, C.byref(o), None, None, fake, fake, fake, fake, fake, fake, wsp, None]
    bad = list(dec)
    bad[4] = None
    assert L.p3d_triplane_decode_backward_f32(*bad) == -1
    bad = list(dec)
    bad[19] = wsp - 1
    assert L.p3d_triplane_decode_backward_f32(*bad) == -3
