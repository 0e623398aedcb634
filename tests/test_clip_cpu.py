"""CPU (-m "not gpu"): CLIP's image tower and the 2-D metrics without a device — the C ABI (include/p3d_clip.h, _lib.CLIP_SIGNATURES and
the library's exports; argument errors come back before any launch), the host-side plans and PIL's coefficient tables as a stand-alone
host program, the front end's restatement against Pillow bit for bit, the network's restatement against `transformers`' CLIP vision
model in float64, the state-dict names, the gates that tests/test_hip_clip.py holds the kernels to (torch's binary32 run passes them,
seeded faults fail them), and the host logic of panic3d_amd/clip.py and metrics.psnr on torch stand-ins of the operators.  On the
parent commit the module, the table and the symbols do not exist, so every test that takes the `P` fixture fails there; the two
gate-sensitivity tests without it (the GEMM's, LayerNorm's and attention's gates) exercise tests/clip_cases.py alone."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import clip_cases as CC
import host_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = torch.nn.functional


@pytest.fixture(scope="module")
def P():
    import panic3d_amd
    panic3d_amd.build()
    return panic3d_amd


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    exe = host_build.compile_host(tmp_path_factory.mktemp("clip_plan"), "clip_plan_host.cpp")
    return lambda *a: subprocess.run([exe] + [str(v) for v in a], check=True, capture_output=True, text=True).stdout.split("\n")[:-1]


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_clip_header_table_and_exports_agree(P):
    hdr = open(os.path.join(ROOT, "include", "p3d_clip.h")).read()
    declared = set(re.findall(r"\b(p3d_(?:clip|psnr)[a-z0-9_]+)\s*\(", hdr)) - {"p3d_clip_step"}
    lib = P._lib
    assert declared == set(lib.CLIP_SIGNATURES) and len(declared) == 17
    others = set(lib.SIGNATURES) | set(lib.GRAD_SIGNATURES) | set(lib.SYN_GRAD_SIGNATURES) | set(lib.PASTE_GRAD_SIGNATURES) | set(lib.DISC_SIGNATURES) \
        | set(lib.LOSS_SIGNATURES) | set(lib.OPTIM_SIGNATURES) | set(lib.LPIPS_SIGNATURES) | set(lib.ENCODER_SIGNATURES) | set(lib.METRICS_SIGNATURES) \
        | set(lib.RMLINE_SIGNATURES)
    assert not declared & others
    L = lib.lib()
    for name in declared:
        assert hasattr(L, name)
    B = P._build
    assert "p3d_clip.hip" in B.SOURCES and os.path.join("..", "..", "include", "p3d_clip.h") in B.HEADERS and "p3d_clip_plan.hpp" in B.HEADERS
    for unit in (B.RENDER_UNIT, B.SYNTHESIS_UNIT):
        assert not any("p3d_clip" in s for s in unit)
    for name in ("KC", "CUS", "TILE_64", "TILE_32", "MAX_SPLIT", "XCDS", "GELU", "PATCH", "HEAD_DIM", "MAX_T", "MAX_SIDE", "MAX_S", "KIND_PREPARE",
                 "KIND_GEMM", "KIND_LAYERNORM", "KIND_EMBED", "KIND_ATTENTION"):
        assert int(re.search(rf"#define P3D_CLIP_{name} (\d+)", hdr).group(1)) == getattr(lib, f"P3D_CLIP_{name}")
    assert lib.P3D_ABI_VERSION == 9 and L.p3d_abi_version() == 9
    src = open(os.path.join(B.CSRC, "p3d_clip.hip")).read()
    assert "mfma_f32_16x16x4f32" in src and "atomic" not in src.replace("with atomics", "")
    buf = (ctypes.c_size_t * 64)()
    n = L.p3d_clip_struct_layout(buf, 64)
    assert n == 24 and buf[0] == ctypes.sizeof(lib.ClipStep) == 112
    assert list(buf[1:n]) == [getattr(lib.ClipStep, name).offset for name, _ in lib.ClipStep._fields_]
    assert L.p3d_clip_struct_layout(buf, 3) == -2 and L.p3d_clip_struct_layout(None, 64) == -1
    assert P.CLIPVisual is P.clip.CLIPVisual and P.CLIPSimilarity is P.clip.CLIPSimilarity
    assert P.psnr is P.metrics.psnr and P.image_metrics is P.metrics.image_metrics


def test_clip_argument_errors_without_gpu(P):
    L = P._lib.lib()
    p = 256  # never dereferenced: the checks come first

    def gemm(a=p, M=5, K=70, w=p, Nout=9, bias=p, res=None, flags=0, N=0, S=0, patch=0, out=p, plan=0, ws=p, nbytes=1 << 20):
        return L.p3d_clip_gemm_f32(a, M, K, w, Nout, bias, res, flags, N, S, patch, out, plan, ws, nbytes, None)
    assert gemm(a=None) == -1 and gemm(w=None) == -1 and gemm(out=None) == -1 and gemm(M=0) == -1 and gemm(K=0) == -1 and gemm(Nout=0) == -1
    assert gemm(flags=4) == -2 and gemm(plan=3 << 8 | 1) == -2 and gemm(plan=1 << 8) == -2 and gemm(plan=-1) == -2
    assert gemm(N=1) == -2 and gemm(S=64) == -2 and gemm(M=1 << 20, K=1 << 12) == -2
    # the patch mode restates M and K
    patch = dict(flags=2, N=2, S=64, patch=32, M=8, K=3072)
    assert gemm(**dict(patch, M=9)) == -2 and gemm(**dict(patch, K=3071)) == -2 and gemm(**dict(patch, S=65)) == -2 and gemm(**dict(patch, N=0)) == -1
    # a split needs its workspace: K = 70 is two chunks
    need = L.p3d_clip_gemm_workspace_bytes(5, 70, 9, 1 << 8 | 2)
    assert need == 2 * 5 * 9 * 4 and L.p3d_clip_gemm_workspace_bytes(5, 70, 9, 1 << 8 | 1) == 0 and L.p3d_clip_gemm_workspace_bytes(5, 70, 9, 7 << 8) == 0
    assert gemm(plan=1 << 8 | 2, nbytes=need - 1) == -3 and gemm(plan=1 << 8 | 2, ws=None) == -1

    ln = lambda x=p, M=3, D=70, ld=70, g=p, b=p, eps=1e-5, y=p: L.p3d_clip_layernorm_f32(x, M, D, ld, g, b, eps, y, None)
    assert ln(x=None) == -1 and ln(g=None) == -1 and ln(b=None) == -1 and ln(y=None) == -1 and ln(M=0) == -1 and ln(D=0) == -1
    assert ln(ld=69) == -2 and ln(eps=-1.0) == -2 and ln(eps=float("nan")) == -2
    emb = lambda x=p, cls=p, pos=p, N=2, T=5, D=64, g=p, b=p, y=p: L.p3d_clip_embed_f32(x, cls, pos, N, T, D, g, b, 1e-5, y, None)
    assert emb(x=None) == -1 and emb(cls=None) == -1 and emb(pos=None) == -1 and emb(N=0) == -1 and emb(T=0) == -1 and emb(y=None) == -1
    att = lambda x=p, N=2, T=5, heads=2, D=128, y=p: L.p3d_clip_attention_f32(x, N, T, heads, D, y, None)
    assert att(x=None) == -1 and att(y=None) == -1 and att(N=0) == -1 and att(T=0) == -1 and att(heads=0) == -1
    assert att(T=65) == -2 and att(D=127) == -2 and att(D=192) == -2 and att(heads=3) == -2
    cos = lambda a=p, b=p, n=2, D=32, y=p: L.p3d_clip_cosine_f32(a, b, n, D, y, None)
    assert cos(a=None) == -1 and cos(b=None) == -1 and cos(y=None) == -1 and cos(n=0) == -1 and cos(D=0) == -1
    prep = lambda img=p, N=1, C=4, H=40, W=33, S=16, tx=p, ty=p, out=p, ws=p, nb=1 << 20: L.p3d_clip_prepare_f32(img, N, C, H, W, S, tx, ty, out, ws, nb, None)
    assert prep(img=None) == -1 and prep(tx=None) == -1 and prep(ty=None) == -1 and prep(out=None) == -1 and prep(ws=None) == -1 and prep(N=0) == -1
    assert prep(H=0) == -1 and prep(C=2) == -2 and prep(H=16385) == -2 and prep(S=4097) == -2
    need = L.p3d_clip_prepare_workspace_bytes(1, 40, 33, 16)
    assert 0 < need <= 3 * 40 * 16 and prep(nb=need - 1) == -3 and L.p3d_clip_prepare_workspace_bytes(1, 40, 0, 16) == 0
    ps = lambda a=p, b=p, n=1000, out=p, ws=p, nb=1 << 20: L.p3d_psnr_f32(a, b, n, out, ws, nb, None)
    assert ps(a=None) == -1 and ps(b=None) == -1 and ps(out=None) == -1 and ps(ws=None) == -1 and ps(n=0) == -1
    assert L.p3d_psnr_workspace_bytes(1000) == 12 and L.p3d_psnr_workspace_bytes(4097) == 24 and L.p3d_psnr_workspace_bytes(1 << 30) == 12 * 1024
    assert ps(n=4097, nb=23) == -3


def _table(P, recs):
    tab = (P._lib.ClipStep * len(recs))()
    for t, r in zip(tab, recs):
        for k, v in r.items():
            setattr(t, k, v)
    return tab


def test_forward_table_is_checked_before_any_launch(P):
    """The record checks of the walk: bad buffer index, short buffer, workspace too small, and every field that restates a size.  Every
    fault sits in the LAST record: nothing may have been launched for the records before it (pointer 256 would fault the process)."""
    L = P._lib.lib()
    p = 256
    ln = dict(kind=2, M=10, K=64, Nout=64, ld=64, in_=0, out=1, res=-1, eps=1e-5, w_off=0, b_off=64)
    gemm = dict(kind=1, M=10, K=64, Nout=192, in_=1, out=2, res=-1, w_off=128, b_off=128 + 64 * 192)
    attn = dict(kind=4, M=10, K=192, Nout=64, N=2, T=5, heads=1, in_=2, out=1, res=-1)
    proj = dict(kind=1, M=10, K=64, Nout=64, in_=1, out=0, res=0, w_off=0, b_off=-1)
    wf = 128 + 64 * 192 + 192
    off, blen = (ctypes.c_int64 * 3)(0, 640, 1280), (ctypes.c_int64 * 3)(640, 640, 1920)

    def run(recs, weights=p, wf=wf, arena=p, af=3200, off=off, blen=blen, nb=3, ws=p, nbytes=1 << 20):
        return L.p3d_clip_forward_f32(_table(P, recs), len(recs), weights, wf, arena, af, off, blen, nb, ws, nbytes, None)
    ok = [ln, gemm, attn, proj]
    assert run(ok, weights=None) == -1 and run(ok, arena=None) == -1 and run(ok, off=None) == -1 and run(ok, nb=0) == -1
    assert L.p3d_clip_forward_f32(None, 4, p, wf, p, 3200, off, blen, 3, p, 0, None) == -1
    bad = lambda **kw: [ln, gemm, attn, dict(proj, **kw)]
    assert run(bad(kind=9)) == -2 and run(bad(in_=3)) == -2 and run(bad(out=-1)) == -2 and run(bad(in_=0, res=-1)) == -2   # a bad buffer index; in == out
    assert run(bad(res=1)) == -2 and run(bad(res=3)) == -2                                                               # res == in; a bad index
    assert run(bad(M=11)) == -2 and run(bad(Nout=65)) == -2                                                              # a short buffer
    assert run(bad(w_off=wf - 64 * 64 + 1)) == -2 and run(bad(w_off=-1)) == -2 and run(bad(b_off=wf)) == -2 and run(bad(b_off=-2)) == -2
    assert run(bad(flags=4)) == -2 and run(bad(T=5)) == -2 and run(bad(ld=64)) == -2 and run(bad(plan=5 << 8 | 1)) == -2
    assert run(ok, af=3199) == -2 and run(ok, wf=wf - 1) == -2
    assert run([ln, gemm, dict(attn, T=4)]) == -2 and run([ln, gemm, dict(attn, heads=2)]) == -2 and run([ln, gemm, dict(attn, K=191)]) == -2
    assert run([ln, gemm, dict(attn, T=65, N=1)]) == -2 and run([ln, gemm, dict(attn, flags=1)]) == -2
    assert run([gemm, dict(ln, ld=63)]) == -2 and run([gemm, dict(ln, M=11)]) == -2 and run([gemm, dict(ln, ld=65)]) == -2  # 9 * 65 + 64 > 640
    assert run([gemm, dict(ln, M=2, ld=320, Nout=63)]) == -2
    embed = dict(kind=3, M=10, K=64, Nout=64, N=2, T=5, in_=0, out=1, res=-1, eps=1e-5, w_off=0, b_off=64, w2_off=0, b2_off=128)
    assert run([gemm, dict(embed, M=11)]) == -2 and run([gemm, dict(embed, b2_off=wf - 319)]) == -2 and run([gemm, dict(embed, heads=1)]) == -2
    # the workspace: a forced split of the GEMM (K = 64 is one chunk; K = 192 of a second GEMM gives three)
    split = dict(kind=1, M=10, K=192, Nout=64, in_=2, out=0, res=-1, w_off=0, b_off=-1, plan=1 << 8 | 3)
    need = L.p3d_clip_workspace_bytes(_table(P, [ln, gemm, split]), 3)
    assert need == 3 * 10 * 64 * 4 and L.p3d_clip_workspace_bytes(_table(P, ok), 4) == 0
    assert run([ln, gemm, split], nbytes=need - 1) == -3 and run([ln, gemm, split], ws=None) == -1
    assert L.p3d_clip_workspace_bytes(_table(P, [dict(ln, kind=9)]), 1) == 0
    # the front end as a record: its tables must lie inside the blob
    pl = P.ops.clip_resize_plan(20, 16, 8)
    prep = dict(kind=0, M=1, K=3, Nout=3, N=1, S=8, H=20, W=16, in_=2, out=0, res=-1, w_off=0, b_off=8 * (2 + pl["ksx"]))
    assert run([ln, gemm, dict(prep, Nout=4)]) == -2 and run([ln, gemm, dict(prep, N=2)]) == -2 and run([ln, gemm, dict(prep, K=2)]) == -2 and run([ln, gemm, dict(prep, b_off=wf)]) == -2
    assert run([ln, gemm, prep], ws=None) == -1


def test_public_operators_check_before_any_launch(P):
    ops = P.ops
    z = torch.zeros
    for call in (lambda: ops.clip_gemm(z(2, 4), z(4, 3)), lambda: ops.clip_layernorm(z(2, 4), z(4), z(4)), lambda: ops.clip_attention(z(2, 192), 1, 2, 1),
                 lambda: ops.clip_embed(z(4, 8), z(8), z(5, 8), z(8), z(8)), lambda: ops.clip_cosine(z(2, 4), z(2, 4)), lambda: ops.clip_prepare(z(1, 3, 8, 8), 4),
                 lambda: ops.psnr_sums(z(4), z(4)), lambda: P.CLIPVisual(**CC.TINY1)(torch.rand(1, 3, 70, 70)), lambda: P.psnr(torch.rand(4), torch.rand(4))):
        with pytest.raises(RuntimeError, match="CUDA/ROCm"):  # a host pointer never reaches a kernel
            call()
    assert ops.clip_resize_plan(512, 512, 224)["h"] == 224 and ops.clip_resize_plan(301, 187, 224)["h"] == CC.resize_hw(301, 187, 224)[0] == 360
    with pytest.raises(RuntimeError, match="range"):
        ops.clip_resize_plan(20000, 10, 224)
    with pytest.raises(ValueError, match="64 \\* heads"):
        P.CLIPVisual(width=100, heads=2)
    with pytest.raises(ValueError, match="tokens"):
        P.CLIPVisual(width=64, heads=1, layers=1, image_size=224, patch_size=16)


# ---- the plans and the tables, as a host program -------------------------------------------------------------------------------------------
def test_gemm_plan_fills_the_chip(P, host):
    """Every GEMM of the real network at the pair size (N = 2), at a subject's worth (N = 28) and at ragged sizes: the documented fill
    condition — at least 256 workgroups wherever tile-32 tiles x chunks >= 256, else tile 32 with one chunk per split — through the host
    program (which also walks the XCD deal) and through the library alike."""
    kinds = set()
    sizes = [(N * 49, 3072, 768) for N in (2, 28)] + [(N * 50, K, No) for N in (2, 28) for K, No in ((768, 2304), (768, 768), (768, 3072), (3072, 768))]
    sizes += [(2, 768, 512), (28, 768, 512), (1, 4, 1), (5, 64, 64), (50, 100, 70), (67, 192, 130), (100, 768, 96), (4000, 64, 4000), (300, 64, 1000)]
    for M, K, No in sizes:
        tag, tile, split, cps, wgs, grid, ws = host("gemm", M, K, No, 0)[0].split()
        tile, split, cps, wgs, grid, ws = int(tile), int(split), int(cps), int(wgs), int(grid), int(ws)
        pl = P.ops.clip_gemm_plan(M, K, No)
        assert tag == "plan" and (pl["tile"], pl["split"], pl["cps"], pl["workgroups"], pl["workspace_bytes"]) == (tile, split, cps, wgs, ws)
        assert pl["code"] == tile << 8 | split
        chunks, nt = -(-K // 64), -(-No // 64)
        tm = 64 if tile == 1 else 32
        assert wgs == -(-M // tm) * nt * split and grid >= wgs and grid % 8 == 0
        assert ws == (split * M * No * 4 if split > 1 else 0)
        if -(-M // 32) * nt * chunks >= 256:
            assert wgs >= 256, (M, K, No, pl)
        else:
            assert tile == 2 and cps == 1 and split == chunks, (M, K, No, pl)
        kinds.add((tile, split > 1))
    assert kinds == {(1, False), (2, False), (1, True), (2, True)}, kinds  # all four rules
    # force_plan is honoured (want clipped to the chunk count; 255 splits at the most), refused sizes return the error code
    assert host("gemm", 100, 768, 96, 2 << 8 | 2)[0].split()[1:4] == ["2", "2", "6"] and host("gemm", 100, 768, 96, 1 << 8 | 255)[0].split()[1:4] == ["1", "12", "1"]
    assert host("gemm", 5, 64, 64, 1 << 8 | 7)[0].split()[1:4] == ["1", "1", "1"]
    big = host("gemm", 1, 64 * 576, 8, 1 << 8 | 255)[0].split()
    assert big[2:4] == ["192", "3"]
    assert host("gemm", 0, 4, 4, 0) == ["error -1"] and host("gemm", 4, 4, 4, 3 << 8 | 1) == ["error -2"] and host("gemm", 4, 4, 4, 1 << 8) == ["error -2"]
    assert host("gemm", 1 << 20, 1 << 12, 4, 0) == ["error -2"]
    # the attention's query blocks
    for N, T, heads in ((2, 50, 12), (28, 50, 12), (1, 1, 1), (3, 17, 3), (1, 64, 1), (1000, 5, 2)):
        tag, wgs, qb, rows, lds = host("attn", N, T, heads)[0].split()
        pl = P.ops.clip_attention_plan(N, T, heads)
        assert (pl["workgroups"], pl["qblocks"], pl["rows"], pl["lds_bytes"]) == (int(wgs), int(qb), int(rows), int(lds))
        assert int(wgs) == N * heads * int(qb) and int(lds) == 4 * (64 * (64 + 65 + 64) + 4 * 64) <= 64 * 1024
        if N * heads * -(-T // 4) >= 256:
            assert int(wgs) >= 256
    assert 4 * 50 * (64 + 65 + 64) <= 38 * 1024 + 640  # Q, K, V of one head at T = 50: the 38 KB the design counts on
    pair = P.ops.clip_attention_plan(2, 50, 12)
    assert (pair["qblocks"], pair["rows"], pair["workgroups"]) == (13, 4, 312)
    assert host("attn", 1, 65, 1) == ["error -2"] and host("attn", 0, 5, 1) == ["error -1"]


@pytest.mark.parametrize("hw,S", CC.RESIZE_CASES)
def test_resize_tables_and_restatement_equal_pillow(P, host, hw, S):
    """The table builder's integers equal the restatement's (PIL's precompute_coeffs / normalize_coeffs_8bpc, restated in
    clip_cases.pil_table), and the restatement's pixels equal Pillow's resize followed by the crop, exactly."""
    pytest.importorskip("PIL")
    H, W = hw
    h, w = CC.resize_hw(H, W, S)
    oy, ox = CC.crop_offset(h, S), CC.crop_offset(w, S)
    pl = P.ops.clip_resize_plan(H, W, S)
    assert [int(v) for v in host("resize", H, W, S)[0].split()[1:]] == [pl[k] for k in ("h", "w", "offy", "offx", "ksy", "ksx", "row_lo", "row_hi")]
    assert (pl["h"], pl["w"], pl["offy"], pl["offx"]) == (h, w, oy, ox)
    for n_in, n_out, first in ((W, w, ox), (H, h, oy)):
        want = CC.pil_table(n_in, n_out)[first:first + S]
        lines = host("table", n_in, n_out, first, S)
        tab = P.ops.clip_resize_table(n_in, n_out, first, S)
        assert len(lines) == S and tab.shape[0] == S
        for line, row, (xmin, k) in zip(lines, tab, want):
            assert [int(v) for v in line.split()] == [xmin, len(k)] + k
            assert row[:2 + len(k)].tolist() == [xmin, len(k)] + k and not row[2 + len(k):].any()
    lo = min(xmin for xmin, _ in CC.pil_table(H, h)[oy:oy + S])
    hi = max(xmin + len(k) for xmin, k in CC.pil_table(H, h)[oy:oy + S])
    assert (pl["row_lo"], pl["row_hi"]) == (lo, hi)
    for levels in (True, False):
        img = CC.image_case(hw, levels=levels, channels=4)
        assert np.array_equal(CC.preprocess_u8(img, S), CC.pil_preprocess_u8(img, S))
    assert CC.prepare_gate(f"{hw}->{S} (stand-in)", CC.TorchOps.prepare(CC.image_case(hw), S), CC.image_case(hw), S) == []


def test_quantisation_maps_every_level_to_itself_and_the_crop_rounds_half_to_even(P):
    k = torch.arange(256)
    assert torch.equal(torch.floor((k.float() / 255.0).clamp(0, 1) * 255.0).long(), k)
    assert CC.crop_offset(225, 224) == 0 and CC.crop_offset(227, 224) == 2 and CC.crop_offset(228, 224) == 2  # Python's round: half to even
    for long in (224, 225, 226, 227, 228, 229, 301):  # the library's plan rounds the same way, on either axis
        assert P.ops.clip_resize_plan(long, 224, 224)["offy"] == P.ops.clip_resize_plan(224, long, 224)["offx"] == CC.crop_offset(long, 224)


def test_host_program_under_address_and_undefined_sanitizers(tmp_path):
    """The plan header's host code as a plain executable built with -fsanitize=address,undefined (no GPU code, nothing preloaded)."""
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "clip_plan_host_san")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", host_build.CSRC,
                        os.path.join(ROOT, "tests", "clip_plan_host.cpp"), "-o", exe], capture_output=True, text=True)
    if r.returncode:  # only a missing sanitizer runtime is a reason to skip: any other compile error is a failure
        if re.search(r"cannot find -l(asan|ubsan)|lib(asan|ubsan)[^\n]*(not found|No such file)|libclang_rt\.(asan|ubsan)[^\n]*(not found|No such file)|"
                     r"unsupported option '-fsanitize|unrecognized (command[- ]line )?option '-fsanitize", r.stderr):
            pytest.skip("the host compiler has no sanitizer runtime: " + r.stderr[-200:])
        pytest.fail("clip_plan_host.cpp does not compile under -fsanitize=address,undefined:\n" + r.stderr[-2000:])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    for args in (("gemm", 100, 768, 2304, 0), ("gemm", 1, 4, 1, 2 << 8 | 255), ("attn", 2, 50, 12), ("resize", 97, 640, 224), ("table", 640, 1478, 627, 224),
                 ("table", 33, 64, 0, 64), ("resize", 16384, 1, 4096), ("table", 16384, 224, 0, 224)):
        subprocess.run([exe] + [str(a) for a in args], check=True, capture_output=True, env=env)


# ---- the network's restatement against transformers ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny1", "tiny2", "full"])
def test_restatement_agrees_with_transformers_in_float64(P, monkeypatch, name):
    monkeypatch.setenv("HF_HUB_OFFLINE", "1")
    tr = pytest.importorskip("transformers")
    arch = CC.NETWORK_CASES[name][0]
    cfg = tr.CLIPVisionConfig(hidden_size=arch["width"], intermediate_size=4 * arch["width"], num_hidden_layers=arch["layers"],
                              num_attention_heads=arch["heads"], image_size=arch["image_size"], patch_size=arch["patch_size"], projection_dim=arch["output_dim"])
    assert cfg.hidden_act == "quick_gelu" and cfg.layer_norm_eps == 1e-5
    if name == "full":
        d = tr.CLIPVisionConfig()
        assert (d.hidden_size, d.intermediate_size, d.num_hidden_layers, d.num_attention_heads, d.image_size, d.patch_size, d.projection_dim) == \
            (768, 3072, 12, 12, 224, 32, 512)
    torch.manual_seed(5)
    hf = tr.CLIPVisionModelWithProjection(cfg).eval().double()
    if name == "full":
        assert sum(p.numel() for p in hf.parameters()) == 87849216
    with torch.no_grad():
        for p in hf.parameters():  # (transformers initialises biases to 0 and LayerNorms to the identity: every term has to count)
            p.copy_(torch.randn(p.shape, dtype=torch.float64) * (0.5 if p.ndim == 1 else p.shape[-1] ** -0.5))
    sd = P.CLIPVisual.convert_hf_state_dict(hf.state_dict())
    assert set(sd) == set(P.CLIPVisual(**arch).state_dict())
    x = torch.randn(2, 3, arch["image_size"], arch["image_size"], dtype=torch.float64)
    with torch.no_grad():
        want = hf(pixel_values=x).image_embeds
        got = CC.network(sd, x, arch["heads"], torch.float64)
    e = CC.rel_l2(got, want)
    print(f"clip restatement vs transformers ({name}): rel-L2 {e:.3e}")
    assert tuple(got.shape) == tuple(want.shape) == (2, arch["output_dim"]) and e <= 1e-12


# ---- the state dict ---------------------------------------------------------------------------------------------------------------------
def test_state_dict_names_counts_and_loading(P):
    full = P.CLIPVisual()
    sd = full.state_dict()
    assert len(sd) == 152 and sum(p.numel() for p in full.parameters()) == 87849216
    assert set(sd) == set(CC.make_weights(**CC.FULL))
    for name, shape in (("conv1.weight", (768, 3, 32, 32)), ("class_embedding", (768,)), ("positional_embedding", (50, 768)), ("proj", (768, 512)),
                        ("transformer.resblocks.11.attn.in_proj_weight", (2304, 768)), ("transformer.resblocks.0.attn.in_proj_bias", (2304,)),
                        ("transformer.resblocks.3.attn.out_proj.weight", (768, 768)), ("transformer.resblocks.3.mlp.c_fc.weight", (3072, 768)),
                        ("transformer.resblocks.3.mlp.c_proj.weight", (768, 3072)), ("ln_post.bias", (768,)), ("ln_pre.weight", (768,))):
        assert tuple(sd[name].shape) == shape
    assert all(not p.requires_grad for p in full.parameters())
    del full, sd
    want = CC.make_weights(**CC.TINY1, seed=4)
    a = P.CLIPVisual(**CC.TINY1)
    a.load_state_dict(want)
    assert all(torch.equal(v, want[k]) for k, v in a.state_dict().items())
    b = P.CLIPVisual(**CC.TINY1)
    b.load_state_dict(a.state_dict())  # round trip
    assert all(torch.equal(v, want[k]) for k, v in b.state_dict().items())
    c = P.CLIPVisual(**CC.TINY1)       # a whole CLIP model's dict: visual.* in float16, the text tower ignored
    c.load_state_dict({**{f"visual.{k}": v.half() for k, v in want.items()}, "token_embedding.weight": torch.zeros(3, 3), "logit_scale": torch.zeros(())})
    assert all(v.dtype == torch.float32 and torch.equal(v, want[k].half().float()) for k, v in c.state_dict().items())
    with pytest.raises(RuntimeError, match="Missing key"):
        P.CLIPVisual(**CC.TINY1).load_state_dict({k: v for k, v in want.items() if k != "proj"})


# ---- the gates: torch's binary32 run passes, seeded faults fail ---------------------------------------------------------------------------------
def test_gemm_gate_accepts_binary32_and_rejects_faults():
    for shape in CC.GEMM_SHAPES:
        c = CC.gemm_case(shape)
        for bias, gelu, res in CC.EPILOGUES:
            y, s, K = CC.gemm_ref(c, bias, gelu, res)
            got = CC.TorchOps.gemm(c["a"], c["w"], c["bias"] if bias else None, c["res"] if res else None, gelu, 0, 0)
            assert CC.gate(f"gemm {shape} {bias, gelu, res}", got, y, s, K, verbose=False) == []
            faults = (["bias_per_split"] if bias else []) + (["gelu"] if gelu else []) + (["no_res"] if res else [])
            for fault in faults:
                if shape == (1, 4, 1) and fault == "gelu":
                    continue  # (a single value: the two activations can agree there)
                bad = CC.gemm_ref(c, bias, gelu, res, torch.float32, fault=fault)[0]
                assert CC.gate("", bad, y, s, K, verbose=False) != [], (shape, fault)
    for case in CC.PATCH_CASES:
        c = CC.patch_case(*case)
        assert CC.gate(f"patch {case}", CC.TorchOps.gemm(c["x"], c["wk"], None, None, False, c["patch"], 0), c["y"], c["y_abs"], c["K"], verbose=False) == []
        wrong = c["w"].permute(0, 2, 3, 1).reshape(c["w"].shape[0], -1).t().contiguous()  # the patch flattened in (y, x, c) order
        assert CC.gate("", CC.TorchOps.gemm(c["x"], wrong, None, None, False, c["patch"], 0), c["y"], c["y_abs"], c["K"], verbose=False) != []


def test_layernorm_and_attention_gates_accept_binary32_and_reject_faults():
    for D in CC.LN_D:
        c = CC.ln_case(5, D, "offset")
        assert CC.ln_gate(f"offset D={D}", F.layer_norm(c["x"], (D,), c["gamma"], c["beta"], CC.EPS), c, verbose=False) == []
        assert CC.ln_gate("", CC.layernorm(c["x"], c["gamma"], c["beta"], fault="one_pass"), c, verbose=False) != [], D  # the one-pass variance
        k = CC.ln_case(3, D, "constant")
        assert torch.equal(F.layer_norm(k["x"], (D,), k["gamma"], k["beta"], CC.EPS), k["beta"].expand(3, D))
    # the embedding form through the same gate: the positional embedding added after ln_pre fails
    g = torch.Generator().manual_seed(1)
    N, T, D = 2, 5, 64
    patches, cls, pos = torch.randn(N * (T - 1), D, generator=g), torch.randn(D, generator=g), torch.randn(T, D, generator=g)
    c = CC.ln_case(N * T, D)
    x = (torch.cat([cls.expand(N, 1, D), patches.reshape(N, T - 1, D)], 1) + pos).reshape(N * T, D)
    assert CC.ln_gate("embed", F.layer_norm(x, (D,), c["gamma"], c["beta"], CC.EPS), c, x=x, verbose=False) == []
    assert CC.ln_gate("", CC.embed(patches, cls, pos, N, c["gamma"], c["beta"], fault="pos_after_ln"), c, x=x, verbose=False) != []
    for kind, faults in (("plain", ("no_scale", "kv_swap")), ("pm120", ("no_max",)), ("pm80", ("kv_swap",)), ("dominant", ("kv_swap",))):
        c = CC.attn_case(3, 17, 3, kind)
        assert CC.attn_gate(kind, CC.attention(c["qkv"], 3, 17, 3), c, verbose=False) == []
        for fault in faults:
            assert CC.attn_gate("", CC.attention(c["qkv"], 3, 17, 3, fault=fault), c, verbose=False) != [], (kind, fault)


def test_front_end_gate_rejects_a_missing_rounding_constant_and_a_shifted_crop(P):
    """The gate on the integer sums the kernels form, taken from the LIBRARY's tables (p3d_clip_resize_plan / _table): they pass; without
    the rounding constant, or with the tables of a crop one pixel off, they fail."""
    pytest.importorskip("PIL")
    for hw, S in (((301, 187), 224), ((33, 40), 64), ((230, 225), 224)):
        img = CC.image_case(hw)
        pl = P.ops.clip_resize_plan(hw[0], hw[1], S)
        tabs = lambda dy=0, dx=0: (P.ops.clip_resize_table(hw[1], pl["w"], pl["offx"] + dx, S), P.ops.clip_resize_table(hw[0], pl["h"], pl["offy"] + dy, S))
        assert CC.prepare_gate("", CC.preprocess_from_tables(img, *tabs()), img, S, verbose=False) == []
        assert CC.prepare_gate("", CC.preprocess_from_tables(img, *tabs(), fault="no_round"), img, S, verbose=False) != []
        shifted = tabs(dy=1) if pl["h"] > S else tabs(dx=1)
        assert CC.prepare_gate("", CC.preprocess_from_tables(img, *shifted), img, S, verbose=False) != []
        assert CC.prepare_gate("", CC.preprocess(img, S), img, S, verbose=False) == []
        assert CC.prepare_gate("", CC.preprocess(img, S, fault="no_round"), img, S, verbose=False) != []
        assert CC.prepare_gate("", CC.preprocess(img, S, fault="crop"), img, S, verbose=False) != []
        off = CC.preprocess(img, S) * (1 + 4 * CC.EPS32)  # a normalisation two ulps off
        assert CC.prepare_gate("", off, img, S, verbose=False) != []


@pytest.mark.parametrize("fault", ["gelu", "kv_swap", "no_scale", "pos_after_ln", "no_round", "crop"])
def test_network_gate_rejects_faults(P, monkeypatch, fault):
    """The whole-network gate on the stand-ins: torch's binary32 run passes (network_case's f32 IS that run), every seeded fault fails."""
    c = CC.network_case("tiny1")
    assert CC.network_gate("tiny1 f32", c["f32"], c, verbose=False) == []
    CC.install_ops(monkeypatch, P.ops, fault=fault)
    model = P.CLIPVisual(**c["arch"])
    model.load_state_dict(c["sd"])
    bad = model(c["img"], fused=False)
    assert CC.network_gate(f"[{fault}] tiny1", bad, c, verbose=False) != []


# ---- the module's host logic on the stand-ins -------------------------------------------------------------------------------------------
def test_network_host_logic_on_stand_ins(P, monkeypatch):
    CC.install_ops(monkeypatch, P.ops)
    for name in ("tiny1", "tiny2"):
        c = CC.network_case(name)
        model = P.CLIPVisual(**c["arch"])
        model.load_state_dict(c["sd"])
        fused = model(c["img"])
        assert tuple(fused.shape) == (c["N"], c["arch"]["output_dim"]) and CC.network_gate(f"{name} (stand-ins)", fused, c) == []
        layered = model(c["img"], fused=False)
        assert torch.equal(fused, layered)  # the table walk and the step-by-step calls: the same operands in the same order
        assert torch.equal(model.encode_image(c["x"]), fused) and torch.equal(model.encode_image(c["x"], fused=False), fused)
        recs, buf_len, (buf, shape) = model.records(c["N"], tuple(c["img"].shape[1:]))
        L = c["arch"]["layers"]
        assert len(recs) == 3 + 7 * L + 2 and [r["kind"] for r in recs[:3]] == ["prepare", "gemm", "embed"] and shape == (c["N"], c["arch"]["output_dim"])
        assert model.program(c["N"], tuple(c["img"].shape[1:]))[0].launches >= len(recs) + 1
    # the default network's walk of a preprocessed batch: 88 steps (conv1, embed, 12 x 7, ln_post, proj); 50 of its 50 GEMMs are split at
    # the pair size (138 launches), only proj at a subject's worth (89)
    recs = P.CLIPVisual.records(_Shape(), 2)[0]
    assert len(recs) == 2 + 7 * 12 + 2 == 88
    for N, want in ((2, 138), (28, 89)):
        gemms = [r for r in P.CLIPVisual.records(_Shape(), N)[0] if r["kind"] == "gemm"]
        assert len(gemms) == 50 and 88 + sum(P.ops.clip_gemm_plan(r["M"], r["K"], r["Nout"])["split"] > 1 for r in gemms) == want


class _Shape:
    """CLIPVisual.records needs the sizes and the operands' offsets only: the default configuration without its 351 MB."""
    width, layers, heads, image_size, patch_size, output_dim, tokens = 768, 12, 12, 224, 32, 512, 50

    def operands(self):
        class Any(dict):
            def __missing__(self, k):
                return (0, ())
        return None, Any()


def test_errors_the_operand_cache_and_the_similarity(P, monkeypatch):
    CC.install_ops(monkeypatch, P.ops)
    c = CC.network_case("tiny1")
    model = P.CLIPVisual(**c["arch"])
    model.load_state_dict(c["sd"])
    with pytest.raises(NotImplementedError, match="inference only"):
        model(c["img"].clone().requires_grad_(True))
    with torch.no_grad():
        model(c["img"].clone().requires_grad_(True))  # nothing is recorded: allowed
    with pytest.raises(ValueError, match="image batch"):
        model(c["img"][:, :2])
    with pytest.raises(RuntimeError, match="float32"):
        model(c["img"].double())
    with pytest.raises(ValueError, match="preprocessed"):
        model.encode_image(c["img"])
    # the cached operands and programs: reused while nothing changes, re-derived after an in-place write or a reload
    o1, p1 = model.operands(), model.program(3, (4, 80, 70))
    assert model.operands() is o1 and model.program(3, (4, 80, 70)) is p1
    before = model(c["img"])
    with torch.no_grad():
        model.transformer.resblocks[1].mlp.c_fc.weight.mul_(1.5)
    assert model.operands() is not o1 and model.program(3, (4, 80, 70)) is not p1
    assert not torch.equal(model(c["img"]), before)
    o2 = model.operands()
    model.load_state_dict(c["sd"])  # copy_ bumps every version
    assert model.operands() is not o2 and torch.equal(model(c["img"]), before)
    w = c["sd"]["transformer.resblocks.0.attn.in_proj_weight"]
    assert torch.equal(model.operand("0.in_proj.w"), w.t()) and torch.equal(model.operand("conv1"), c["sd"]["conv1.weight"].reshape(128, -1).t())
    # the similarity
    sim = P.CLIPSimilarity(model)
    a, b = c["img"], c["img"].roll(5, -1)
    s = sim(a, b)
    ea, eb = c["f64"], CC.network(c["sd"], CC.preprocess(b, 64), 2, torch.float64)
    assert tuple(s.shape) == (3,) and float((s.double() - CC.cosine(ea, eb)).abs().max()) < 1e-5
    assert float((sim(a[0], b[0]) - s[:1]).abs().max()) < 1e-6 and float((sim(b, a) - s).abs().max()) < 1e-6
    with pytest.raises(NotImplementedError, match="inference only"):
        sim(a.clone().requires_grad_(True), b)
    with pytest.raises(ValueError, match="as many"):
        sim(a, b[:2])


def test_similarity_from_a_saved_state_dict(P, monkeypatch, tmp_path):
    """CLIPSimilarity(path): the architecture is read off the tensors' shapes, with and without the `visual.` prefix of a whole CLIP model."""
    CC.install_ops(monkeypatch, P.ops)
    c = CC.network_case("tiny2")
    for pre in ("", "visual."):
        path = str(tmp_path / f"clip{len(pre)}.pt")
        torch.save({**{pre + k: v.half() if pre else v for k, v in c["sd"].items()}, **({"logit_scale": torch.zeros(())} if pre else {})}, path)
        m = P.CLIPSimilarity(path).model
        assert {k: getattr(m, k) for k in CC.TINY2} == CC.TINY2 and not m.training
        want = c["sd"]["proj"].half().float() if pre else c["sd"]["proj"]
        assert torch.equal(m.proj, want)


class _Lpips(torch.nn.Module):
    def forward(self, preds, target):
        return (preds - target).abs().mean(dim=(1, 2, 3))


def test_psnr_and_image_metrics_against_float64(P, monkeypatch):
    CC.install_ops(monkeypatch, P.ops)
    for shape in CC.PSNR_SHAPES:
        c = CC.psnr_case(shape)
        for rng in (None, 1.0, 2.0):
            got, want = P.psnr(c["pred"], c["target"], rng), CC.psnr64(c["pred"], c["target"], rng)
            assert abs(got - want) <= 1e-5 * abs(want), (shape, rng, got, want)
    c = CC.psnr_case((1, 3, 7, 5))
    assert P.psnr(c["target"], c["target"]) == float("inf")
    const = torch.full((1, 3, 7, 5), 0.5)
    assert P.psnr(c["pred"], const) == float("-inf") and np.isnan(P.psnr(const, const)) and abs(P.psnr(c["pred"], const, 1.0) - CC.psnr64(c["pred"], const, 1.0)) < 1e-4
    with pytest.raises(ValueError, match="one shape"):
        P.psnr(c["pred"], c["target"][:, :2])
    with pytest.raises(ValueError, match="positive"):
        P.psnr(c["pred"], c["target"], 0.0)
    with pytest.raises(NotImplementedError, match="inference only"):
        P.psnr(c["pred"].clone().requires_grad_(True), c["target"])
    n = CC.network_case("tiny1")
    model = P.CLIPVisual(**n["arch"])
    model.load_state_dict(n["sd"])
    pred, gt = n["img"][:, :3].contiguous(), n["img"][:, :3].roll(3, -1).contiguous()
    m = P.image_metrics(pred, gt, _Lpips(), P.CLIPSimilarity(model))
    assert set(m) == {"lpips", "psnr", "clip"} and all(isinstance(v, float) for v in m.values())
    assert abs(m["psnr"] - CC.psnr64(pred, gt)) <= 1e-5 * abs(m["psnr"]) and abs(m["lpips"] - float((pred - gt).abs().mean())) < 1e-6
    eb = CC.network(n["sd"], CC.preprocess(gt, 64), 2, torch.float64)
    ea = CC.network(n["sd"], CC.preprocess(pred, 64), 2, torch.float64)
    assert abs(m["clip"] - float(CC.cosine(ea, eb).mean())) < 1e-5 and m["clip"] < 1.0
