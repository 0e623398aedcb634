"""CPU (-m "not gpu"): the geometry metrics without a device — the C ABI of the point-to-mesh distance (include/p3d_metrics.h,
_lib.METRICS_SIGNATURES and the library's exports; argument errors come back before any launch), its launch plan as a host program,
the host wiring of panic3d_amd/metrics.py on a stand-in of the operator against plain-Python oracles written from the stated semantics
of `_scripts/eval/measure.py:54-99, :197-201`, the area sampler, and the restatements and gates that tests/test_hip_metrics.py holds the
kernel to: float32 against float64 on every case, and float64 against seeded faults.  On the parent commit the module, the operator
and the symbols do not exist."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import metrics_cases as MC
from host_build import compile_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def P():
    import panic3d_amd
    panic3d_amd.build()
    return panic3d_amd


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_metrics_header_table_and_exports_agree(P):
    hdr = open(os.path.join(ROOT, "include", "p3d_metrics.h")).read()
    declared = set(re.findall(r"\b(p3d_[a-z0-9_]+)\s*\(", hdr))
    lib = P._lib
    assert declared == set(lib.METRICS_SIGNATURES) and len(declared) == 3
    others = set(lib.SIGNATURES) | set(lib.GRAD_SIGNATURES) | set(lib.SYN_GRAD_SIGNATURES) | set(lib.PASTE_GRAD_SIGNATURES) | set(lib.DISC_SIGNATURES) \
        | set(lib.LOSS_SIGNATURES) | set(lib.OPTIM_SIGNATURES) | set(lib.LPIPS_SIGNATURES) | set(lib.ENCODER_SIGNATURES)
    assert not declared & others
    L = lib.lib()
    for name in declared:
        assert hasattr(L, name)
    assert "p3d_metrics.hip" in P._build.SOURCES and "p3d_metrics_plan.hpp" in P._build.HEADERS
    assert os.path.join("..", "..", "include", "p3d_metrics.h") in P._build.HEADERS
    assert not {"p3d_metrics.hip", "p3d_metrics_plan.hpp"} & (set(P._build.SYNTHESIS_UNIT) | set(P._build.RENDER_UNIT))
    for name in ("NO_CULL", "SLICES_SHIFT", "MAX_SLICES", "QUERY_BLOCK", "FACE_TILE"):
        assert int(re.search(rf"#define P3D_PM_{name} (\d+)", hdr).group(1)) == getattr(lib, f"P3D_PM_{name}")
    assert lib.P3D_ABI_VERSION == 9 and L.p3d_abi_version() == 9
    assert P.point_mesh_squared_distance is P.metrics.point_mesh_squared_distance and P.geometry_metrics is P.metrics.geometry_metrics


def test_metrics_argument_errors_without_gpu(P):
    L = P._lib.lib()
    p = 256  # never dereferenced: the checks come first
    big = 1 << 40

    def call(Q=10, V=5, F=4, flags=1, margin=0.0, wb=big, **ptr):
        a = dict(dict.fromkeys(("points", "verts", "faces", "d2", "face", "closest", "ws"), p), **ptr)
        return L.p3d_point_mesh_dist2_f32(a["points"], Q, a["verts"], V, a["faces"], F, flags, margin, a["d2"], a["face"], a["closest"], a["ws"], wb, None)
    for k in ("points", "verts", "faces", "d2", "ws"):
        assert call(**{k: None}) == -1, k
    assert call(ws=264) == -1, "a workspace that is not 16-byte aligned"
    assert call(F=0) == -2 and call(F=-1) == -2 and call(V=0) == -2 and call(V=1 << 31) == -2
    assert call(F=(1 << 26) + 1) == -2 and call(Q=(1 << 26) + 1) == -2 and call(Q=-1) == -1
    assert call(flags=2) == -1 and call(flags=1 << 20) == -1, "an unknown flag bit"
    assert call(flags=257 << 8) == -2, "more slices than P3D_PM_MAX_SLICES"
    assert call(margin=-1.0) == -1 and call(margin=float("nan")) == -1 and call(margin=float("inf")) == -1
    need = L.p3d_point_mesh_workspace_bytes(10, 4)
    assert need == 4 * 64 + 1 * 32 + 1 * 64 + 10 * 4 + 256 * 10 * 8, "records, boxes, sample records, seeds and partial (dist2, face)"
    assert call(wb=need - 1) == -3 and call(wb=0) == -3
    assert call(Q=0) == 0 and call(Q=0, face=None, closest=None) == 0, "Q = 0 is a no-op"
    assert call(Q=0, F=0) == -2 and call(Q=0, d2=None) == -1, "... after the checks"
    assert L.p3d_point_mesh_workspace_bytes(10, 0) == 0 and L.p3d_point_mesh_workspace_bytes(-1, 4) == 0
    assert L.p3d_point_mesh_workspace_bytes(0, 1) == 64 + 32 + 64
    out = (P._lib.C.c_int64 * 6)()
    assert L.p3d_point_mesh_plan(10, 4, 0, None, 6) == -1 and L.p3d_point_mesh_plan(10, 4, 0, out, 5) == -1
    assert L.p3d_point_mesh_plan(10000, 2000000, 0, out, 6) == 0 and list(out) == [79, 31250, 255, 123, 128, 64]


# ---- the plan's host program -------------------------------------------------------------------------------------------------------------
QB, FT = 128, 64
PLAN_SIZES = sorted({(q, f) for q in (1, 63, 64, 65, QB - 1, QB, QB + 1, 10000) for f in (1, FT - 1, FT, FT + 1, 2 * FT + 1, 256 * FT, 256 * FT + 1, 2000000)})


def test_plan_host_program(tmp_path):
    exe = compile_host(tmp_path, "metrics_plan_host.cpp")

    def run(q, f, flags):
        r = subprocess.run([exe, str(q), str(f), str(flags)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, (q, f, flags, r.stderr)  # the program itself walks the slices and the blocks: exactly-once coverage
        return r.stdout.split()
    for q, f in PLAN_SIZES:
        for forced in (0, 1, 2, 3, 64, 256):
            out = run(q, f, forced << 8)
            assert out[0] == "plan", (q, f, forced, out)
            qblocks, ntiles, slices, tps = (int(x) for x in out[1:5])
            assert qblocks == -(-q // QB) and ntiles == -(-f // FT)
            # every face in exactly one slice, every query in exactly one block (restated here from the printed numbers)
            owner = np.arange(ntiles) // tps
            assert owner.max() == slices - 1 and len(np.unique(owner)) == slices
            assert (np.arange(q) // QB).max() == qblocks - 1
            assert slices <= (forced or 256) and slices <= ntiles
            if forced and forced <= ntiles and ntiles % forced == 0:
                assert slices == forced
    assert run(10000, 2000000, 0)[1:5] == ["79", "31250", "255", "123"]
    assert run(0, 5, 0)[:2] == ["plan", "0"]
    assert run(5, 0, 0) == ["error", "-2"] and run(5, 5, 2) == ["error", "-1"] and run(5, 5, 257 << 8) == ["error", "-2"] and run(-1, 5, 0) == ["error", "-1"]


# ---- the restatements and their gates ----------------------------------------------------------------------------------------------------
def _table():
    v, f, q, _ = MC.region_case()
    yield "regions", q, v, f
    vs, fs = MC.latlon_sphere()
    yield "sphere", MC.queries(200, 1), vs, fs
    yield "sphere-on-surface", MC.on_surface_queries(vs, fs, 200, 2), vs, fs
    v, f = MC.soup(200, 3)
    yield "soup", MC.queries(200, 4), v, f
    for w in (1e-3, 1e-5, 1e-7, 0.0):
        v, f, q = MC.slivers(w, MC.SLIVER_SEED)
        yield f"slivers-{w:g}-random", q[:64], v, f


@pytest.mark.parametrize("name,q,v,f", list(_table()), ids=[c[0] for c in _table()])
def test_float32_restatement_against_float64(name, q, v, f):
    d64, f64, c64, every = MC.restate(q, v, f, want_all=True)
    d32, f32, c32 = MC.restate(q, v, f, np.float32)
    gate = MC.gate_of(q, v)
    assert not np.isnan(d32).any() and not np.isnan(c32).any() and not np.isnan(d64).any()
    worst = float(np.abs(d32 - d64).max())
    print(f"{name}: |d2 - d2_64| = {worst / (MC.EPS * MC.scale_of(q, v)):.3f} * 2^-24 * scale")
    assert worst <= gate
    clear = MC.clear_winner(every, gate)
    assert (f32[clear] == f64[clear]).all()
    rows = np.arange(len(q))
    assert (every[rows, f32] - d64 <= gate).all(), "an unclear winner is still within the gate of the minimum"
    assert np.abs(((q.astype(np.float64) - c64) ** 2).sum(1) - d64).max() <= 1e-12, "closest attains d2 (float64)"
    assert np.abs(((q - c32).astype(np.float64) ** 2).sum(1) - d32).max() <= gate


def test_region_case_by_hand():
    v, f, q, expect = MC.region_case()
    d64 = MC.restate(q, v, f)[0]
    for d, e in zip(d64, expect):
        assert e is None or abs(d - e) < 1e-15
    assert d64[5] > 0.125 ** 2 and d64[10] > 0


def test_case_conditions():
    """What tests/test_hip_metrics.py assumes of its cases: enough queries with a clear winner; zero-area triangles in the sphere."""
    vs, fs = MC.latlon_sphere()
    a, b, c = (vs[fs[:, k]].astype(np.float64) for k in range(3))
    assert (np.linalg.norm(np.cross(b - a, c - a), axis=1) == 0).sum() == 2 * 24, "one zero-area triangle per pole cell"
    for name, q, v, f in (("sphere", MC.queries(129, 1), vs, fs), ("soup", MC.queries(129, 4), *MC.soup(200, 3))):
        every = MC.restate(q, v, f, want_all=True)[3]
        share = MC.clear_winner(every, MC.gate_of(q, v)).mean()
        print(name, "clear winners:", share)
        assert share >= 0.4
    v, f, _ = MC.slivers(0.0, MC.SLIVER_SEED)
    a, b, c = (v[f[:, k]].astype(np.float64) for k in range(3))
    assert (np.cross(b - a, c - a) == 0).all(), "width 0 is exactly collinear in float32"


def _sliver_errors(w, fault=None, dtype=np.float32):
    v, f, q = MC.slivers(w, MC.SLIVER_SEED)
    d64 = MC.restate(q, v, f)[0]
    d = MC.restate(q, v, f, dtype, fault=fault)[0].astype(np.float64)
    return np.abs(np.sqrt(np.maximum(d, 0)) - np.sqrt(d64))


def test_sliver_gates_are_the_measured_ones():
    """The float32 restatement's worst |dist - dist64| per sliver width IS the recorded value (to the two digits it was rounded up to)."""
    for w in MC.SLIVER_WIDTHS:
        worst = float(_sliver_errors(w).max())
        print(f"slivers width {w:g}: restatement |dist - dist64| = {worst:.3e}, recorded {MC.SLIVER_RESTATEMENT_ERR[w]:.1e}")
        assert worst <= MC.SLIVER_RESTATEMENT_ERR[w] <= 1.25 * worst + 1e-9


# ---- seeded faults: each must break a gate ---------------------------------------------------------------------------------------------
def test_fault_region_walk_breaks_the_sliver_gate():
    for w in (1e-3, 1e-5):
        err = _sliver_errors(w, fault="region_walk")
        assert np.nanmax(err) > 10 * MC.SLIVER_KERNEL_FACTOR * MC.SLIVER_RESTATEMENT_ERR[w]
    vs, fs = MC.soup(200, 3)  # ... and is fine on well-shaped triangles: the formulation, not the transcription, is at fault
    q = MC.queries(200, 4)
    assert np.abs(MC.restate(q, vs, fs, np.float32, fault="region_walk")[0] - MC.restate(q, vs, fs)[0]).max() <= MC.gate_of(q, vs)


@pytest.mark.parametrize("fault", ["unclamped_t", "dropped_edge"])
def test_fault_breaks_the_d2_gate(fault):
    v, f, q, _ = MC.region_case()
    d64 = MC.restate(q, v, f)[0]
    assert np.abs(MC.restate(q, v, f, fault=fault)[0] - d64).max() > MC.gate_of(q, v)
    vs, fs = MC.soup(200, 3)
    q = MC.queries(200, 4)
    assert np.abs(MC.restate(q, vs, fs, fault=fault)[0] - MC.restate(q, vs, fs)[0]).max() > MC.gate_of(q, vs)


def test_fault_ge_inside_gives_nan_on_a_zero_area_triangle():
    v = np.asarray([[0, 0, 0], [0.25, 0, 0], [0.5, 0, 0]], np.float32)  # collinear along x
    f = np.asarray([[0, 1, 2]], np.int32)
    q = np.asarray([[0.125, 0.25, 0.0]], np.float32)
    assert np.isnan(MC.restate(q, v, f, fault="ge_inside")[0]).all()
    assert MC.restate(q, v, f)[0][0] == 0.0625 and MC.restate(q, v, f, np.float32)[0][0] == 0.0625
    same = np.zeros((3, 3), np.float32) + 0.25  # three equal vertices
    assert MC.restate(q, same, f, np.float32)[0][0] == np.float32(0.125 ** 2 + 0 + 0.25 ** 2)


def test_fault_highest_index_on_duplicated_faces():
    v, f = MC.duplicated(*MC.soup(20, 5))
    q = MC.queries(50, 6)
    assert (MC.restate(q, v, f)[1] < 20).all() and (MC.restate(q, v, f, np.float32)[1] < 20).all()
    assert (MC.restate(q, v, f, fault="highest_index")[1] >= 20).all()
    v, f, q = MC.shared_edge_case()
    assert (MC.restate(q, v, f)[1] == 0).all() and (MC.restate(q, v, f, np.float32)[1] == 0).all()


# ---- the wiring of metrics.py, on the stand-in --------------------------------------------------------------------------------------------
@pytest.fixture()
def M(P, monkeypatch):
    monkeypatch.setattr(P.ops, "point_mesh_dist2", MC.stand_in_point_mesh_dist2)
    return P.metrics


def _mesh200():
    g = np.random.default_rng(7)
    v = g.uniform(-0.35, 0.35, (200, 3)).astype(np.float32)
    f = g.integers(0, 200, (300, 3)).astype(np.int32)
    return v, f


ROI = ((100, 120), (250, 300))


def test_filter_mesh_against_the_oracle(M):
    v, f = _mesh200()
    for roi in (ROI, ((0, 0), (512, 512)), ((500, 500), (5, 5))):
        ref = MC.filter_mesh_oracle(v, f, roi, 0.7)
        got = M.filter_mesh(torch.from_numpy(v), torch.from_numpy(f), roi, 0.7)
        assert got["faces"].dtype == torch.int32
        assert np.array_equal(got["verts"].numpy(), ref["verts"]) and np.array_equal(got["faces"].numpy(), ref["faces"])
    assert 0 < len(MC.filter_mesh_oracle(v, f, ROI, 0.7)["faces"]) < 300, "the ROI bites"
    empty = M.filter_mesh(torch.from_numpy(v), torch.from_numpy(f), ((500, 500), (5, 5)), 0.7)
    assert empty["faces"].shape == (0, 3), "an ROI that removes every face"
    with pytest.raises(ValueError):
        M.point_mesh_squared_distance(torch.zeros(4, 3), empty["verts"], empty["faces"])


def test_point_mesh_f1_against_the_oracle(M):
    g = np.random.default_rng(8)
    p2s, s2p = g.uniform(0, 0.02, 500), g.uniform(0, 0.03, 400)
    for th in (0.005, 0.01, 0.05):
        ref = MC.f1_oracle(p2s, s2p, th)
        got = M.point_mesh_f1(torch.from_numpy(p2s), torch.from_numpy(s2p), th)
        for k in ("precision", "recall", "f1"):
            assert float(got[k]) == pytest.approx(float(ref[k]), abs=1e-15), k
    zero = M.point_mesh_f1(torch.from_numpy(p2s) + 1, torch.from_numpy(s2p) + 1, 0.005)
    assert float(zero["f1"]) == 0.0 == MC.f1_oracle(p2s + 1, s2p + 1, 0.005)["f1"] and float(zero["precision"]) == 0.0
    half = M.point_mesh_f1(torch.from_numpy(p2s) + 1, torch.from_numpy(s2p) * 0, 0.005)
    assert float(half["f1"]) == 0.0 and float(half["recall"]) == 1.0


def test_geometry_metrics_against_the_oracle(M):
    v, f = _mesh200()
    vp, fp = MC.latlon_sphere(6, 8, 0.3)
    pp, pg = MC.queries(150, 9, 0.4), MC.queries(130, 10, 0.4)
    got = M.geometry_metrics({"verts": torch.from_numpy(vp), "faces": torch.from_numpy(fp)}, {"verts": torch.from_numpy(v), "faces": torch.from_numpy(f)},
                             points_pred=torch.from_numpy(pp), points_gt=torch.from_numpy(pg))
    assert set(got) == {"p2s", "s2p", "cd", "f1_005", "f1_010", "f1_050", "f1_100", "f1_500", "points_pred", "points_gt"}
    p2s = np.sqrt(MC.restate(pp, v, f, np.float32)[0].astype(np.float64))  # measure.py:187-196: pred points to the gt mesh, and back
    s2p = np.sqrt(MC.restate(pg, vp, fp, np.float32)[0].astype(np.float64))
    ref = MC.geometry_oracle(p2s, s2p)
    for k, r in ref.items():
        assert float(got[k]) == pytest.approx(float(r), abs=1e-14), k
    assert 0 < ref["f1_050"] < 1 and ref["f1_500"] == 1.0
    assert got["points_pred"].numpy() is not None and np.array_equal(got["points_pred"].numpy(), pp)
    # without points: sampled on the meshes, n_sample of them, on their faces
    gen = torch.Generator().manual_seed(3)
    got = M.geometry_metrics({"verts": torch.from_numpy(vp), "faces": torch.from_numpy(fp)}, {"verts": torch.from_numpy(v), "faces": torch.from_numpy(f)},
                             n_sample=64, generator=gen)
    assert got["points_pred"].shape == (64, 3) and got["points_gt"].shape == (64, 3)
    assert float(np.abs(np.linalg.norm(got["points_pred"].numpy(), axis=1)).max()) <= 0.3 + 1e-6
    assert MC.restate(got["points_gt"].numpy(), v, f)[0].max() <= 1e-12


def test_wrapper_rejects_bad_faces_before_the_operator(P, monkeypatch):
    monkeypatch.setattr(P.ops, "point_mesh_dist2", lambda *a, **k: pytest.fail("a bad mesh reached the operator"))
    v, f = _mesh200()
    pts, vt = torch.zeros(4, 3), torch.from_numpy(v)
    for bad in (200, -1):
        g = f.copy()
        g[17, 1] = bad
        with pytest.raises(ValueError, match="index"):
            P.metrics.point_mesh_squared_distance(pts, vt, torch.from_numpy(g))
        with pytest.raises(ValueError, match="index"):
            P.metrics.point_mesh_squared_distance(pts, vt, torch.from_numpy(g), cull=True)
    with pytest.raises(ValueError, match="int32"):
        P.metrics.point_mesh_squared_distance(pts, vt, torch.from_numpy(f).long())
    with pytest.raises(ValueError):
        P.metrics.point_mesh_squared_distance(pts, vt, torch.from_numpy(f)[:, :2])
    with pytest.raises(ValueError):
        P.metrics.point_mesh_squared_distance(pts, vt, torch.from_numpy(f.reshape(-1)))


def test_morton_sort_is_undone(M):
    v, f = MC.soup(40, 12)
    q = MC.queries(100, 13)
    plain = M.point_mesh_squared_distance(torch.from_numpy(q), torch.from_numpy(v), torch.from_numpy(f), cull=False)
    seen = {}
    real = MC.stand_in_point_mesh_dist2
    M.ops.point_mesh_dist2 = lambda p, *a, **k: (seen.update(points=p.numpy().copy(), **k), real(p, *a, **k))[1]
    culled = M.point_mesh_squared_distance(torch.from_numpy(q), torch.from_numpy(v), torch.from_numpy(f), cull=True)
    for a, b in zip(plain, culled):
        assert torch.equal(a, b)
    assert not np.array_equal(seen["points"], q) and np.array_equal(np.sort(seen["points"], 0), np.sort(q, 0)), "the operator saw a permutation"
    lo, hi = np.minimum(v.min(0), q.min(0)), np.maximum(v.max(0), q.max(0))
    codes = M.morton_codes(torch.from_numpy(seen["points"]), torch.from_numpy(lo), torch.from_numpy(hi)).numpy()
    assert (np.diff(codes) >= 0).all() and codes.max() < 1 << 30
    assert seen["cull"] is True and seen["cull_margin"] == pytest.approx(64 * 2.0 ** -24 * float(((hi - lo).astype(np.float64) ** 2).sum()), rel=1e-6)
    assert int(M.morton_codes(torch.tensor([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]), torch.zeros(3), torch.ones(3))[0]) == 0x09249249


# ---- the culling case of tests/test_hip_metrics.py really skips ------------------------------------------------------------------------------
def _sorted_like_the_wrapper(P, q, v):
    lo, hi = np.minimum(v.min(0), q.min(0)), np.maximum(v.max(0), q.max(0))
    codes = P.metrics.morton_codes(torch.from_numpy(q), torch.from_numpy(lo), torch.from_numpy(hi))
    margin = P.metrics.CULL_MARGIN_FACTOR * float(((hi - lo).astype(np.float64) ** 2).sum())
    return q[torch.sort(codes)[1].numpy()], margin


def test_far_sliver_tiles_are_skipped(P):
    """An emulation of the kernel's cull test (the seed alone as the bound: a lower bound of what the kernel skips, for every slicing) on
    the far-sliver case: every wave skips all three sliver tiles and keeps the two near ones.  On the other order cases of the GPU
    test the share of skipped visits is printed; only the spheres skip."""
    v, f, q = MC.far_sliver_case()
    qs, margin = _sorted_like_the_wrapper(P, q, v)
    skipped = MC.emulate_cull(qs, v, f, margin)
    assert skipped.shape == (3, 5) and skipped[:, 2:].all() and not skipped[:, :2].any()
    a, b, c = (v[f[128:, k]].astype(np.float64) for k in range(3))
    sin = np.linalg.norm(np.cross(b - a, c - a), axis=1) / (np.linalg.norm(b - a, axis=1) * np.linalg.norm(c - a, axis=1))
    assert sin.max() < 1e-3, "the far tiles hold slivers only"
    d64, f64, _ = MC.restate(q, v, f)
    assert (f64 < 128).all(), "no far face is any query's answer"
    vs, fs = MC.latlon_sphere(24, 48, 0.3)
    qs, margin = _sorted_like_the_wrapper(P, MC.on_surface_queries(vs, fs, 700, 2), vs)
    share = MC.emulate_cull(qs, vs, fs, margin).mean()
    print("sphere-on-surface: skipped visits", share)
    assert share > 0.1


# ---- the sampler ----------------------------------------------------------------------------------------------------------------------------
def test_sample_points_lie_on_their_faces(P):
    v, f = MC.latlon_sphere(6, 8, 0.3)
    pts, idx, bary = P.metrics.sample_points_on_mesh(torch.from_numpy(v), torch.from_numpy(f), 500, generator=torch.Generator().manual_seed(1))
    assert pts.dtype == torch.float32 and pts.shape == (500, 3) and idx.shape == (500,) and bary.shape == (500, 3)
    assert bool((bary >= 0).all()) and float((bary.sum(1) - 1).abs().max()) <= 1e-15
    d2 = np.asarray([MC.restate(p[None], v, f[i:i + 1])[0][0] for p, i in zip(pts.numpy(), idx.numpy())])
    assert np.sqrt(d2).max() <= 1e-6
    a, b, c = (v[f[:, k]].astype(np.float64) for k in range(3))
    area = np.linalg.norm(np.cross(b - a, c - a), axis=1)
    assert (area[idx.numpy()] > 0).all(), "a zero-area face is never drawn"
    again = P.metrics.sample_points_on_mesh(torch.from_numpy(v), torch.from_numpy(f), 500, generator=torch.Generator().manual_seed(1))[0]
    assert torch.equal(pts, again)


def test_sample_counts_follow_the_areas(P):
    v = np.asarray([[0, 0, 0], [1, 0, 0], [0, 2, 0], [3, 0, 0], [3, 2, 0], [3, 0, 6]], np.float32)
    f = np.asarray([[0, 1, 2], [0, 3, 2], [3, 4, 5]], np.int32)  # areas 1 * 2 / 2, 3 * 2 / 2, 2 * 6 / 2
    a, b, c = (v[f[:, k]].astype(np.float64) for k in range(3))
    area = 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1)
    assert np.array_equal(area, [1.0, 3.0, 6.0])
    n = 20000
    idx = P.metrics.sample_points_on_mesh(torch.from_numpy(v), torch.from_numpy(f), n, generator=torch.Generator().manual_seed(5))[1].numpy()
    prob = area / area.sum()
    counts = np.bincount(idx, minlength=3)
    sigma = np.sqrt(n * prob * (1 - prob))
    assert (np.abs(counts - n * prob) <= 5 * sigma).all(), (counts, n * prob, sigma)


def test_sample_on_a_zero_area_mesh_raises(P):
    v = np.asarray([[0, 0, 0], [0.25, 0, 0], [0.5, 0, 0]], np.float32)
    f = np.asarray([[0, 1, 2], [0, 0, 0]], np.int32)
    with pytest.raises(ValueError, match="area"):
        P.metrics.sample_points_on_mesh(torch.from_numpy(v), torch.from_numpy(f), 10)
    with pytest.raises(ValueError):
        P.metrics.sample_points_on_mesh(torch.from_numpy(v), torch.from_numpy(f).long(), 10)


# ---- the end-to-end case's conditions (tests/test_hip_metrics.py, case 6) ----------------------------------------------------------------
def test_end_to_end_radius_leaves_no_point_near_a_threshold():
    """Both meshes of the case are inscribed in one sphere, so a point of one is at most the sum of the two sagittas from the other: far
    below 0.005 - gate at E2E_RADIUS, so no float64 distance sits near the thresholds 0.005 and 0.01 (the GPU test asserts the same on
    the distances themselves)."""
    R, voxel = MC.E2E_RADIUS, MC.E2E_BOX / MC.E2E_N
    v, f = MC.latlon_sphere(MC.E2E_NLAT, MC.E2E_NLON, R)
    centres = v[f].astype(np.float64).mean(1)
    sag = R - np.linalg.norm(centres, axis=1).min()
    sag_mc = 3 * voxel ** 2 / (8 * R)  # a chord no longer than a voxel's diagonal
    print("sagitta of the latitude-longitude sphere:", sag, "bound of the extracted mesh's:", sag_mc, "voxel:", voxel)
    assert sag + sag_mc < 0.005 - 1e-4
