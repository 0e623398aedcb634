"""GPU: the point-to-mesh distance kernels (csrc/p3d_metrics.hip) against the float64 restatement of tests/metrics_cases.py under the
project's gate — regions of one triangle, ragged shapes with canaries, slivers, ties — the bit-identity of every tiling, slicing and
culling of the face loop, and the geometry metrics end to end on a mesh extracted on the device.  On the parent commit the module, the
operator and the symbols do not exist."""
import numpy as np
import pytest
import torch

import metrics_cases as MC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P():
    import panic3d_amd
    panic3d_amd.build()
    panic3d_amd._lib.lib()
    return panic3d_amd


def _run(P, q, v, f, **kw):
    out = P.metrics.point_mesh_squared_distance(torch.from_numpy(q).cuda(), torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda(), **kw)
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out)


def _check(q, v, f, d2, face, closest, name):
    """The gates of cases 1 and 2: d2, face where float64 has a clear winner (a within-gate face elsewhere), closest."""
    d64, f64, _, every = MC.restate(q, v, f, want_all=True)
    gate, scale = MC.gate_of(q, v), MC.scale_of(q, v)
    assert not np.isnan(d2).any() and not np.isnan(closest).any(), name
    print(f"{name}: |d2 - d2_64| = {np.abs(d2 - d64).max() / (MC.EPS * scale):.3f} * 2^-24 * scale")
    assert np.abs(d2 - d64).max() <= gate, name
    clear = MC.clear_winner(every, gate)
    assert clear.mean() >= 0.4, (name, "a condition on the case", clear.mean())
    assert ((face >= 0) & (face < len(f))).all() and (face[clear] == f64[clear]).all(), name
    rows = np.arange(len(q))
    assert (every[rows, face] - d64 <= gate).all(), name
    c64 = closest.astype(np.float64)
    assert np.abs(((q.astype(np.float64) - c64) ** 2).sum(1) - d2).max() <= gate, (name, "|p - C|^2 = d2")
    off = np.sqrt([MC.restate(c[None], v, f[i:i + 1])[0][0] for c, i in zip(c64, face)])
    assert off.max() <= 4 * MC.EPS * np.sqrt(scale), (name, "C lies on the returned face")


# ---- 1. regions ---------------------------------------------------------------------------------------------------------------------------
def test_regions_of_one_triangle(P):
    v, f, q, expect = MC.region_case()
    for cull in (False, True):
        d2, face, closest = _run(P, q, v, f, cull=cull)
        _check(q, v, f, d2, face, closest, f"regions cull={cull}")
        assert (face == 0).all() and (d2[7:10] == 0).all(), "on a vertex, on an edge, in the plane inside: exactly 0"
        assert np.array_equal(closest[7:10], q[7:10])


# ---- 2. ragged shapes -----------------------------------------------------------------------------------------------------------------------
QS = (1, 63, 64, 65, 129)               # ..., one above the query block (P3D_PM_QUERY_BLOCK = 128)
FS = ((1, 0), (63, 0), (64, 0), (65, 0), (129, 2))  # (F, forced slices): 65 = one above the face tile AND above a slice of one tile (the
#                                         plan's choice at these sizes); 129 with two slices = one above a slice of two tiles
CANARY = 64


def _raw_call(P, q, v, f, flags, margin=0.0):
    """p3d_point_mesh_dist2_f32 on buffers with canaries around the three outputs and past the stated workspace size."""
    L, C = P._lib.lib(), P._lib.C
    dev = torch.device("cuda")
    Q, V, F = len(q), len(v), len(f)
    qd, vd, fd = torch.from_numpy(q).to(dev), torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    need = L.p3d_point_mesh_workspace_bytes(Q, F)
    ws = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device=dev)
    bufs = {k: torch.full((CANARY + n + CANARY,), s, dtype=t, device=dev)
            for k, n, s, t in (("d2", Q, -7.0, torch.float32), ("face", Q, -7, torch.int32), ("closest", 3 * Q, -7.0, torch.float32))}
    ptr = lambda t, off: C.c_void_p(t.data_ptr() + off * t.element_size())
    rc = L.p3d_point_mesh_dist2_f32(ptr(qd, 0), Q, ptr(vd, 0), V, ptr(fd, 0), F, flags, margin, ptr(bufs["d2"], CANARY), ptr(bufs["face"], CANARY),
                                    ptr(bufs["closest"], CANARY), ptr(ws, 0), need, P.ops._stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert bool((ws[need:] == 0xA5).all()), "the workspace past its stated size"
    out = {}
    for k, b in bufs.items():
        b = b.cpu().numpy()
        assert (b[:CANARY] == -7).all() and (b[-CANARY:] == -7).all(), f"canaries around {k}"
        out[k] = b[CANARY:-CANARY]
    return out["d2"], out["face"], out["closest"].reshape(Q, 3)


@pytest.mark.parametrize("F,slices", FS)
@pytest.mark.parametrize("Q", QS)
def test_ragged_soup(P, Q, F, slices):
    v, f = MC.soup(F, 20 + F)
    q = MC.queries(Q, 7 if Q == 1 else 30 + Q)
    flags = P._lib.P3D_PM_NO_CULL | (slices << P._lib.P3D_PM_SLICES_SHIFT)
    plan = P.ops.point_mesh_plan(Q, F, slices=slices)
    assert plan["qblocks"] == -(-Q // 128) and plan["ntiles"] == -(-F // 64) and plan["slices"] == (slices or plan["ntiles"])
    d2, face, closest = _raw_call(P, q, v, f, flags)
    _check(q, v, f, d2, face, closest, f"soup Q={Q} F={F}")
    # culling on, a non-zero margin: the seeding launches, the sample records and the seed array under the same canaries
    margin = P.metrics.CULL_MARGIN_FACTOR * float(((np.maximum(v.max(0), q.max(0)) - np.minimum(v.min(0), q.min(0))).astype(np.float64) ** 2).sum())
    culled = _raw_call(P, q, v, f, slices << P._lib.P3D_PM_SLICES_SHIFT, margin)
    assert margin > 0 and all(np.array_equal(a, b) for a, b in zip((d2, face, closest), culled)), "culling on, under canaries"
    again = _run(P, q, v, f, cull=False, slices=slices)
    assert all(np.array_equal(a, b) for a, b in zip((d2, face, closest), again)), "the wrapper and the raw call"


@pytest.mark.parametrize("F", (65, 576))
@pytest.mark.parametrize("Q", QS)
def test_ragged_sphere_with_zero_area_triangles(P, Q, F):
    v, f = MC.latlon_sphere()
    f = f[:F]  # the first 48 faces are the north pole's row: every second one has zero area
    q = MC.queries(Q, {65: 10, 576: 8}[F] if Q == 1 else 40 + Q)  # (the single query: one whose float64 winner is clear)
    if F < 576:
        q[:, 2] = np.abs(q[:, 2]) * 0.5 + 0.3  # above the cap, so the nearest face is inside it, not on its rim
    d2, face, closest = _raw_call(P, q, v, f, P._lib.P3D_PM_NO_CULL)
    _check(q, v, f, d2, face, closest, f"sphere Q={Q} F={F}")


# ---- 3. slivers -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", MC.SLIVER_WIDTHS)
def test_slivers(P, width):
    v, f, q = MC.slivers(width, MC.SLIVER_SEED)
    d64 = MC.restate(q, v, f)[0]
    for cull in (False, True):
        d2, face, closest = _run(P, q, v, f, cull=cull)
        assert not np.isnan(d2).any() and not np.isnan(closest).any() and (d2 >= 0).all()
        err = np.abs(np.sqrt(d2.astype(np.float64)) - np.sqrt(d64))
        print(f"slivers width {width:g} cull={cull}: |dist - dist64| = {err.max():.3e}; the restatement's {MC.SLIVER_RESTATEMENT_ERR[width]:.1e}")
        assert err.max() <= MC.SLIVER_KERNEL_FACTOR * MC.SLIVER_RESTATEMENT_ERR[width]


# ---- 4. ties ----------------------------------------------------------------------------------------------------------------------------------
def test_ties_take_the_lowest_index(P):
    v, f0 = MC.soup(100, 5)
    v, f = MC.duplicated(v, f0)  # 200 faces: the copies sit in other tiles and, with 4 slices, in other slices
    q = MC.queries(300, 6)
    base = _run(P, q, v, f0, cull=False)
    for kw in (dict(cull=False), dict(cull=True), dict(cull=False, slices=4), dict(cull=False, slices=1)):
        d2, face, closest = _run(P, q, v, f, **kw)
        assert (face < 100).all(), kw
        assert all(np.array_equal(a, b) for a, b in zip((d2, face, closest), base)), kw
    v, f, q = MC.shared_edge_case()
    for cull in (False, True):
        d2, face, closest = _run(P, q, v, f, cull=cull)
        assert (face == 0).all() and np.array_equal(d2, q[:, 2] ** 2), "equidistant from both faces: the lower index"
    d2, face, _ = _run(P, q, v, f[::-1].copy(), cull=False)
    assert (face == 0).all(), "... whichever of the two comes first"


# ---- 5. order independence ------------------------------------------------------------------------------------------------------------------
def _order_cases():
    vs, fs = MC.latlon_sphere(24, 48, 0.3)  # 2304 faces in latitude order: 36 tiles whose boxes are thin bands
    yield "sphere-on-surface", MC.on_surface_queries(vs, fs, 700, 2), vs, fs
    yield "sphere-random", MC.queries(300, 3), vs, fs
    v, f = MC.soup(1000, 3, size=0.02)
    yield "soup", MC.queries(300, 4), v, f
    order = np.argsort(v[f].mean(1)[:, 0], kind="stable")  # the same soup with its faces sorted along x: tiles that can be culled
    yield "soup-sorted", MC.queries(300, 4), v, f[order].copy()
    v, f, q = MC.far_sliver_case()  # (tests/test_metrics_cpu.py shows that every wave skips its three sliver tiles)
    yield "far-slivers", q, v, f
    parts = [MC.slivers(w, MC.SLIVER_SEED + i, n=48) for i, w in enumerate(MC.SLIVER_WIDTHS)]
    v = np.concatenate([p[0] for p in parts])
    f = np.concatenate([p[1] + 3 * 48 * i for i, p in enumerate(parts)]).astype(np.int32)
    yield "slivers", np.concatenate([p[2] for p in parts]), v, f


@pytest.mark.parametrize("name,q,v,f", list(_order_cases()), ids=[c[0] for c in _order_cases()])
def test_every_order_gives_the_same_bits(P, name, q, v, f):
    base = _run(P, q, v, f, cull=False)
    assert not np.isnan(base[0]).any()
    variants = [dict(cull=False), dict(cull=True), dict(cull=False, sort=True), dict(cull=True, sort=False)] + \
               [dict(cull=c, slices=s) for c in (False, True) for s in (1, 2, 3, 7, 256)]
    for kw in variants:
        out = _run(P, q, v, f, **kw)
        for what, a, b in zip(("dist2", "face", "closest"), base, out):
            assert np.array_equal(a.view(np.int32), b.view(np.int32)), (name, kw, what, int((a != b).sum()))
    if name == "sphere-on-surface":
        assert base[0].max() <= MC.gate_of(q, v), "d2 ~ 0: the adversarial case of the margin"


# ---- 6. end to end ----------------------------------------------------------------------------------------------------------------------------
def test_geometry_metrics_end_to_end(P):
    n, box = MC.E2E_N, MC.E2E_BOX
    vol = torch.from_numpy(MC.sphere_density(n, MC.E2E_RADIUS_VOXELS)).cuda()
    pred = P.volume.marching_cubes(vol, None, box, level=0.5)  # numpy arrays, as generate.py stores them
    pred_t = P.volume.marching_cubes(vol, None, box, level=0.5, as_tensors=True)
    assert torch.is_tensor(pred_t["verts"]) and pred_t["verts"].is_cuda and np.array_equal(pred_t["verts"].cpu().numpy(), pred["verts"])
    assert np.array_equal(pred_t["faces"].cpu().numpy(), pred["faces"]) and pred["faces"].dtype == np.int32 and len(pred["faces"]) > 1000
    vg, fg = MC.latlon_sphere(MC.E2E_NLAT, MC.E2E_NLON, MC.E2E_RADIUS, (MC.E2E_CENTER,) * 3)
    gt = {"verts": vg, "faces": fg}
    gen = torch.Generator(device="cuda").manual_seed(4)
    got = P.geometry_metrics(pred_t, gt, n_sample=2000, generator=gen)
    assert set(got) == {"p2s", "s2p", "cd", "f1_005", "f1_010", "f1_050", "f1_100", "f1_500", "points_pred", "points_gt"}
    assert all(torch.is_tensor(x) and x.is_cuda for x in got.values())
    pp, pg = got["points_pred"].cpu().numpy(), got["points_gt"].cpu().numpy()
    assert pp.shape == (2000, 3) and pg.shape == (2000, 3)
    d_p2s = MC.restate(pp, vg, fg, chunk=64)[0]
    d_s2p = MC.restate(pg, pred["verts"], pred["faces"], chunk=64)[0]
    assert MC.restate(pp[:100], pred["verts"], pred["faces"])[0].max() <= 1e-12 and MC.restate(pg[:100], vg, fg)[0].max() <= 1e-12, "on their meshes"
    p2s, s2p = np.sqrt(d_p2s), np.sqrt(d_s2p)
    ref = MC.geometry_oracle(p2s, s2p)
    for k in ("p2s", "s2p", "cd"):
        print(k, float(got[k]), ref[k])
        assert abs(float(got[k]) - ref[k]) <= 1e-6, k
    # F1: equal once the points within the d2 gate of a threshold are left out — at most 0.5 % of a case, none at 0.005 and 0.01
    gates = (MC.gate_of(pp, vg), MC.gate_of(pg, pred["verts"]))
    gp = P.point_mesh_squared_distance(pp, vg, fg)[0].cpu().numpy().astype(np.float64)
    gs = P.point_mesh_squared_distance(pg, pred["verts"], pred["faces"])[0].cpu().numpy().astype(np.float64)
    assert np.abs(gp - d_p2s).max() <= gates[0] and np.abs(gs - d_s2p).max() <= gates[1]
    for th in (0.005, 0.01, 0.05, 0.1, 0.5):
        keep_p, keep_s = np.abs(d_p2s - th * th) > gates[0], np.abs(d_s2p - th * th) > gates[1]
        assert (~keep_p).mean() <= 0.005 and (~keep_s).mean() <= 0.005
        if th <= 0.01:
            assert keep_p.all() and keep_s.all(), "the radius leaves no float64 distance near this threshold"
        assert np.array_equal(np.sqrt(gp[keep_p]) <= th, p2s[keep_p] <= th) and np.array_equal(np.sqrt(gs[keep_s]) <= th, s2p[keep_s] <= th)
        if keep_p.all() and keep_s.all():
            assert float(got["f1_%03d" % round(th * 1000)]) == pytest.approx(MC.f1_oracle(p2s, s2p, th)["f1"], abs=1e-15)
    voxel = box / n
    print(f"cd = {float(got['cd']):.3e} = {float(got['cd']) / voxel:.4f} voxels of {voxel:.3e}")
    assert float(got["cd"]) < voxel, "the extractor's geometric error, a first number: below one voxel"
