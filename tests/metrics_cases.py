"""Shared by tests/test_metrics_cpu.py and tests/test_hip_metrics.py: the case table of the point-to-mesh distance, the restatement of
its arithmetic contract (include/p3d_metrics.h) written from the formulas — brute force over every (point, face) pair, numpy, in
float64 and in float32 — seeded faults of that restatement, a stand-in of ops.point_mesh_dist2 for the CPU wiring tests, and the mesh
builders.  Nothing here imports the package."""
import numpy as np

EPS = 2.0 ** -24
GATE_FACTOR = 8.0  # the project's usual factor on 2^-24 * scale; the float32 restatement measures 0.15


def scale_of(points, verts):
    """3 (max|p|_inf + max|v|_inf)^2: the size of a squared distance's rounding unit."""
    return 3.0 * (float(np.abs(points).max(initial=0.0)) + float(np.abs(verts).max())) ** 2


def gate_of(points, verts):
    return GATE_FACTOR * EPS * scale_of(points, verts)


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
def _fma(a, b, c, dt):
    """fma in dt.  float32: the product of two float32 is exact in float64, the sum is then rounded twice (to 53 bits, to 24): equal to
    the fused result except in rare double-rounding cases, which the gates that compare float32 runs leave room for."""
    if dt == np.float32:
        return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    return a * b + c


def _dot(u, v, dt):
    return _fma(u[..., 2], v[..., 2], _fma(u[..., 1], v[..., 1], u[..., 0] * v[..., 0], dt), dt)


def _cross(u, v, dt):
    return np.stack([_fma(u[..., 1], v[..., 2], -(u[..., 2] * v[..., 1]), dt), _fma(u[..., 2], v[..., 0], -(u[..., 0] * v[..., 2]), dt),
                     _fma(u[..., 0], v[..., 1], -(u[..., 1] * v[..., 0]), dt)], -1)


def _seg(p, a, b, dt, clamp=True):
    ab, ap = b - a, p - a
    den, num = _dot(ab, ab, dt), _dot(ab, ap, dt)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = num / np.where(den > 0, den, dt(1))
    if clamp:
        t = np.minimum(np.maximum(t, dt(0)), dt(1))
    t = np.where(den > 0, t, dt(0)) + np.zeros_like(num)
    r = np.stack([_fma(-t, ab[..., k], ap[..., k], dt) for k in range(3)], -1)
    point = np.stack([_fma(t, ab[..., k], a[..., k], dt) for k in range(3)], -1)
    return _dot(r, r, dt), point


def _face(p, a, b, c, dt, strict=True):
    ab, ac, bc, ca = b - a, c - a, c - b, a - c
    ap, bp, cp = p - a, p - b, p - c
    n = _cross(ab, ac, dt)
    nn = _dot(n, n, dt)
    gt = (lambda x: x > 0) if strict else (lambda x: x >= 0)
    inside = gt(nn) & gt(_dot(_cross(ab, ap, dt), n, dt)) & gt(_dot(_cross(bc, bp, dt), n, dt)) & gt(_dot(_cross(ca, cp, dt), n, dt))
    h = _dot(n, ap, dt)
    with np.errstate(divide="ignore", invalid="ignore"):
        val = np.where(inside, (h * h) / np.where(strict & (nn <= 0), dt(1), nn), dt(np.inf))
        w = h / np.where(nn > 0, nn, dt(1))
    point = np.stack([_fma(-w, n[..., k] + np.zeros_like(h), p[..., k] + np.zeros_like(h), dt) for k in range(3)], -1)
    return val, point


def _region_walk(p, a, b, c, dt):
    """The textbook closest-point walk (barycentric coordinates from products of dot products): the formulation the contract REJECTS.
    Kept as a seeded fault: in float32 it breaks the sliver gate."""
    ab, ac, ap = b - a, c - a, p - a
    d1, d2 = (ab * ap).sum(-1), (ac * ap).sum(-1)
    bp = p - b
    d3, d4 = (ab * bp).sum(-1), (ac * bp).sum(-1)
    cp = p - c
    d5, d6 = (ab * cp).sum(-1), (ac * cp).sum(-1)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    with np.errstate(divide="ignore", invalid="ignore"):
        den = va + vb + vc
        v, w = vb / den, vc / den
        out = a + ab * v[..., None] + ac * w[..., None]
        e_bc = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        out = np.where(((va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0))[..., None], b + (c - b) * e_bc[..., None], out)
        out = np.where(((vb <= 0) & (d2 >= 0) & (d6 <= 0))[..., None], a + ac * (d2 / (d2 - d6))[..., None], out)
        out = np.where(((d6 >= 0) & (d5 <= d6))[..., None], c + np.zeros_like(out), out)
        out = np.where(((vc <= 0) & (d1 >= 0) & (d3 <= 0))[..., None], a + ab * (d1 / (d1 - d3))[..., None], out)
        out = np.where(((d3 >= 0) & (d4 <= d3))[..., None], b + np.zeros_like(out), out)
        out = np.where(((d1 <= 0) & (d2 <= 0))[..., None], a + np.zeros_like(out), out)
    r = p - out
    return (r * r).sum(-1).astype(dt)


FAULTS = ("region_walk", "unclamped_t", "dropped_edge", "ge_inside", "highest_index")


def restate(points, verts, faces, dtype=np.float64, fault=None, want_all=False, chunk=128):
    """d2 [Q], face [Q] int32, closest [Q,3] (and the whole [Q,F] matrix of d2 with want_all) by the contract, every operation in
    `dtype`.  fault: one of FAULTS, a deliberately wrong variant."""
    assert fault is None or fault in FAULTS
    dt = np.float32 if dtype == np.float32 else np.float64
    P, Vv, Fc = np.asarray(points, dt), np.asarray(verts, dt), np.asarray(faces)
    a, b, c = (Vv[Fc[:, k]][None] for k in range(3))
    Q, F = P.shape[0], Fc.shape[0]
    d2, face, closest = np.empty(Q, dt), np.empty(Q, np.int32), np.empty((Q, 3), dt)
    every = np.empty((Q, F), dt) if want_all else None
    for lo in range(0, Q, chunk):
        p = P[lo:lo + chunk, None, :]
        if fault == "region_walk":
            m = _region_walk(p, a, b, c, dt)
            pts = None
        else:
            segs = [_seg(p, a, b, dt, clamp=fault != "unclamped_t"), _seg(p, b, c, dt, clamp=fault != "unclamped_t"),
                    _seg(p, c, a, dt, clamp=fault != "unclamped_t")]
            if fault == "dropped_edge":
                segs[2] = (np.full_like(segs[2][0], np.inf), segs[2][1])
            fc = _face(p, a, b, c, dt, strict=fault != "ge_inside")
            terms = np.stack([s[0] for s in segs] + [fc[0]], 0)  # [4,q,F]
            pts = np.stack([s[1] + np.zeros_like(fc[1]) for s in segs] + [fc[1]], 0)
            m = np.minimum(np.minimum(np.minimum(terms[0], terms[1]), terms[2]), terms[3])
        f = (F - 1 - np.argmin(m[:, ::-1], 1)) if fault == "highest_index" else np.argmin(m, 1)
        rows = np.arange(m.shape[0])
        d2[lo:lo + chunk], face[lo:lo + chunk] = m[rows, f], f
        if pts is not None:
            which = np.argmax(terms[:, rows, f] == m[rows, f][None], 0)  # the first term, in the order ab, bc, ca, face, that attains it
            closest[lo:lo + chunk] = pts[which, rows, f]
        else:
            closest[lo:lo + chunk] = np.nan
        if want_all:
            every[lo:lo + chunk] = m
    return (d2, face, closest, every) if want_all else (d2, face, closest)


def distance_to_face64(points, verts, faces, face_index):
    """float64 squared distance from points[i] to the ONE face face_index[i]."""
    out = np.empty(len(points))
    V64 = np.asarray(verts, np.float64)
    for i, (p, f) in enumerate(zip(np.asarray(points, np.float64), np.asarray(face_index))):
        out[i] = restate(p[None], V64, np.asarray(faces)[f:f + 1])[0][0]
    return out


def clear_winner(every64, gate):
    """Queries whose float64 best and second-best face distances differ by more than the gate: where `face` is comparable."""
    if every64.shape[1] < 2:
        return np.ones(every64.shape[0], bool)
    s = np.sort(every64, 1)
    return (s[:, 1] - s[:, 0]) > gate


def stand_in_point_mesh_dist2(points, verts, faces, cull=False, cull_margin=0.0, slices=0, want_face=True, want_closest=True):
    """ops.point_mesh_dist2 on torch CPU tensors: the float32 restatement.  For the wiring tests of panic3d_amd/metrics.py."""
    import torch
    assert points.dtype == torch.float32 and verts.dtype == torch.float32 and faces.dtype == torch.int32
    d2, f, c = restate(points.numpy(), verts.numpy(), faces.numpy(), np.float32)
    return torch.from_numpy(d2), torch.from_numpy(f) if want_face else None, torch.from_numpy(c) if want_closest else None


# ---- meshes ----------------------------------------------------------------------------------------------------------------------------
def latlon_sphere(nlat=12, nlon=24, radius=0.3, center=(0.0, 0.0, 0.0)):
    """A latitude-longitude sphere: (nlat + 1) x nlon vertices (each pole nlon times), two triangles per cell — one of the two in a
    pole row has zero area.  verts [V,3] float32, faces [F,3] int32."""
    th = np.pi * np.arange(nlat + 1) / nlat
    ph = 2 * np.pi * np.arange(nlon) / nlon
    T, Ph = np.meshgrid(th, ph, indexing="ij")
    v = np.stack([np.sin(T) * np.cos(Ph), np.sin(T) * np.sin(Ph), np.cos(T)], -1).reshape(-1, 3) * radius + np.asarray(center)
    v[:nlon] = v[0]  # the poles exactly
    v[-nlon:] = v[-1]
    idx = lambda i, j: i * nlon + (j % nlon)
    f = []
    for i in range(nlat):
        for j in range(nlon):
            f.append((idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)))
            f.append((idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)))
    return v.astype(np.float32), np.asarray(f, np.int32)


def soup(F, seed, extent=0.35, size=0.08):
    """F random triangles, each with its own three vertices."""
    g = np.random.default_rng(seed)
    c = g.uniform(-extent, extent, (F, 1, 3))
    v = (c + g.normal(0, size, (F, 3, 3))).reshape(-1, 3)
    return v.astype(np.float32), np.arange(3 * F, dtype=np.int32).reshape(F, 3)


def queries(Q, seed, extent=0.45):
    return np.random.default_rng(seed).uniform(-extent, extent, (Q, 3)).astype(np.float32)


def on_surface_queries(verts, faces, Q, seed):
    """Points on the faces (float32 roundings of them): d2 ~ 0, the adversarial case of the culling margin."""
    g = np.random.default_rng(seed)
    f = g.integers(0, len(faces), Q)
    w = g.dirichlet((1, 1, 1), Q)
    tri = verts[faces[f]].astype(np.float64)
    return (w[:, :, None] * tri).sum(1).astype(np.float32)


SLIVER_WIDTHS = (1e-3, 1e-5, 1e-7, 0.0)
SLIVER_HEIGHTS = (0.0, 1e-4, 5e-3, 1e-1)


def slivers(width, seed, n=24):
    """n thin triangles a, b, c = a + ab / 2 + width * perp with dyadic a and ab, so width 0 is EXACTLY collinear in float32; and the
    queries: random ones, and ones placed above each sliver's interior at SLIVER_HEIGHTS along the sliver's normal.
    verts, faces, queries."""
    g = np.random.default_rng(seed)
    q12 = lambda x: np.round(x * 4096) / 4096
    a = q12(g.uniform(-0.3, 0.3, (n, 3)))
    ab = q12(g.uniform(-0.25, 0.25, (n, 3)))
    ab[np.abs(ab).sum(1) == 0] = 1 / 4096
    r = g.normal(size=(n, 3))
    perp = np.cross(ab, r)
    perp /= np.linalg.norm(perp, axis=1, keepdims=True)
    normal = np.cross(ab, perp)
    normal /= np.linalg.norm(normal, axis=1, keepdims=True)
    c = a + ab / 2 + width * perp
    verts = np.stack([a, a + ab, c], 1).reshape(-1, 3).astype(np.float32)
    faces = np.arange(3 * n, dtype=np.int32).reshape(n, 3)
    inner = a + 0.45 * ab + 0.4 * width * perp  # inside the triangle
    above = np.concatenate([inner + h * normal for h in SLIVER_HEIGHTS])
    return verts, faces, np.concatenate([queries(64, seed + 1), above.astype(np.float32)])


# Worst |dist - dist64| (distances, not squares) of the float32 restatement on slivers(width, SLIVER_SEED), measured by
# tests/test_metrics_cpu.py::test_sliver_gates_are_the_measured_ones and rounded up to two digits.  tests/test_hip_metrics.py holds the
# kernel to SLIVER_KERNEL_FACTOR times these: the same arithmetic, and the margin covers an fma's double rounding in the restatement.
SLIVER_SEED = 11
SLIVER_RESTATEMENT_ERR = {1e-3: 2.1e-7, 1e-5: 2.3e-5, 1e-7: 4.4e-8, 0.0: 1.2e-8}
SLIVER_KERNEL_FACTOR = 4.0


def region_case():
    """One triangle and queries in each of its seven Voronoi regions (above the plane, so every term is exercised), then exactly on a
    vertex, on an edge, in the plane inside, and in the plane outside."""
    verts = np.asarray([[0.0, 0.0, 0.0], [0.5, 0.0, 0.0], [0.0, 0.375, 0.0]], np.float32)
    faces = np.asarray([[0, 1, 2]], np.int32)
    z = 0.125
    q = [(0.125, 0.125, z),      # the face
         (-0.25, -0.25, z),     # vertex a
         (0.75, -0.125, z),     # vertex b
         (-0.125, 0.625, z),    # vertex c
         (0.25, -0.25, z),      # edge ab
         (0.375, 0.3125, z),    # edge bc
         (-0.25, 0.1875, z),    # edge ca
         (0.5, 0.0, 0.0),       # exactly on vertex b
         (0.25, 0.0, 0.0),      # exactly on edge ab
         (0.125, 0.125, 0.0),   # in the plane, inside
         (0.5, 0.5, 0.0)]       # in the plane, outside
    expect = [z * z, 0.125 + z * z, 0.0625 + 0.015625 + z * z, 0.015625 + 0.0625 + z * z, 0.0625 + z * z, None, 0.0625 + z * z, 0.0, 0.0, 0.0, None]
    return verts, faces, np.asarray(q, np.float32), expect


def duplicated(verts, faces):
    """Every face twice: face i again at index i + F."""
    return verts, np.concatenate([faces, faces])


def shared_edge_case():
    """Two triangles that share the edge (0,0,0)-(1,0,0) and queries straight above that edge: equidistant from both faces."""
    verts = np.asarray([[0, 0, 0], [1, 0, 0], [0.5, 1, 0], [0.5, -1, 0]], np.float32)
    faces = np.asarray([[0, 1, 2], [1, 0, 3]], np.int32)
    q = np.asarray([[0.25, 0, 0.5], [0.5, 0, 0.25], [0.75, 0, 1.0], [0.5, 0, 0.0]], np.float32)
    return verts, faces, q


# The end-to-end case: volume.marching_cubes of sphere_density(E2E_N, E2E_RADIUS_VOXELS) in a box of width E2E_BOX against a
# latitude-longitude sphere of the same radius and centre.  marching_cubes maps index i to i / n * box - box / 2, so the grid's centre
# (n - 1) / 2 lands at E2E_CENTER on every axis.  Both meshes are inscribed in the sphere, and their sagittas are far below 0.005.
E2E_N, E2E_BOX, E2E_RADIUS_VOXELS, E2E_NLAT, E2E_NLON = 24, 0.7, 8.0, 24, 48
E2E_RADIUS = E2E_RADIUS_VOXELS / E2E_N * E2E_BOX
E2E_CENTER = ((E2E_N - 1) / 2 / E2E_N - 0.5) * E2E_BOX


def sphere_density(n, radius_voxels):
    """An analytic density whose 0.5 level is a sphere of radius_voxels around the grid's centre: [n,n,n] float32."""
    i = np.arange(n, dtype=np.float64) - (n - 1) / 2
    r = np.sqrt(i[:, None, None] ** 2 + i[None, :, None] ** 2 + i[None, None, :] ** 2)
    return (0.5 + (radius_voxels - r) * 0.25).astype(np.float32)


# ---- oracles of the host wiring (plain Python from the stated semantics; tests/test_metrics_cpu.py) -------------------------------------
def filter_mesh_oracle(verts, faces, roi, bw, size=512):
    """What metrics.filter_mesh promises, vertex by vertex and face by face: keep a vertex strictly inside the rectangle of the region
    of interest — ((row, column), (height, width)) in pixels of a size^2 view of a box of width bw; columns along +x from -bw/2, rows
    along -y from +bw/2 —, keep a face when its three vertices are kept, and renumber through a dictionary of the survivors."""
    (row, col), (height, width) = roi
    left = -bw / 2 + ((col / size) * bw)
    top = bw / 2 - ((row / size) * bw)
    right, bottom = left + bw * (width / size), top - bw * (height / size)
    remap, kept = {}, []
    for i, vert in enumerate(verts):
        if left < vert[0] < right and bottom < vert[1] < top:
            remap[i] = len(kept)
            kept.append(vert)
    out = [[remap[int(i)] for i in tri] for tri in faces if all(int(i) in remap for i in tri)]
    return {"verts": np.asarray(kept, verts.dtype).reshape(-1, 3), "faces": np.asarray(out, np.int64).reshape(-1, 3)}


def f1_oracle(p2s, s2p, thresh):
    """Precision = the share of predicted points within thresh of the ground truth, recall = the share of ground-truth points within
    thresh of the prediction, F1 = their harmonic mean, 0 when there is nothing to average."""
    precision = sum(1 for d in p2s if d <= thresh) / len(p2s)
    recall = sum(1 for d in s2p if d <= thresh) / len(s2p)
    f1 = 0.0 if precision + recall == 0 else 2 * precision * recall / (precision + recall)
    return {"precision": precision, "recall": recall, "f1": f1}


def geometry_oracle(p2s, s2p, thresholds=(0.005, 0.01, 0.05, 0.1, 0.5)):
    """The scalars of metrics.geometry_metrics from the two arrays of distances: their means, the Chamfer distance as the mean of the
    two, and F1 per threshold under the key f1_XXX, XXX = the threshold in thousandths."""
    out = {"p2s": float(np.mean(p2s)), "s2p": float(np.mean(s2p))}
    out["cd"] = 0.5 * (out["p2s"] + out["s2p"])
    for th in thresholds:
        out["f1_%03d" % round(th * 1000)] = f1_oracle(p2s, s2p, th)["f1"]
    return out


# ---- culling: a case that really skips, and an emulation that shows it ---------------------------------------------------------------------
def far_sliver_case(seed=21, n_near=128, n_far=192, n_queries=300):
    """Two tiles of ordinary small triangles around a cluster of queries, then three tiles of slivers (widths 1e-6 ... 0, edges ~0.02:
    normals that are rounding noise) packed into a small box about 1.2 away: compact, far, and skipped.  verts, faces, queries."""
    g = np.random.default_rng(seed)
    c = g.uniform(-0.1, 0.1, (n_near, 1, 3))
    near = (c + g.normal(0, 0.01, (n_near, 3, 3))).reshape(-1, 3)
    a = np.asarray([1.2, 0.1, -0.1]) + g.uniform(-0.03, 0.03, (n_far, 3))
    ab = g.normal(0, 0.012, (n_far, 3))
    perp = np.cross(ab, g.normal(size=(n_far, 3)))
    perp /= np.linalg.norm(perp, axis=1, keepdims=True)
    width = np.asarray([1e-6, 1e-7, 1e-8, 0.0])[np.arange(n_far) % 4][:, None]
    far = np.stack([a, a + ab, a + ab * g.uniform(0.2, 0.8, (n_far, 1)) + width * perp], 1).reshape(-1, 3)
    verts = np.concatenate([near, far]).astype(np.float32)
    faces = np.arange(3 * (n_near + n_far), dtype=np.int32).reshape(-1, 3)
    return verts, faces, g.uniform(-0.12, 0.12, (n_queries, 3)).astype(np.float32)


def emulate_cull(sorted_points, verts, faces, margin, wave=128, tile=64):
    """Which (wave, tile) visits the kernel's culling is SURE to skip, whatever the slicing: the test of include/p3d_metrics.h with
    the seed alone as the bound (the running minimum can only lower it).  sorted_points: in the order the kernel sees them.  Returns a
    bool array [waves, tiles].  float64 geometry on the float32 data; a visit within 1e-6 of the threshold counts as not skipped."""
    P, V = np.asarray(sorted_points, np.float64), np.asarray(verts, np.float64)
    tri = V[np.asarray(faces)]
    ntiles = -(-len(faces) // tile)
    seed = restate(sorted_points, verts, np.asarray(faces)[::tile], np.float32)[0].astype(np.float64)
    skipped = np.zeros((-(-len(P) // wave), ntiles), bool)
    for t in range(ntiles):
        part = tri[t * tile:(t + 1) * tile]
        lo, hi = part.min((0, 1)), part.max((0, 1))
        edge = max(((part[:, k] - part[:, (k + 1) % 3]) ** 2).sum(1).max() for k in range(3))
        gap2 = (np.maximum(0, np.maximum(lo - P, P - hi)) ** 2).sum(1)
        wanted = ~(gap2 > seed + margin + edge + 1e-6)
        for w in range(skipped.shape[0]):
            skipped[w, t] = not wanted[w * wave:(w + 1) * wave].any()
    return skipped
