/* p3d_metrics.h — C ABI of the geometry metrics' operator (MI355X / gfx950): the squared distance from points to a triangle mesh, the
 * closest face and the closest point (what `igl.point_mesh_squared_distance` gives `_scripts/eval/measure.py:77-86`), by brute force
 * over every (point, face) pair.
 *
 * Conventions of panic3d_hip.h: raw DEVICE pointers, the stream last, 0 / negative P3D_E_* / positive hipError_t, no allocation
 * (a caller-owned workspace, its size from the *_workspace_bytes query), every argument checked before any launch.
 *
 * THE ARITHMETIC CONTRACT (binary32, round to nearest even, no contraction beyond the fmas named here; vectors are (x, y, z)):
 *   u - v        = (u.x - v.x, u.y - v.y, u.z - v.z)
 *   dot(u, v)    = fma(u.z, v.z, fma(u.y, v.y, u.x * v.x))
 *   cross(u, v)  = (fma(u.y, v.z, -(u.z * v.y)), fma(u.z, v.x, -(u.x * v.z)), fma(u.x, v.y, -(u.y * v.x)))
 *
 *   seg(p; a, b):   ab = b - a;  ap = p - a;  den = dot(ab, ab);  num = dot(ab, ap)
 *                   t  = den > 0 ? min(max(num / den, 0), 1) : 0                    (IEEE division)
 *                   r  = (fma(-t, ab.x, ap.x), fma(-t, ab.y, ap.y), fma(-t, ab.z, ap.z))
 *                   result = dot(r, r);   its point = (fma(t, ab.x, a.x), fma(t, ab.y, a.y), fma(t, ab.z, a.z))
 *   face(p; a, b, c): ab = b - a; ac = c - a; bc = c - b; ca = a - c; ap = p - a; bp = p - b; cp = p - c
 *                   n = cross(ab, ac);  nn = dot(n, n)
 *                   if nn > 0 and dot(cross(ab, ap), n) > 0 and dot(cross(bc, bp), n) > 0 and dot(cross(ca, cp), n) > 0:
 *                       h = dot(n, ap);  result = (h * h) / nn;  its point: w = h / nn, (fma(-w, n.x, p.x), fma(-w, n.y, p.y), fma(-w, n.z, p.z))
 *                   else result = +inf
 *   d2(p, T) = min(min(min(seg(p; a, b), seg(p; b, c)), seg(p; c, a)), face(p; T))
 *
 * The textbook region walk (barycentric coordinates from products of dot products) is NOT used: in binary32 it is wrong by up to
 * 3.6e-2 on thin triangles in a scene of extent 0.7, and marching-cubes meshes are full of slivers.  Here the three segment terms are
 * well conditioned and always an upper bound, and a zero-area triangle (three equal vertices included) degenerates to its edges:
 * no NaN, no special case.  Inputs are finite; every strict comparison above is false on a NaN.
 *
 * Per query: dist2 = the minimum of d2 over the faces; face = the LOWEST face index whose binary32 d2 equals that minimum; closest =
 * the point of the first term, in the order ab, bc, ca, face, that equals d2 of that face.  A minimum is associative and commutative
 * and every (point, face) value is a function of that pair alone, so the outputs do not depend on how the face loop is tiled, sliced
 * or culled: they are bit-identical for every slice count and with culling on or off.
 */
#ifndef P3D_METRICS_H
#define P3D_METRICS_H
#include "panic3d_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define P3D_PM_NO_CULL 1            /* flags bit 0: visit every face tile */
#define P3D_PM_SLICES_SHIFT 8       /* flags bits 8..19: the number of face slices (0: the plan's choice; more than there are face tiles */
#define P3D_PM_SLICES_MASK 0xfff00  /*                   is cut to that; above P3D_PM_MAX_SLICES: P3D_E_RANGE) */
#define P3D_PM_MAX_SLICES 256
#define P3D_PM_QUERY_BLOCK 128      /* queries of one workgroup (one wave, two queries per lane) */
#define P3D_PM_FACE_TILE 64         /* faces of one LDS stage and of one bounding box */
#define P3D_PM_MAX_Q (1 << 26)
#define P3D_PM_MAX_F (1 << 26)

/* The launch shape of p3d_point_mesh_dist2_f32 for Q queries, F faces and these flags: out[0..5] = query blocks, face tiles, face slices,
 * face tiles per slice, P3D_PM_QUERY_BLOCK, P3D_PM_FACE_TILE.  Slice s holds the face tiles [s * tiles_per_slice, (s+1) * tiles_per_slice)
 * that exist; none is empty.  Returns 0, P3D_E_ARG (out NULL, cap < 6, an unknown flag bit, Q < 0) or P3D_E_RANGE (F < 1, Q or F above
 * the maxima, a forced slice count above P3D_PM_MAX_SLICES). */
int p3d_point_mesh_plan(int64_t Q, int64_t F, int flags, int64_t* out, int cap);

/* Bytes of workspace for Q queries against F faces, whatever the flags: the per-face records (64 bytes each), one bounding box and one
 * sample record per face tile, and one seed distance and P3D_PM_MAX_SLICES partial (dist2, face) pairs per query.  0 when Q or F is out
 * of range.  The workspace is 16-byte aligned (P3D_E_ARG otherwise). */
size_t p3d_point_mesh_workspace_bytes(int64_t Q, int64_t F);

/* points [Q][3], verts [V][3], faces [F][3] int32, dist2 [Q], face [Q] int32 (optional), closest [Q][3] (optional).
 * Q = 0 is a no-op that returns 0 (after the checks of the other arguments that do not need Q).  F < 1 or V < 1: P3D_E_RANGE.  The face
 * indices are the caller's responsibility (the Python wrapper checks 0 <= index < V); an index outside [0, V) is read as the nearest
 * valid one, so no load leaves `verts`, and the result for such a mesh is unspecified.
 * Culling (unless P3D_PM_NO_CULL): queries that are neighbours in the array should be neighbours in space (the wrapper sorts them by
 * Morton code).  A wave skips a face tile when, for EVERY query it holds, the squared distance from the query to the tile's box exceeds
 *     min(the query's running dist2, the query's seed)  +  cull_margin  +  the longest squared edge in the tile.
 * The seed of a query is its smallest d2 to the first face of every tile, from a run of the same loop over those faces alone (1/64 of the
 * pairs) in front of the main one: an upper bound of the result that lets every face slice cull from its first tile on.
 * cull_margin >= 0 (P3D_E_ARG otherwise) covers the rounding of every d2 below a true lower bound: 64 * 2^-24 * D^2, D the diagonal of
 * the joint box of mesh and queries; the edge term bounds what an inside test passed on a badly conditioned normal can take off the
 * face term.  Outputs are bit-identical with and without culling.  Nothing but the outputs and the workspace is written. */
int p3d_point_mesh_dist2_f32(const float* points, int64_t Q, const float* verts, int64_t V, const int32_t* faces, int64_t F, int flags,
                             float cull_margin, float* dist2, int32_t* face, float* closest, void* workspace, size_t workspace_bytes,
                             void* stream);

#ifdef __cplusplus
}
#endif
#endif
