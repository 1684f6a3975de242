/*
 * shader_ray_winding.h -- generalized winding numbers on a resident scene: caller-supplied points in, how many times the
 * scene's surface winds around each point out, robust on open, non-manifold and self-intersecting meshes; and a signed
 * distance whose sign comes from it.
 *
 * libshray_winding.so implements it, a client of libshray_hip.so (include/shader_ray_hip.h): a scene created there is queried
 * here, and errors are read with shray_last_error().  The winding number is that of Jacobson, Kavan and Sorkine-Hornung
 * (Robust inside-outside segmentation using generalized winding numbers, SIGGRAPH 2013), evaluated by the tree walk over
 * per-node dipole expansions of Barill, Dickson, Schmidt, Levin and Jacobson (Fast winding numbers for soups and clouds,
 * SIGGRAPH 2018), DESIGN section 13.
 *
 * Semantics.  Arithmetic as in include/shader_ray_point.h: IEEE fp32, single rounding, no FMA contraction, correctly rounded
 * division and square root, dot(x, y) = (x.x*y.x + x.y*y.y) + x.z*y.z, cross(u, w) = (u.y*w.z - u.z*w.y, u.z*w.x - u.x*w.z,
 * u.x*w.y - u.y*w.x), max(x, y) = x > y ? x : y.  Vector + - and scalar * / act per component.  Triangle t has corners
 * a, b, c = positions[9t .. 9t+8].  The tree is the scene's packed tree (csrc/packed_layout.h): node k is the k-th in its
 * pre-order (name 4k), lo and hi its box from octant copy 7 (entry and exit planes), a branch's negative child the one copy
 * 7's a' names, the positive child its b'.  Sums start from +0 and add one term at a time in the order given.
 *   - Per triangle: n = cross(b-a, c-a); N_t = n * 0.5; A_t = 0.5 * sqrtf(dot(n, n)); x_t = ((a + b) + c) / 3.
 *   - Per node, one record of SHRAY_WINDING_DATA_FLOATS floats: { P[3], r, N[3], A, M[9] row-major, 0, 0, 0 }.
 *       leaf, over its triangles in index order:  A = sum A_t;  S = sum A_t * x_t (S = S + x_t * A_t);  N = sum N_t;
 *             P = S / A, or (lo + hi) * 0.5 when A == 0;  then M_ij = sum (x_t,i - P_i) * N_t,j, i the row.
 *       branch, negative child n, positive child p:  A = A_n + A_p;  P = (P_n * A_n + P_p * A_p) / A, or (lo + hi) * 0.5 when
 *             A == 0;  N = N_n + N_p;  M_ij = (M_n,ij + (P_n,i - P_i) * N_n,j) + (M_p,ij + (P_p,i - P_i) * N_p,j).
 *       every node:  r = sqrtf(max(max(...max(e_0, e_1)..., e_6), e_7)), e_c = dot(k_c - P, k_c - P), k_c the box corner
 *             (bit 0 of c: hi.x else lo.x, bit 1: y, bit 2: z).
 *   - Query w(q; beta), q the point's p (its max_dist2 is ignored).  A point with a non-finite coordinate gives NaN.  Else
 *     w = +0, and from the root, depth first in pre-order (the negative child first, the positive one when the negative
 *     subtree is done), at each node:
 *       d = P - q, d2 = dot(d, d), br = beta * r.  If d2 > br * br (far): w = w + T_far and the subtree is skipped, with
 *         len = sqrtf(d2), i3 = 1 / (d2 * len), i5 = i3 / d2, tr = (M_00 + M_11) + M_22, m_i = (M_i0*d.x + M_i1*d.y) + M_i2*d.z,
 *         T_far = (((dot(N, d) + tr) * i3) - ((3 * dot(d, m)) * i5)) * K4,  K4 = (float)(1 / (4 pi)).
 *       Else a leaf adds its triangles in index order: w = w + T_t, with a' = a - q, b' = b - q, c' = c - q,
 *         det = dot(a', cross(b', c')), la = sqrtf(dot(a', a')) (likewise lb, lc),
 *         den = (((la * lb) * lc + dot(a', b') * lc) + dot(a', c') * lb) + dot(b', c') * la,
 *         T_t = 0 when det == 0, else atan_yx(det, den) * K2,  K2 = (float)(1 / (2 pi)), atan_yx the renderer's fp32 atan2
 *         (csrc/trace_common.h, oracle atan2).  (The zero rule drops the spurious +-1/2 of a degenerate triangle or of a point
 *         in a triangle's plane.)  A branch goes on to its children.
 *     beta = +INFINITY is the exact mode: no node is far (a product with +inf is +inf or NaN), every triangle is summed.  A
 *     NaN or negative beta is refused.  beta = 2 is the usual choice (SHRAY_WINDING_BETA).  For outward, counter-clockwise
 *     winding, w is about 1 inside a closed mesh and 0 outside, -1 inside an inward-wound one, 2 where two closed parts
 *     overlap; on an open mesh it varies smoothly between.
 *   - Winding-signed distance: the closest-point query (shray_closest_points's record, bit for bit) with the sign from w:
 *     -sqrtf(dist2) if w > 0.5 and dist2 > 0, else +sqrtf(dist2); NaN on a miss (w is then not computed).
 *
 * Coordinate range.  det and den are of degree 3 in the coordinates, T_far's dot(d, m) of degree 5.  Measured on meshes whose
 * largest coordinate is 1.7 scaled by S = 2^k (tests/point_scale_cases.py): in the exact mode w is
 * bit-identical to the unscaled scene's for -33 <= k <= 31.  A finite beta is not covariant (node boxes carry an absolute
 * 1e-5 pad, which moves r): its inside test w > 0.5 agrees with the exact mode's away from the surface for -31 <= k <= 20.
 * Outside, the rules above are applied as written: w = +0 for every finite point once every det underflows (k <= -57); w is
 * NaN for a finite point whenever a term is, which in the exact mode is det = inf - inf (no point up to k = 36, every point
 * from k = 44) and for a finite beta already dot(d, m) = inf - inf (the far points from k = 21, every point for
 * 28 <= k <= 34); from k = 35 up A is +inf, no node is far, and a finite beta gives the exact mode's bits.
 *
 * What is derived, and when.  The node records are derived on the device, per scene, by the first query (or download) and
 * kept with the scene; the derivation is enqueued on that call's stream.  That first call also reads the tree's topology
 * back once, synchronously (a refit never changes it).  An event recorded after each derivation orders it for everything
 * else: a later query on another stream waits for it on the device, and the download waits for it on the host.  A refit
 * (include/shader_ray_refit.h, host or device form) marks the records stale, and the next query re-derives them on its own
 * stream.  The records are one buffer per scene, rewritten in place by a re-derivation: queries of the old geometry still
 * running on another stream must be ordered before the query that re-derives.
 *
 * Errors are the signed-distance query's: count == 0 is a no-op; a negative count, a NULL pointer, a NaN or negative beta, a
 * point or record buffer that is not 16-byte aligned, or an output buffer that is not 4-byte aligned fail with
 * SHRAY_ERR_INVALID_ARGUMENT; a scene without a packed tree or with a tree deeper than SHRAY_POINT_MAX_HEIGHT is refused with
 * SHRAY_ERR_BAD_TREE before anything is launched; counts beyond one launch's grid are split over launches.
 */
#ifndef SHADER_RAY_WINDING_H
#define SHADER_RAY_WINDING_H

#include <stdint.h>

#include "shader_ray_point.h"

#ifdef __cplusplus
extern "C" {
#endif

/* floats per node of shray_scene_winding_data_download: P[3], r, N[3], A, M[9], three zeros */
enum { SHRAY_WINDING_DATA_FLOATS = 20 };

/* Barill et al.'s accuracy parameter for a second-order expansion */
#define SHRAY_WINDING_BETA 2.0f

/* Asynchronous: `count` points at d_points -> `count` winding numbers at d_out (float), on `hip_stream` (NULL: the null
 * stream).  Device memory of the scene's device. */
int shray_winding_number_device(shray_scene *scene, const shray_point *d_points, int64_t count, float beta, float *d_out,
                                void *hip_stream);

/* Blocking, host arrays. */
int shray_winding_number(shray_scene *scene, const shray_point *points, int64_t count, float beta, float *out);

/* Asynchronous: `count` winding-signed distances at d_signed (float) and, unless d_closest is NULL, `count` shray_closest
 * records at d_closest, on `hip_stream`. */
int shray_winding_signed_distance_device(shray_scene *scene, const shray_point *d_points, int64_t count, float beta,
                                         float *d_signed, shray_closest *d_closest, void *hip_stream);

/* Blocking, host arrays; `closest` may be NULL. */
int shray_winding_signed_distance(shray_scene *scene, const shray_point *points, int64_t count, float beta, float *signed_out,
                                  shray_closest *closest);

/* Blocking, for tests: SHRAY_WINDING_DATA_FLOATS floats per packed node, in pre-order, into `out` (node_count * 20 floats;
 * node_count from shray_scene_geometry_counts). */
int shray_scene_winding_data_download(shray_scene *scene, float *out);

#ifdef __cplusplus
}
#endif

#endif /* SHADER_RAY_WINDING_H */
