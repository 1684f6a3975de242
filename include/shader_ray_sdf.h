/*
 * shader_ray_sdf.h -- signed distance queries on a resident scene: caller-supplied points in, the distance to the scene's
 * surface out, negative inside, with the closest-point record it came from.
 *
 * libshray_sdf.so implements it, a client of libshray_hip.so (include/shader_ray_hip.h): a scene created there is queried
 * here, and errors are read with shray_last_error().  The sign is the angle-weighted pseudonormal test of Baerentzen and
 * Aanaes (Signed distance computation using the angle weighted pseudonormal, IEEE TVCG 11(3), 2005), DESIGN section 12.
 *
 * Semantics.  Arithmetic as in include/shader_ray_point.h: IEEE fp32, single rounding, no FMA contraction, correctly
 * rounded division and square root, dot(x, y) = (x.x*y.x + x.y*y.y) + x.z*y.z, cross(u, w) = (u.y*w.z - u.z*w.y,
 * u.z*w.x - u.x*w.z, u.x*w.y - u.y*w.x).  Corner k of the scene is positions[3k .. 3k+2]; triangle t has corners 3t, 3t+1,
 * 3t+2 = a, b, c.
 *   - The closest part is the point query.  The input is shray_point, and the shray_closest record of each point is the one
 *     shray_closest_points returns for the same scene and point, bit for bit.
 *   - Welding.  Corners i and j are the same vertex iff all three coordinates compare equal as floats (so -0 == +0).  A
 *     corner with a non-finite coordinate is a vertex of its own.  Only positions are compared: seams with split normals
 *     or colours weld.
 *   - Face normal of triangle t: n = cross(b-a, c-a), len = sqrtf(dot(n, n)), nhat = (n.x/len, n.y/len, n.z/len); nhat = 0
 *     when len is 0 or not finite (the triangle is degenerate).
 *   - Corner angle.  The two edges leaving a corner, in the triangle's order: at a, u = b-a and w = c-a; at b, u = c-b and
 *     w = a-b; at c, u = a-c and w = b-c.  alpha = atan_yx(sqrtf(dot(x, x)), dot(u, w)) with x = cross(u, w), where atan_yx
 *     is the renderer's fp32 atan2 (csrc/trace_common.h, oracle atan2); alpha = 0 when dot(u, u) or dot(w, w) is 0.
 *   - Pseudonormals, not normalised (only the sign of a dot product is used):
 *       vertex  N_v = sum of alpha_k * nhat_t(k) over the corners k welded to v, in ascending corner index, from +0; each
 *               product and each sum rounded once, per component;
 *       edge    an edge is the unordered pair of welded vertices of two corners of a triangle (its slots AB, AC, BC);
 *               N_e = sum of nhat_t over the edge's slots in ascending order of 3t + slot (AB 0, AC 1, BC 2), from +0;
 *       face    N_f = nhat_t.
 *   - Sign.  For a hit record (q, dist2, triangle t, region r): d = p - q per component, s = dot(d, N) with N the vertex
 *     pseudonormal of corner 3t+r for r = 0, 1, 2, the edge pseudonormal of slot AB, AC, BC of t for r = 3, 4, 5, nhat_t for
 *     r = 6.  The signed distance is -sqrtf(dist2) if s < 0 and dist2 > 0, else +sqrtf(dist2).  A miss gives NaN: outside
 *     a finite radius there is no sign.
 *   - Guarantee, and its limits.  With exact arithmetic, on a closed (shray_surface_info.closed), consistently oriented,
 *     non-self-intersecting mesh, the sign is negative exactly inside, for outward (counter-clockwise seen from outside)
 *     winding.  In fp32 the sign can be wrong only very near the surface, where p - q and the rounding of the
 *     pseudonormals are of one size.  Nothing more is promised; on an open or non-manifold mesh the rule above is applied
 *     as written and its sign means nothing.
 *   - Topology (shray_scene_surface_info), counted on the welded vertices.  Each triangle has three edge slots.  An edge
 *     with one slot is a boundary edge, with three or more non-manifold; an edge with two slots is misoriented when both
 *     traverse it (a -> b, b -> c, c -> a) from the same welded vertex.  closed = no boundary, non-manifold or misoriented
 *     edge.  A degenerate triangle is one whose nhat is 0.
 *
 * Coordinate range.  The closest part has the point query's range (include/shader_ray_point.h).  dot(n, n) is of degree 4
 * under sqrtf, the pseudonormals are of degree 0.  Measured on meshes whose largest coordinate is 1.7 scaled by S = 2^k
 * (tests/point_scale_cases.py): the sign data is bit-identical to the unscaled scene's for
 * -26 <= k <= 33, and the signed values are the unscaled ones times S for -26 <= k <= 32.  Outside, the rules above are
 * applied as written: as dot(n, n) underflows to 0 or overflows to +inf, triangles count as degenerate (all of them from
 * k = -36 down and from k = 37 up) and their nhat is 0; the welded topology does not depend on the scale; the value is NaN
 * exactly on a miss and its magnitude is sqrtf(dist2); its sign means nothing.
 *
 * What is derived, and when.  The pseudonormals are derived on the device, per scene, by the first signed query (or
 * surface_info / sign_data download) and kept with the scene; the derivation is enqueued on that call's stream and needs
 * no readback.  An event recorded after it orders it for everything else: a later query on another stream waits for it on
 * the device (no host synchronisation), and surface_info and the sign data download wait for it on the host.  A refit
 * (include/shader_ray_refit.h, host or device form) marks the data stale, and the next signed query re-derives it on its own
 * stream before it walks: a refit and a signed query on one stream see the refit geometry with no synchronisation.  The
 * derived data is one buffer per scene, rewritten in place by a re-derivation: queries of the old geometry still running on
 * another stream must be ordered before the query that re-derives (as every use of a scene across a refit must be).
 *
 * Errors are the point query's: count == 0 is a no-op; a negative count, a NULL pointer, a point or record buffer that is
 * not 16-byte aligned, or a signed-value buffer that is not 4-byte aligned fail with SHRAY_ERR_INVALID_ARGUMENT; a scene
 * without a packed tree or with a tree deeper than SHRAY_POINT_MAX_HEIGHT is refused with SHRAY_ERR_BAD_TREE before
 * anything is launched; counts beyond one launch's grid are split over launches (the walk and the sign alike).
 */
#ifndef SHADER_RAY_SDF_H
#define SHADER_RAY_SDF_H

#include <stdint.h>

#include "shader_ray_point.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct shray_surface_info {
    int64_t vertices;              /* welded vertices */
    int64_t edges;                 /* welded edges */
    int64_t boundary_edges;        /* edges with one slot */
    int64_t nonmanifold_edges;     /* edges with three or more slots */
    int64_t misoriented_edges;     /* edges with two slots that traverse it in the same direction */
    int64_t degenerate_triangles;  /* nhat = 0 */
    int32_t closed;                /* 1: no boundary, non-manifold or misoriented edge */
    int32_t reserved;
} shray_surface_info;

/* floats per triangle of shray_scene_sign_data_download: nhat, the pseudonormals of the vertices of corners a, b, c, and of
 * the edges AB, AC, BC, each 3 floats */
enum { SHRAY_SIGN_DATA_FLOATS = 21 };

/* Asynchronous: `count` points at d_points -> `count` signed distances at d_signed (float) and, unless d_closest is NULL,
 * `count` shray_closest records at d_closest, on `hip_stream` (NULL: the null stream).  Device memory of the scene's
 * device. */
int shray_signed_distance_device(shray_scene *scene, const shray_point *d_points, int64_t count, float *d_signed,
                                 shray_closest *d_closest, void *hip_stream);

/* Blocking, host arrays; `closest` may be NULL. */
int shray_signed_distance(shray_scene *scene, const shray_point *points, int64_t count, float *signed_out, shray_closest *closest);

/* Blocking: the scene's welded topology (derived first if it is not current). */
int shray_scene_surface_info(shray_scene *scene, shray_surface_info *info);

/* Blocking, for tests: SHRAY_SIGN_DATA_FLOATS floats per triangle into `out` (triangle_count * 21 floats). */
int shray_scene_sign_data_download(shray_scene *scene, float *out);

#ifdef __cplusplus
}
#endif

#endif /* SHADER_RAY_SDF_H */
