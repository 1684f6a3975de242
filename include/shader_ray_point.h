/*
 * shader_ray_point.h -- closest-point queries on a resident scene: caller-supplied points in, the nearest point of the
 * scene's surface out, one record per point.
 *
 * libshray_point.so implements it, a client of libshray_hip.so (include/shader_ray_hip.h): a scene created there is
 * queried here, and errors are read with shray_last_error().  The walk uses the scene's packed tree.
 *
 * Semantics.  The answer is defined by a brute-force formula over EVERY triangle of the scene; it does not depend on the
 * tree or the visit order, so it is bit-exact and independently checkable.  All arithmetic is IEEE fp32: single rounding,
 * no FMA contraction, correctly rounded division, left-to-right sums.  dot(x, y) = (x.x*y.x + x.y*y.y) + x.z*y.z.
 * Comparisons with a NaN are false.  min(x, y) = x < y ? x : y and max(x, y) = x > y ? x : y, applied left to right.
 *   - Input: shray_point { p[3], max_dist2 }, 16 bytes, in scene (object) space, the space of the scene's vertex_positions.
 *   - Output: shray_closest { q[3], dist2, u, v, triangle, region }, 32 bytes.
 *   - Per triangle i, with corners a, b, c = positions[9i .. 9i+8] (the triangle index of shray_hit): the closest-point
 *     algorithm of Ericson, Real-Time Collision Detection section 5.1.5, in exactly its order of tests.
 *       ab = b-a, ac = c-a, ap = p-a, bp = p-b, cp = p-c; d1 = dot(ab,ap), d2 = dot(ac,ap), d3 = dot(ab,bp),
 *       d4 = dot(ac,bp), d5 = dot(ab,cp), d6 = dot(ac,cp), vc = d1*d4 - d3*d2, vb = d5*d2 - d1*d6, va = d3*d6 - d5*d4.
 *       The regions are tested in this order: vertex A (region 0), vertex B (1), edge AB (3), vertex C (2), edge AC (4),
 *       edge BC (5), face (6):
 *         A:  d1 <= 0 && d2 <= 0                                   (u, v) = (0, 0),   q = a
 *         B:  d3 >= 0 && d4 <= d3                                  (1, 0),            q = b
 *         AB: vc <= 0 && d1 >= 0 && d3 <= 0     s = d1/(d1-d3)     (s, 0),            q = a + ab*s
 *         C:  d6 >= 0 && d5 <= d6                                  (0, 1),            q = c
 *         AC: vb <= 0 && d2 >= 0 && d6 <= 0     s = d2/(d2-d6)     (0, s),            q = a + ac*s
 *         BC: va <= 0 && (d4-d3) >= 0 && (d5-d6) >= 0
 *                                               s = (d4-d3)/((d4-d3)+(d5-d6))   (1-s, s),   q = b + (c-b)*s
 *         face: den = 1/((va+vb)+vc), u = vb*den, v = vc*den,                    q = (a + ab*u) + ac*v
 *       A quotient s that is not finite is replaced by 0.  In the face region, if u or v is not finite, both become 0.
 *       Then q is clamped per axis to the triangle's vertex box: q.x = min(max(q.x, min(min(a.x,b.x),c.x)),
 *       max(max(a.x,b.x),c.x)), likewise y and z.  Finally dist2 = dot(p-q, p-q).
 *   - Result: among the triangles with dist2 <= max_dist2, the one with the smallest dist2; on a tie the lowest triangle
 *     index.  The record is that triangle's q, dist2, u, v, triangle, region.
 *   - Miss: no triangle qualifies, or p has a non-finite coordinate, or max_dist2 is NaN or negative.  The record is
 *     triangle = SHRAY_HIT_MISS, region = -1, q = p, dist2 = max_dist2 as given, u = v = 0.  max_dist2 = +inf: no limit.
 *   - Every triangle of a leaf is tested (the renderer's max_leaf_tests cap does not apply) and there is no iteration cap.
 *   - The walk is exact, not approximate: a node is skipped only when its box bound exceeds the best dist2 so far, and that
 *     bound is never above the dist2 of a triangle below it, in fp32, bit for bit.
 *   - A scene without a packed tree is refused with SHRAY_ERR_BAD_TREE; so is a tree deeper than SHRAY_POINT_MAX_HEIGHT
 *     (the walk's stack lives in LDS), before anything is launched.  The scene's kernel id is ignored.
 *   - The first query of a scene reads the tree's topology back once, synchronously, to size the stack; the height is then
 *     kept with the scene (a refit does not change it).
 *
 * Coordinate range.  va, vb and vc are of degree 4 in the coordinates, so they leave fp32's normal range long before the
 * positions do.  Measured with the brute-force definition on meshes whose largest coordinate is 1.7, with positions, points
 * and radii scaled by S = 2^k (tests/point_scale_cases.py): every record is the exact image of the
 * unscaled one (q * S, dist2 * S^2, the same u, v, triangle and region, bit for bit) for -25 <= k <= 32.  Outside that range
 * the definition above still holds bit for bit, subnormals, infinities and NaNs included (no flush to zero, no approximate
 * division), and so do its invariants: triangle is in range or SHRAY_HIT_MISS, region in -1 .. 6, q lies in the reported
 * triangle's vertex box, dist2 = dot(p-q, p-q) recomputed and never NaN (a NaN q is replaced by the clamp's selects), the
 * lowest index wins a tie (when every dist2 underflows to 0 or overflows to +inf that is triangle 0, and the walk skips
 * nothing: 0 > 0 and inf > inf are false).  But the record no longer names the geometrically nearest triangle: a third to a
 * half of the points get another one.
 *
 * Errors: count == 0 is a no-op.  A negative count, a NULL pointer or a device pointer that is not 16-byte aligned fail
 * with SHRAY_ERR_INVALID_ARGUMENT.  Counts beyond one launch's grid are split over launches.  A query enqueued on a stream
 * after a refit on that stream sees the refit geometry.
 */
#ifndef SHADER_RAY_POINT_H
#define SHADER_RAY_POINT_H

#include <stdint.h>

#include "shader_ray_query.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct shray_point {
    float p[3];
    float max_dist2;   /* squared search radius; +inf: no limit */
} shray_point;

typedef struct shray_closest {
    float q[3];        /* the nearest surface point (p on a miss) */
    float dist2;       /* dot(p-q, p-q) (max_dist2 on a miss) */
    float u, v;        /* weights of corners b and c: q ~ a + (b-a)*u + (c-a)*v before the clamp */
    int32_t triangle;  /* >= 0: the scene's triangle index; SHRAY_HIT_MISS */
    int32_t region;    /* 0, 1, 2: vertex A, B, C; 3, 4, 5: edge AB, AC, BC; 6: face; -1 on a miss */
} shray_closest;

enum {
    SHRAY_REGION_A = 0, SHRAY_REGION_B = 1, SHRAY_REGION_C = 2, SHRAY_REGION_AB = 3, SHRAY_REGION_AC = 4, SHRAY_REGION_BC = 5,
    SHRAY_REGION_FACE = 6, SHRAY_REGION_NONE = -1
};

/* the deepest tree (edges from the root to its deepest leaf) the walk's LDS stack holds */
enum { SHRAY_POINT_MAX_HEIGHT = 128 };

/* Asynchronous: `count` points at d_points -> `count` records at d_out, on `hip_stream` (NULL: the null stream).  Device
 * memory of the scene's device, 16-byte aligned. */
int shray_closest_points_device(shray_scene *scene, const shray_point *d_points, int64_t count, shray_closest *d_out,
                                void *hip_stream);

/* Blocking, host arrays. */
int shray_closest_points(shray_scene *scene, const shray_point *points, int64_t count, shray_closest *out);

/* Blocking, host arrays, with the walk's work counters: node_visits (box bounds evaluated), leaf_visits, triangle_tests;
 * samples = count; the other fields are 0.  `out` may be NULL. */
int shray_closest_points_counters(shray_scene *scene, const shray_point *points, int64_t count, shray_closest *out,
                                  shray_counters *counters);

#ifdef __cplusplus
}
#endif

#endif /* SHADER_RAY_POINT_H */
