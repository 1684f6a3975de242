/*
 * shader_ray_near.h -- within-radius queries on a resident scene: caller-supplied points in; per point, how many triangles
 * lie within its radius and the nearest K of them in order.
 *
 * libshray_near.so implements it, a client of libshray_hip.so (include/shader_ray_hip.h): a scene created there is queried
 * here, and errors are read with shray_last_error().  DESIGN section 15.
 *
 * Contract.  It adds no new arithmetic.
 *   - Input: shray_point { p[3], max_dist2 } (include/shader_ray_point.h), unchanged.
 *   - Params: shray_near_params { struct_size, max_near, reserved[2] }, 16 bytes.  max_near = K lies in
 *     [0, SHRAY_NEAR_MAX = 64]; shray_near_params_init sets K = 8.
 *   - Per triangle i: the closest-point query's record { q, dist2, u, v, triangle, region } of shader_ray_point.h, by the
 *     same arithmetic: Ericson's order of tests, the finite-or-zero rules, the clamp to the vertex box, and
 *     dist2 = dot(p-q, p-q).
 *   - The near set is S = { i : dist2_i <= max_dist2 }.  It is defined over every triangle of the scene and is independent
 *     of the tree.
 *   - Outputs, two per point:
 *       n = |S|, as an int32;
 *       K records at out[point * K + k]: the min(n, K) members of S with the smallest keys, in ascending order, then miss
 *       records { q = p, dist2 = max_dist2 as given, 0, 0, SHRAY_HIT_MISS, -1 }.
 *     The key is (dist2 by float comparison, triangle index).  Because dist2 is a sum of squares, it is never NaN and never
 *     -0 for a finite p.
 *   - A point with a non-finite p, or with a NaN or negative max_dist2, has n = 0.  All its records are miss records and
 *     nothing is walked.  This is the closest-point query's rule.
 *   - max_dist2 = +inf means every triangle, including one whose dist2 overflowed to +inf.
 *   - There is no leaf-test cap and no iteration cap.
 *
 * Because S is a set and the key is a total order on it, the answer does not depend on the visit order.  Consequences:
 *   - K = 1 without counts is shray_closest_points' record in all 32 bytes, for every point, misses included;
 *   - the records for K are a prefix of the records for any larger K.
 *
 * The walk is exact (DESIGN sections 11 and 15): a node's box bound is never above the dist2 of a triangle below it, in fp32,
 * bit for bit.  With counts (or K = 0, or the counters) a node is skipped iff its bound is above max_dist2; without counts iff
 * it is above the K-th smallest dist2 held, which starts at max_dist2 (a node whose bound equals it is visited: a lower
 * triangle index wins a tie).  Every triangle of a visited leaf is tested.
 *
 * Coordinate range.  As the closest-point query's (include/shader_ray_point.h), over every pair within the radius: measured
 * on meshes whose largest coordinate is 1.7 scaled by S = 2^k (tests/point_scale_cases.py), the counts
 * and all K = 64 records are the exact images of the unscaled ones for -24 <= k <= 28.  Outside, the contract above holds bit
 * for bit with that header's invariants per record, the records sorted by (dist2, index) and n the number of triangles with
 * dist2 <= max_dist2; where every dist2 underflows to 0 or overflows to +inf the order is the index order.
 *
 * Errors: count == 0 is a no-op.  A wrong struct_size, K outside [0, SHRAY_NEAR_MAX], a nonzero reserved field, a negative
 * count, a NULL scene, params or point pointer, a NULL record pointer with K > 0, K == 0 together with no counts (nothing is
 * asked for; with K == 0 the record pointer is neither read nor written), a point or record pointer that is not 16-byte
 * aligned or a count pointer that is not 4-byte aligned fail with SHRAY_ERR_INVALID_ARGUMENT before any device is touched.
 * A scene without a packed tree, or one with a tree higher than SHRAY_POINT_MAX_HEIGHT, fails with SHRAY_ERR_BAD_TREE before
 * any launch.  Counts beyond one launch (2^24 points) are split over launches; point * K is indexed in 64 bits.  The device
 * form is stream-ordered (after a refit on the same stream it sees the new geometry) and never synchronises with the host,
 * except that a scene's first query by this library, the closest-point library or the all-hits library reads the tree's
 * height back once (they share that per-scene state; a refit never changes it).
 */
#ifndef SHADER_RAY_NEAR_H
#define SHADER_RAY_NEAR_H

#include <stdint.h>

#include "shader_ray_point.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { SHRAY_NEAR_MAX = 64 };

typedef struct shray_near_params {
    uint32_t struct_size;   /* sizeof(shray_near_params) */
    int32_t max_near;       /* K: 0 (counts only) .. SHRAY_NEAR_MAX */
    int32_t reserved[2];    /* 0 */
} shray_near_params;

/* max_near = 8, struct_size set */
void shray_near_params_init(shray_near_params *np);

/* Asynchronous: `count` points at d_points (device memory of the scene's device) -> count * K records at d_out (NULL iff
 * K == 0) and, unless d_counts is NULL, `count` near counts at d_counts, on `hip_stream` (NULL: the null stream).  With
 * d_counts NULL the walk skips what cannot reach the nearest K: the same records, and less work wherever more than K
 * triangles lie within the radius. */
int shray_near_triangles_device(shray_scene *scene, const shray_near_params *np, const shray_point *d_points, int64_t count,
                                shray_closest *d_out, int32_t *d_counts, void *hip_stream);

/* Blocking, host arrays (the same rules for records and counts). */
int shray_near_triangles(shray_scene *scene, const shray_near_params *np, const shray_point *points, int64_t count,
                         shray_closest *out, int32_t *counts);

/* Blocking, host arrays, with the work counters of the walk that prunes only by max_dist2 (whatever K): node_visits (box
 * bounds evaluated), leaf_visits, triangle_tests; samples = count; the other fields are 0. */
int shray_near_triangles_counters(shray_scene *scene, const shray_near_params *np, const shray_point *points, int64_t count,
                                  shray_closest *out, int32_t *counts, shray_counters *counters);

#ifdef __cplusplus
}
#endif

#endif /* SHADER_RAY_NEAR_H */
