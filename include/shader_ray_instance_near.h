/*
 * shader_ray_instance_near.h -- instanced within-radius queries: world-space points against a set of placed scenes; per
 * point, how many triangles of how many instances lie within its radius, and the nearest K of them in order with the
 * instances they belong to.
 *
 * libshray_instance_near.so implements it, a client of libshray_hip.so (include/shader_ray_hip.h) and of
 * libshray_instance.so (include/shader_ray_instance.h): the scenes are created in the first, the set in the second, and
 * errors are read with shray_last_error().  DESIGN section 22.
 *
 * Contract.  It adds no new arithmetic: include/shader_ray_instance_point.h's world triangles, include/shader_ray_near.h's
 * near set and order.
 *   - Input: shray_point { p[3], max_dist2 } in world space.
 *   - Params: shray_near_params (include/shader_ray_near.h), unchanged: K = max_near lies in [0, SHRAY_NEAR_MAX], and
 *     shray_near_params_init (libshray_near.so) sets K = 8.
 *   - Per pair (instance i, triangle t).  The three corners of triangle t of instance i's scene are mapped by
 *     include/shader_ray_instance_point.h's formula: the caller's own object_to_world floats M = [A | b], the very floats the
 *     set was created or last updated with; world[r] = the products M[r][c] * v[c] of the nonzero entries only, added left to
 *     right, then + M[r][3] if that is nonzero; fp32, single rounding, no FMA contraction.  Then include/shader_ray_point.h's
 *     per-triangle record { q, dist2, u, v, triangle, region } is computed on the three world corners and p.
 *   - Near set: S = { (i, t) : dist2 <= max_dist2 }, over every triangle of every instance.  S is independent of the top
 *     level, of any tree and of the visit order.
 *   - Key: (dist2 by float comparison, instance, triangle), a total order on S.
 *   - Outputs per point:
 *       n = |S| as an int32, when counts are asked for;
 *       K records at out[point * K + k]: the min(n, K) smallest members of S in ascending key order, then
 *       include/shader_ray_near.h's miss records { q = p, dist2 = max_dist2 as given, 0, 0, SHRAY_HIT_MISS, -1 };
 *       unless d_instances is NULL, K int32 at instances[point * K + k]: the member's instance, -1 behind a miss.
 *     q and dist2 are in world space; triangle is the member scene's own triangle index.
 *   - A point with a non-finite p, or with a NaN or negative max_dist2, has n = 0, all miss records (instances -1), and
 *     nothing is walked.
 *   - max_dist2 = +inf means every pair, including one whose dist2 overflowed to +inf.
 *   - There is no cap of any kind: every triangle of a visited leaf is tested.  The scenes' kernel ids are ignored.
 *
 * Consequences.
 *   1. A set of one identity instance returns shray_near_triangles' bytes and counts, with instance 0 on every held record.
 *   2. K = 1 without counts is shray_closest_points_instances' record and instance for every point, misses included.
 *   3. The records (and instances) for K are a prefix of those for any larger K.
 *   4. The answer equals shray_near_triangles on the merged scene whose positions are the mapped corners in instance order,
 *      with the merged triangle index split into (instance, triangle).
 *   5. An exact duplicate of an instance contributes every pair a second time at the same dist2, and the lower instance
 *      sorts first.
 *
 * The walk is exact (DESIGN sections 20 and 22).  The set's top level skips a node or an instance only when the box bound of
 * its stored box is above the point's reach, and an instance's walk skips a node of the member's tree only when the bound of
 * the node's image box (include/shader_ray_instance_point.h) is.  The reach is max_dist2 with counts (or K = 0, or the
 * counters); without counts it is the K-th smallest dist2 held, which starts at max_dist2.  A node or instance whose bound
 * equals the reach is entered (a lower instance or triangle wins a tie); the top level's root is not tested.  An image box
 * holds every fp32 world corner below its node, and a stored top-level box every pair below it, so a pair in S has
 * bound <= dist2 <= max_dist2: the counting form skips nothing in S.  No margin is involved.
 *
 * Coordinate range.  include/shader_ray_point.h's range applies to the WORLD coordinates: the mapped corners, the points
 * and the radii.  Outside it the definition above still holds bit for bit.
 *
 * Errors, in this order: shray_near_params misuse (NULL, a wrong struct_size, K outside [0, SHRAY_NEAR_MAX], a nonzero
 * reserved field); a negative count; a NULL set or point pointer; a NULL record pointer with K > 0; K == 0 together with no
 * counts (nothing is asked for; with K == 0 the record and instance pointers are neither read nor written); a point or
 * record pointer that is not 16-byte aligned, or an instance or count pointer that is not 4-byte aligned.  All fail with
 * SHRAY_ERR_INVALID_ARGUMENT before any device is touched; count == 0 is then a no-op.  A member scene whose tree is higher
 * than SHRAY_POINT_MAX_HEIGHT fails with SHRAY_ERR_BAD_TREE before any launch (a member without a packed tree is refused
 * when the set is created).  Counts beyond one launch (2^24 points) are split over launches; point * K is indexed in 64 bits.
 *
 * The device form is stream-ordered: after a refit of a member scene and after shray_instance_set_update_device on the same
 * stream it sees the new geometry and the new set, and after a blocking shray_instance_set_update it sees the new maps (their
 * upload is staged on the query's stream).  With K > 8 and d_instances NULL it takes count * K int32 of scratch from the
 * stream's memory pool and gives it back in stream order.  It never synchronises with the host, except that a member scene's
 * first query by this library or another that walks the packed tree reads the tree's height back once (they share that
 * per-scene state; a refit never changes it).
 */
#ifndef SHADER_RAY_INSTANCE_NEAR_H
#define SHADER_RAY_INSTANCE_NEAR_H

#include <stdint.h>

#include "shader_ray_instance.h"
#include "shader_ray_near.h"
#include "shader_ray_point.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Asynchronous: `count` world points at d_points (device memory of the set's device, 16-byte aligned) -> count * K records
 * at d_out (NULL iff K == 0), unless d_instances is NULL count * K instance indices there, and unless d_counts is NULL
 * `count` near counts there, on `hip_stream` (NULL: the null stream).  With d_counts NULL the walk skips what cannot reach
 * the nearest K: the same records, and less work wherever more than K pairs lie within the radius. */
int shray_near_triangles_instances_device(shray_instance_set *set, const shray_near_params *np, const shray_point *d_points,
                                          int64_t count, shray_closest *d_out, int32_t *d_instances, int32_t *d_counts,
                                          void *hip_stream);

/* Blocking, host arrays (the same rules for records, instances and counts). */
int shray_near_triangles_instances(shray_instance_set *set, const shray_near_params *np, const shray_point *points, int64_t count,
                                   shray_closest *out, int32_t *instances, int32_t *counts);

/* Blocking, host arrays, with the work counters of the walk that prunes only by max_dist2 (whatever K), summed over a
 * point's walks: node_visits (image-box bounds evaluated in the members' trees; the top level is not counted), leaf_visits,
 * triangle_tests; traversals counts the instance walks begun; samples = count; the other fields are 0.  A set of one
 * instance never culls at the top level, so one identity instance gives shray_near_triangles_counters' own three counters. */
int shray_near_triangles_instances_counters(shray_instance_set *set, const shray_near_params *np, const shray_point *points,
                                            int64_t count, shray_closest *out, int32_t *instances, int32_t *counts,
                                            shray_counters *counters);

#ifdef __cplusplus
}
#endif

#endif /* SHADER_RAY_INSTANCE_NEAR_H */
