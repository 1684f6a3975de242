/*
 * shader_ray_instance_point.h -- instanced closest-point queries: world-space points against a set of placed scenes; per
 * point, the nearest point of any instance's surface, and which instance it lies on.
 *
 * libshray_instance_point.so implements it, a client of libshray_hip.so (include/shader_ray_hip.h) and of
 * libshray_instance.so (include/shader_ray_instance.h): the scenes are created in the first, the set in the second, and
 * errors are read with shray_last_error().  DESIGN section 20.
 *
 * Contract.  A general affine map does not keep distances, so distance is measured in WORLD space, on each instance's
 * triangles mapped to the world in fp32 by a fixed formula; the answer is then defined by brute force over every triangle
 * of every instance, bit for bit, as include/shader_ray_point.h defines its own.
 *   - Input: shray_point { p[3], max_dist2 } in world space.
 *   - Output: one shray_closest record per point, plus one int32 instance index per point when d_instances is not NULL.
 *   - Instance i's world triangles.  Every corner v of instance i's scene (positions[9t .. 9t+8]) is mapped by the caller's
 *     object_to_world floats M = [A | b]: the very floats the set was created or last updated with, not an inverse.
 *     world[r] = the products M[r][c] * v[c] of the nonzero entries only, added left to right, then + M[r][3] if that is
 *     nonzero.  A row with nothing to add gives 0.  The arithmetic is fp32 with single rounding and no FMA contraction.  This
 *     is the rule of include/shader_ray_instance.h's object ray applied to the forward map.  An identity, translation-free
 *     permutation or flip therefore keeps every coordinate's bits, signed zeros included.
 *   - Per pair (instance, triangle): include/shader_ray_point.h's per-triangle formula, unchanged, on the three world corners
 *     and p: Ericson's order of tests, the replaced non-finite quotients, the clamp to the (world) vertex box, and
 *     dist2 = dot(p-q, p-q).
 *   - Result: among all pairs with dist2 <= max_dist2, the smallest dist2; on a tie the lowest instance, then the lowest
 *     triangle.  The record's q and dist2 are in world space; triangle is the member scene's own triangle index; u, v and
 *     region are as in include/shader_ray_point.h.
 *   - Miss: the record is as in include/shader_ray_point.h (triangle = SHRAY_HIT_MISS, region = -1, q = p,
 *     dist2 = max_dist2 as given, u = v = 0), with instance -1.  The conditions are the same too: p has a non-finite
 *     coordinate, max_dist2 is NaN or negative, or nothing is within reach.
 *   - Every triangle of a leaf is tested and there is no iteration cap.  The scenes' kernel ids are ignored.
 *   - The walk is exact, not approximate.  The set's top level skips a node only when the box bound of its stored box is
 *     above the point's best dist2 so far, and an instance's walk skips a node of the member's tree only when the bound of
 *     the node's IMAGE box is: on world axis r the low end is the corner formula's row r on lo[c] where M[r][c] > 0 and hi[c]
 *     where M[r][c] < 0, the high end the opposite choice.  The formula is monotone in each coordinate, so the image box holds
 *     every fp32 world corner below the node and its bound is never above the dist2 of a triangle below it, in fp32, bit for
 *     bit.  No margin is involved.
 *
 * Consequences.
 *   - A set of one identity instance returns shray_closest_points' bytes, with instance 0 on every hit.
 *   - An exact duplicate of an instance never wins a tie against the lower index.
 *   - The answer depends on neither the top level, nor any tree, nor the visit order.
 *   - The answer equals shray_closest_points on a merged scene whose positions are the mapped corners in instance order.
 *
 * Coordinate range.  include/shader_ray_point.h's range applies to the WORLD coordinates: the mapped
 * corners, the points and the radii.  Outside it the definition above still holds bit for bit.
 *
 * Errors: count == 0 is a no-op.  A negative count, a NULL set, point or record pointer, a point or record pointer that is
 * not 16-byte aligned or an instance pointer that is not 4-byte aligned fail with SHRAY_ERR_INVALID_ARGUMENT before any
 * device is touched.  A member scene whose tree is higher than SHRAY_POINT_MAX_HEIGHT fails with SHRAY_ERR_BAD_TREE before
 * any launch (a member without a packed tree is refused when the set is created).  Counts beyond one launch (2^24 points)
 * are split over launches.
 *
 * The device form is stream-ordered: after a refit of a member scene and after shray_instance_set_update_device on the same
 * stream it sees the new geometry and the new set, and after a blocking shray_instance_set_update it sees the new maps (their
 * upload is staged on the query's stream).  It never synchronises with the host, except that a member scene's first query by
 * this library or another that walks the packed tree reads the tree's height back once (they share that per-scene state; a
 * refit never changes it).
 */
#ifndef SHADER_RAY_INSTANCE_POINT_H
#define SHADER_RAY_INSTANCE_POINT_H

#include <stdint.h>

#include "shader_ray_instance.h"
#include "shader_ray_point.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Asynchronous: `count` world points at d_points (device memory of the set's device, 16-byte aligned) -> `count` records at
 * d_out and, unless d_instances is NULL, `count` instance indices there, on `hip_stream` (NULL: the null stream). */
int shray_closest_points_instances_device(shray_instance_set *set, const shray_point *d_points, int64_t count,
                                          shray_closest *d_out, int32_t *d_instances, void *hip_stream);

/* Blocking, host arrays.  `instances` may be NULL. */
int shray_closest_points_instances(shray_instance_set *set, const shray_point *points, int64_t count, shray_closest *out,
                                   int32_t *instances);

/* Blocking, host arrays, with the work counters summed over a point's walks: node_visits (image-box bounds evaluated in the
 * members' trees; the top level is not counted), leaf_visits, triangle_tests; traversals counts the instance walks begun;
 * samples = count; the other fields are 0.  `out` and `instances` may be NULL.  A set of one instance never culls at the top
 * level, so the counters of one identity instance are shray_closest_points_counters' own. */
int shray_closest_points_instances_counters(shray_instance_set *set, const shray_point *points, int64_t count, shray_closest *out,
                                            int32_t *instances, shray_counters *counters);

#ifdef __cplusplus
}
#endif

#endif /* SHADER_RAY_INSTANCE_POINT_H */
