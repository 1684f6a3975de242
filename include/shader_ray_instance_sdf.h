/*
 * shader_ray_instance_sdf.h -- instanced signed distance queries: world-space points against a set of placed scenes; per
 * point, the distance to the nearest instance's surface, negative inside that instance, with the closest-point record and
 * the instance it came from.
 *
 * libshray_instance_sdf.so implements it, a client of libshray_hip.so (include/shader_ray_hip.h), of libshray_instance.so
 * (include/shader_ray_instance.h), and, through their C entry points only, of libshray_instance_point.so
 * (include/shader_ray_instance_point.h) and libshray_sdf.so (include/shader_ray_sdf.h).  Errors are read with
 * shray_last_error().  DESIGN section 26.
 *
 * Contract.  A general affine map keeps neither distances nor angles.  So the magnitude is measured in world space, and the
 * sign is decided in object space.  Being inside a closed surface is invariant under an invertible affine map, mirrors
 * included.  The angle-weighted pseudonormals are valid for the object-space nearest feature, where the scene already has
 * them.
 *
 * Input is shray_point {p, max_dist2} in world space.  Per point:
 *   1. Closest part.  (record, instance i) is exactly what shray_closest_points_instances_device returns for the same set
 *      and point, byte for byte: world q, world dist2, member triangle, u, v, region, and instance -1 on a miss.
 *   2. Object point.  p_o[r] is row r of the set's current W (the matrix shray_instance_set_world_to_object returns) applied
 *      to p by the object ray's rule of include/shader_ray_instance.h:
 *        - products of nonzero entries only, added left to right;
 *        - then + W[r][3] if that is nonzero;
 *        - fp32, no contraction.
 *   3. Object sign.  sigma is the value shray_signed_distance gives on instance i's member scene for the point
 *      {p_o, +inf}.  That is the brute-force closest record in object space, then dot(p_o - q_o, N) with that scene's sign
 *      data, all as include/shader_ray_sdf.h defines it.
 *   4. Result.
 *        - -sqrtf(dist2) when sigma < 0 and dist2 > 0;
 *        - +sqrtf(dist2) otherwise.  This includes sigma NaN, which happens when p_o overflowed to a non-finite coordinate;
 *        - NaN on a miss.
 *
 * Consequences.
 *   - A set of one identity instance returns shray_signed_distance's bytes: W is the identity, so p_o has p's bits.
 *   - The sign is that of the NEAREST instance.  For pairwise disjoint closed instances that is the sign of their union: a
 *     point inside A and outside B is nearer to A's surface than to B's.  Where instances overlap it is the nearest one's
 *     sign and nothing more.
 *   - With exact arithmetic, on a closed, consistently oriented member, the sign is negative exactly inside for every
 *     invertible map: non-uniform scale, shear and mirror included.  In fp32 it can be wrong only very near the surface.
 *     That is include/shader_ray_sdf.h's caveat, plus the rounding of W and p_o.
 *   - The answer depends on neither the top level, nor any tree, nor the visit order.
 *
 * Out of scope: instanced winding numbers, gradients, and an "inside any instance" union test for overlapping sets.
 *
 * How it runs.  Stage 1 is shray_closest_points_instances_device on the same stream, into the caller's record and instance
 * buffers or into stream-ordered scratch.  Stage 2 is one lane per point: the lanes of a wave that hold one instance walk
 * that member's packed tree in object space (the closest-point walk of include/shader_ray_point.h), seeded with the dist2 of
 * the world record's own triangle at p_o, which gives the +inf walk's record bit for bit, and then sign
 * their value.  A member scene's sign data is derived, and re-derived after a refit, as include/shader_ray_sdf.h says, on
 * the query's stream.
 *
 * Counters (the counting form) are those of the sign walks only: node_visits, leaf_visits and triangle_tests as
 * include/shader_ray_point.h counts them (the seed's one evaluation is not a test of the walk and is not counted);
 * traversals = the sign walks begun, one per hit; samples = count; the other fields are 0.
 *
 * Errors are the instanced closest-point query's: count == 0 is a no-op.  A negative count, a NULL set, point or signed-value
 * pointer, a point or record pointer that is not 16-byte aligned, or a signed-value or instance pointer that is not 4-byte
 * aligned fail with SHRAY_ERR_INVALID_ARGUMENT before any device is touched.  A member scene whose tree is higher than
 * SHRAY_POINT_MAX_HEIGHT fails with SHRAY_ERR_BAD_TREE before any launch.  Counts beyond one launch (2^24 points) are split
 * over launches.
 *
 * The device form is stream-ordered like the instanced closest-point query's: after a refit of a member scene and after
 * shray_instance_set_update_device on the same stream it sees the new geometry, the new sign data and the new set.  It never
 * synchronises with the host, apart from the one readback of a member tree's height on that scene's first walking query.
 */
#ifndef SHADER_RAY_INSTANCE_SDF_H
#define SHADER_RAY_INSTANCE_SDF_H

#include <stdint.h>

#include "shader_ray_instance_point.h"
#include "shader_ray_sdf.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Asynchronous: `count` world points at d_points (device memory of the set's device, 16-byte aligned) -> `count` signed
 * distances at d_signed (float) and, unless they are NULL, `count` shray_closest records at d_closest and `count` instance
 * indices at d_instances, on `hip_stream` (NULL: the null stream). */
int shray_signed_distance_instances_device(shray_instance_set *set, const shray_point *d_points, int64_t count, float *d_signed,
                                           shray_closest *d_closest, int32_t *d_instances, void *hip_stream);

/* Blocking, host arrays.  `closest` and `instances` may be NULL. */
int shray_signed_distance_instances(shray_instance_set *set, const shray_point *points, int64_t count, float *signed_out,
                                    shray_closest *closest, int32_t *instances);

/* Blocking, host arrays, with the counters of the sign walks (above).  `signed_out`, `closest` and `instances` may be
 * NULL. */
int shray_signed_distance_instances_counters(shray_instance_set *set, const shray_point *points, int64_t count, float *signed_out,
                                             shray_closest *closest, int32_t *instances, shray_counters *counters);

#ifdef __cplusplus
}
#endif

#endif /* SHADER_RAY_INSTANCE_SDF_H */
