/*
 * shader_ray_instance_winding.h -- instanced winding numbers: world-space points against a set of placed scenes; per point,
 * how many times the placed surfaces wind around it, summed over every instance of the set, the lowest instance that
 * contains it, and a signed distance whose sign is that of the union.
 *
 * libshray_instance_winding.so implements it, a client of libshray_hip.so (include/shader_ray_hip.h), of libshray_instance.so
 * (include/shader_ray_instance.h), and, through their C entry points only, of libshray_instance_point.so
 * (include/shader_ray_instance_point.h) and libshray_winding.so (include/shader_ray_winding.h).  Errors are read with
 * shray_last_error().  DESIGN section 28.
 *
 * Contract.  Arithmetic is that of include/shader_ray_point.h: fp32, no contraction.  Input is shray_point {p, max_dist2} in
 * world space, plus `beta` as in include/shader_ray_winding.h.
 *   - Orientation.  For instance i, with W the set's current world-to-object matrix (the floats
 *     shray_instance_set_world_to_object returns), evaluate in double with no contraction:
 *       det = W00*(W11*W22 - W12*W21) - W01*(W10*W22 - W12*W20) + W02*(W10*W21 - W11*W20).
 *     The products of two floats are exact in double.  The rest is left to right as written.  s_i = -1 when det < 0, else +1.
 *     It is taken from W because W is the matrix that maps the point.
 *   - Object point.  p_o is W applied to p by the object ray's rule of include/shader_ray_instance.h, as in
 *     include/shader_ray_instance_sdf.h step 2.
 *   - Term.  w_i is the value shray_winding_number gives on instance i's member scene for {p_o} and beta, bit for bit.  That
 *     includes NaN when p_o has a non-finite coordinate.  t_i = -w_i when s_i < 0, else w_i.
 *   - Sum.  w = +0; for i ascending over every instance of the set, w = w + t_i.  A world point with a non-finite coordinate
 *     gives NaN with no walk.  There is no top-level cull: every instance contributes.  A distant one contributes its root's
 *     far-field term when beta is finite.
 *   - Containing instance (optional output): the lowest i with t_i > 0.5, or -1 when none.  A NaN term is not above 0.5.
 *   - Winding-signed distance.  The record and the instance are shray_closest_points_instances_device's bytes.  The value is
 *     -sqrtf(dist2) when w > 0.5 and dist2 > 0, else +sqrtf(dist2).  A miss gives NaN, and w is then not computed.  The sign
 *     is the union's.  It is also negative where closed outward-wound instances overlap.
 * A NaN is any NaN: its sign and payload are not part of the contract.
 *
 * Consequences.
 *   - A set of one identity instance returns shray_winding_number's bytes.
 *   - For closed members, w is the world winding number of the placed meshes under every invertible map, up to rounding:
 *     the winding number of a closed surface is a degree, and w_world(p) = sign(det W) * w_object(W p).  A mirror reverses the
 *     winding of what it places: the mirror image of an outward-wound member is an inward-wound world mesh and counts -1
 *     inside, as shray_winding_number would say of that world mesh; a member meant to be placed by mirrors and to count +1
 *     is wound inward in its own frame.
 *   - For open members, w equals the world value under similarity maps: rotation, uniform scale, translation and their
 *     mirrors.
 *   - For open members under non-uniform scale or shear, w is the member's own-frame value: a solid angle is not kept by such
 *     a map.  The inside test w > 0.5 is then made in the asset's own shape.  DESIGN section 28 has the measured differences
 *     from the world value (up to 0.07 on an open cube).
 *   - A finite beta's far test d2 > (beta * r)^2 is made in object space.  Under a map of condition kappa the world-space
 *     ratio can be as low as beta / kappa.  Accuracy under the test maps is measured, not promised.
 *   - The answer depends on no top level, no visit order across instances and no tree but each member's own.
 *
 * Out of scope: a top-level far field over groups of instances, a world-frame value for open members under non-conformal
 * maps, gradients, and point clouds.
 *
 * How it runs.  One lane per point in one-wave workgroups; the loop over the instances is wave-uniform, every lane visits
 * every instance in order, maps its point and runs include/shader_ray_winding.h's walk on the member's tree and node
 * records.  The orientations are computed on the device on the query's stream by every query.  A member scene's node records
 * are derived, and re-derived after a refit, as include/shader_ray_winding.h says, on the query's stream.  The winding-signed
 * distance runs shray_closest_points_instances_device first, on the same stream, into the caller's buffers or into
 * stream-ordered scratch of at most 2^22 records at a time, and walks only for hits.
 *
 * Errors.  count == 0 is a no-op.  A negative count, a NULL set, point or value pointer, a NaN or negative beta, a point or
 * record pointer that is not 16-byte aligned, or a value, instance or containing pointer that is not 4-byte aligned fail with
 * SHRAY_ERR_INVALID_ARGUMENT before any device is touched.  A member scene whose tree is higher than SHRAY_POINT_MAX_HEIGHT
 * fails with SHRAY_ERR_BAD_TREE before any launch.  Counts beyond one launch (2^24 points) are split over launches.
 *
 * The device forms are stream-ordered like the instanced closest-point query's: after a refit of a member scene and after
 * shray_instance_set_update_device on the same stream they see the new geometry, the new node records, the new W and its
 * orientation.  They never synchronise with the host, apart from the one readback of a member tree's topology on that
 * scene's first use.
 */
#ifndef SHADER_RAY_INSTANCE_WINDING_H
#define SHADER_RAY_INSTANCE_WINDING_H

#include <stdint.h>

#include "shader_ray_instance_point.h"
#include "shader_ray_winding.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Asynchronous: `count` world points at d_points (device memory of the set's device, 16-byte aligned) -> `count` winding
 * numbers at d_out (float) and, unless it is NULL, `count` containing instances at d_containing (int32), on `hip_stream`
 * (NULL: the null stream). */
int shray_winding_number_instances_device(shray_instance_set *set, const shray_point *d_points, int64_t count, float beta,
                                          float *d_out, int32_t *d_containing, void *hip_stream);

/* Blocking, host arrays.  `containing` may be NULL. */
int shray_winding_number_instances(shray_instance_set *set, const shray_point *points, int64_t count, float beta, float *out,
                                   int32_t *containing);

/* Asynchronous: `count` winding-signed distances at d_signed (float) and, unless they are NULL, `count` shray_closest records
 * at d_closest and `count` instance indices at d_instances, on `hip_stream`. */
int shray_winding_signed_distance_instances_device(shray_instance_set *set, const shray_point *d_points, int64_t count, float beta,
                                                   float *d_signed, shray_closest *d_closest, int32_t *d_instances,
                                                   void *hip_stream);

/* Blocking, host arrays.  `closest` and `instances` may be NULL. */
int shray_winding_signed_distance_instances(shray_instance_set *set, const shray_point *points, int64_t count, float beta,
                                            float *signed_out, shray_closest *closest, int32_t *instances);

/* Blocking, for tests: the orientation s_i of every instance, +1.0f or -1.0f, `count` floats into `out`, computed on the
 * device by the kernel the queries run. */
int shray_instance_set_orientations(shray_instance_set *set, float *out);

#ifdef __cplusplus
}
#endif

#endif /* SHADER_RAY_INSTANCE_WINDING_H */
