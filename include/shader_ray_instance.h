/*
 * shader_ray_instance.h -- instanced ray queries: rays traced through many placed copies of resident scenes at once.
 *
 * libshray_instance.so implements it, a client of libshray_hip.so (include/shader_ray_hip.h): the scenes are created there,
 * and errors are read with shray_last_error().  An instance is a resident scene plus an object-to-world transform; a set of
 * instances has a small top-level BVH over their world boxes, and a query walks it and runs the ray query's own per-scene walk
 * (include/shader_ray_query.h) for every instance a ray reaches.  Rays, hits and query parameters are the ray query's.
 *
 * Semantics:
 *   Transforms
 *   - object_to_world is a row-major 3 x 4 affine map: world = A * object + b, A = columns 0..2, b = column 3.  The library
 *     inverts it in double and rounds the result to float.  That float matrix is W (world to object), and
 *     shray_instance_set_world_to_object returns it.  A transform with any non-finite entry, a singular linear part, or a
 *     non-finite W is refused.
 *   - The object ray: for row r, the products W[r][c] * v[c] are added left to right, but only for entries where
 *     W[r][c] != 0; for the origin, W[r][3] is then added if it is nonzero.  In fp32, with no FMA contraction.  Skipping zero
 *     entries means an identity, a translation, an axis permutation or an axis flip leaves the signed zeros of a direction
 *     unchanged (the walk's octant choice and its +-0 slab quotients depend on them).  tmax is not transformed.
 *   Hits
 *   - t, u, v and triangle are the object-space walk's values; t is the world ray's parameter too (an affine map keeps it).
 *   - The result is the hit with the smallest t over all instances; on equal t the lowest instance index wins, whatever the
 *     order of the top-level walk.  (A walk of instance i starts its running closest hit from the best t so far, or from
 *     nextafterf(best t, +inf) when i is lower than the best hit's instance, clamped to 1e8 as the ray query clamps tmax.
 *     Because an accepted hit always lies below 1e8, that clamp never changes a tie; the one consequence it could have, a tie
 *     at exactly 1e8 going to the instance found first, cannot arise.)
 *   - A miss, or a ray with tmax <= 0 or NaN: triangle = SHRAY_HIT_MISS, t = tmax, u = v = 0, instance -1.
 *   Walks
 *   - Every instance walk is the packed stack traversal in its convergent form (the ray query's kernel id 0); the scene's
 *     kernel id (shray_scene_set_kernel) is ignored.  A scene without a packed tree is refused when the set is created.
 *   - A walk that ends in the iteration cap ends the ray: triangle = SHRAY_HIT_CAP, t = -1, instance -1.  The cap applies per
 *     walk, so which rays reach it depends on the walk order (a walk started from a lower bound visits fewer nodes).
 *   - any_hit: the ray ends at the first walk that reports a hit; the instance and (t, u, v, triangle) are that walk's own
 *     result.  (any == MISS) == (closest == MISS) on every ray.
 *   - The top-level cull is conservative: an instance whose walk would report a hit is never skipped.  (A walk that would
 *     only reach the cap may be skipped when the ray misses the instance's widened world box.)
 *   Counters
 *   - Summed over a ray's walks: traversals counts walks, bad_hits capped rays.  A set of one instance never culls, so its
 *     counters are the ray query's.
 *   Updates and lifetime
 *   - shray_instance_set_update re-reads every member scene's root box and its device view (a refit changes both) and rebuilds
 *     the top level; callers must call it after refitting any member scene (include/shader_ray_refit.h), and a query traced
 *     between the refit and the update may miss the moved geometry.  Create and update wait for the set's device
 *     (hipDeviceSynchronize) before they read the root boxes, so a refit enqueued before the call, on any stream, is complete
 *     by then; a refit another thread enqueues during the call is not ordered with it.  A failed update leaves the set as
 *     it was.
 *   - shray_instance_set_update_device is the same update, enqueued on a HIP stream: it builds, on the set's device, the set
 *     shray_instance_set_update would build from the same transforms and member scenes, bit for bit (top-level nodes, W
 *     records, scene views), so every later query's hits, instances and counters are the host update's too.  (The one
 *     exception is the sign of a zero box coordinate in a node over a world box of zero extent at the origin, which the host's
 *     fold leaves to its order.)  Member root
 *     boxes are read on the device, ordered after earlier work on its stream (a refit enqueued there before it), and member
 *     views are re-read on the host without waiting.  It neither waits for the device nor copies anything back to the host.
 *     A query enqueued later on the same stream sees the new set; work on other streams that reads the set, and updates of
 *     one set made on different streams, are ordered by the caller, as with a refit.  d_object_to_world is read when the
 *     update runs, so it stays alive and unchanged until then.
 *   - A device update validates every transform on the device by the host's rules.  If any is refused, the update writes
 *     nothing: the set keeps its previous transforms and arrays, as after a failed host update, and
 *     shray_instance_set_update_status reports the lowest refused instance.  A NULL set, or a d_object_to_world that is not
 *     4-byte aligned or not device memory of the set's device holding count * 12 floats, fails at the call with
 *     SHRAY_ERR_INVALID_ARGUMENT and enqueues nothing (update_status still reports the update before it).
 *   - The set's transforms are those of the last applied update, host or device.  shray_instance_set_update(set, NULL) and
 *     shray_instance_set_world_to_object wait for a device update and read its result back; a host update after a device
 *     update is the host update alone.
 *   - The set holds the scene handles, not copies: destroying a member scene while a set uses it is the caller's error.
 *     All member scenes live on one device.
 *
 * Errors: count == 0 is a no-op.  A negative count, a NULL pointer, a device pointer that is not 16-byte aligned (an instance
 * array: 4-byte aligned), a wrong struct_size, or a set of 0 or more than 2^20 instances fail with SHRAY_ERR_INVALID_ARGUMENT;
 * a scene without a packed tree with SHRAY_ERR_BAD_TREE; creating a set with no HIP device visible with SHRAY_ERR_NO_DEVICE.
 * Counts beyond one launch's grid are split over launches.
 */
#ifndef SHADER_RAY_INSTANCE_H
#define SHADER_RAY_INSTANCE_H

#include <stdint.h>

#include "shader_ray_hip.h"
#include "shader_ray_query.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct shray_instance_set shray_instance_set;

typedef struct shray_instance {
    shray_scene *scene;          /* resident, with a packed tree; every instance's scene on one device */
    float object_to_world[12];   /* row-major 3 x 4 affine map */
} shray_instance;

enum { SHRAY_INSTANCE_MAX = 1 << 20 };

/* A set of `count` instances (the array is copied; the scenes are not). */
int shray_instance_set_create(const shray_instance *instances, int32_t count, shray_instance_set **out);

/* New transforms (count * 12 floats, instance order), or NULL to keep them; re-reads the member scenes either way. */
int shray_instance_set_update(shray_instance_set *set, const float *object_to_world);

/* Asynchronous, on hip_stream (NULL: the null stream): the set's new object-to-world maps, count * 12 floats (row-major 3 x 4,
 * instance order) in device memory of the set's device, or NULL to keep the current ones; every member scene's root box is
 * re-read on the device, ordered after earlier work on hip_stream.  A refused update changes nothing (see update_status). */
int shray_instance_set_update_device(shray_instance_set *set, const float *d_object_to_world, void *hip_stream);

/* Blocks until the most recent update_device has finished.  *refused = -1 if it was applied (or none was made), otherwise the
 * lowest instance index whose transform was refused; that update changed nothing. */
int shray_instance_set_update_status(shray_instance_set *set, int32_t *refused);

void shray_instance_set_destroy(shray_instance_set *set);

int shray_instance_set_count(const shray_instance_set *set, int32_t *count);

/* W of every instance: count * 12 floats, row-major 3 x 4 */
int shray_instance_set_world_to_object(const shray_instance_set *set, float *out);

/* Asynchronous: `count` world-space rays at d_rays -> `count` hits at d_hits and, unless d_instances is NULL, the hit's
 * instance at d_instances, on `hip_stream` (NULL: the null stream).  Device memory of the set's device. */
int shray_trace_instances_device(shray_instance_set *set, const shray_query_params *qp, const shray_ray *d_rays, int64_t count,
                                 shray_hit *d_hits, int32_t *d_instances, void *hip_stream);

/* Blocking, host arrays; `instances` may be NULL. */
int shray_trace_instances(shray_instance_set *set, const shray_query_params *qp, const shray_ray *rays, int64_t count,
                          shray_hit *hits, int32_t *instances);

/* Blocking, host arrays, with the walks' counters summed as above (closest-hit walks: any_hit is ignored here, as in
 * shray_trace_rays_counters); samples = count.  `hits` and `instances` may be NULL. */
int shray_trace_instances_counters(shray_instance_set *set, const shray_query_params *qp, const shray_ray *rays, int64_t count,
                                   shray_hit *hits, int32_t *instances, shray_counters *out);

#ifdef __cplusplus
}
#endif

#endif /* SHADER_RAY_INSTANCE_H */
