/*
 * shader_ray_instance_multihit.h -- instanced all-hits ray queries: world-space rays through a set of placed scenes; per ray,
 * how many surfaces it crosses over all instances and the first K crossings in order, each with its instance.
 *
 * libshray_instance_multihit.so implements it, a client of libshray_hip.so (include/shader_ray_hip.h) and of
 * libshray_instance.so (include/shader_ray_instance.h): the scenes are created in the first, the set in the second, and
 * errors are read with shray_last_error().  DESIGN section 16.
 *
 * Contract.  Rays are shray_ray in world space, records are shray_hit, parameters are shray_multihit_params
 * (include/shader_ray_multihit.h, unchanged).  For a set of N instances and one world ray with tmax > 0 (else: no walk, zero
 * crossings):
 *   - The object ray of instance i is include/shader_ray_instance.h's: the rows of the set's W[i], nonzero entries only,
 *     left to right, fp32, no FMA contraction.  tmax is not transformed.
 *   - S_i is include/shader_ray_multihit.h's crossing set of that object ray on instance i's scene with B = tmax.
 *   - S is the union over i of {(t, u, v, triangle, i)} for the members of S_i.  t is the world ray's parameter too (an
 *     affine map keeps it), so the members of different instances compare directly.
 *   - The key is (t as a float comparison, instance index, triangle index).  Two members of S differ in instance or
 *     triangle, so this is a total order.
 *
 * Output per ray:
 *   - n = |S| as an int32 (the crossing count, which may exceed K);
 *   - K = max_hits records in ray-major order, hits[ray * K + k], and, when asked for, K instance indices
 *     instances[ray * K + k];
 *   - these hold the min(n, K) members of S with the smallest keys, in ascending key order;
 *   - the remaining slots are {tmax, 0, 0, SHRAY_HIT_MISS} with instance -1.
 *
 * There is no iteration cap, and SHRAY_HIT_CAP never appears.  max_leaf_tests applies per leaf as in the all-hits query.
 * The scenes' kernel ids (shray_scene_set_kernel) are ignored.  The top level skips an instance only when that cannot change
 * the answer: when the ray misses the instance's widened world box over [0, tmax] (no walk of it would accept a hit), and,
 * in the form without counts, when the box begins beyond the K-th smallest t held (a box that begins exactly there is
 * visited: a lower instance index wins the tie).
 *
 * S is a set and the order is total on it, so the answer does not depend on the order of the top-level walk or of any
 * instance's walk.  Consequences:
 *   - a set of one identity instance gives shray_trace_all_hits' bytes, with instance 0 on every held record;
 *   - without counts, max_hits = 1 returns for every ray exactly the first record of the max_hits = 8 answer;
 *   - record 0 and its instance are shray_trace_instances' closest hit (uncapped) whenever the two smallest keys differ in
 *     t and no closest-hit walk met a NaN candidate;
 *   - an exact duplicate of an instance contributes every crossing a second time at the same t, and the lower instance
 *     index sorts first.
 *
 * Errors: count == 0 is a no-op.  A NULL set, params or ray pointer, a NULL hit pointer with max_hits > 0, max_hits == 0
 * with a NULL count pointer (d_hits is then neither read nor written), max_hits outside [0, SHRAY_MULTIHIT_MAX],
 * max_leaf_tests outside [0, 2^24], a nonzero reserved, a wrong struct_size, a negative count, a ray or hit pointer that is
 * not 16-byte aligned or an instance or count pointer that is not 4-byte aligned fail with SHRAY_ERR_INVALID_ARGUMENT before
 * any device is touched.  A member scene whose tree is higher than SHRAY_POINT_MAX_HEIGHT fails with SHRAY_ERR_BAD_TREE
 * before any launch (a member without a packed tree is refused when the set is created).  Counts beyond one launch (2^24
 * rays) are split over launches.
 *
 * The device form is stream-ordered: after a refit of a member scene and after shray_instance_set_update_device on the same
 * stream it sees the new geometry and the new set.  It never synchronises with the host, except that a member scene's first
 * query by this library, the all-hits library or the closest-point library reads the tree's height back once (they share
 * that per-scene state; a refit never changes it).  With max_hits > 8 and d_instances NULL it takes count * K int32 of
 * stream-ordered scratch (hipMallocAsync / hipFreeAsync on hip_stream) for the instance half of the keys.
 */
#ifndef SHADER_RAY_INSTANCE_MULTIHIT_H
#define SHADER_RAY_INSTANCE_MULTIHIT_H

#include <stdint.h>

#include "shader_ray_instance.h"
#include "shader_ray_multihit.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Asynchronous: `count` world rays at d_rays (device memory of the set's device) -> count * K hits at d_hits (NULL iff
 * K == 0), unless d_instances is NULL count * K instance indices there, and unless d_counts is NULL `count` crossing counts
 * there, on `hip_stream` (NULL: the null stream).  With d_counts NULL the walks skip what cannot reach the first K: the same
 * records, and less work wherever rays cross more than K surfaces. */
int shray_trace_instances_all_hits_device(shray_instance_set *set, const shray_multihit_params *mp, const shray_ray *d_rays,
                                          int64_t count, shray_hit *d_hits, int32_t *d_instances, int32_t *d_counts,
                                          void *hip_stream);

/* Blocking, host arrays (the same rules for hits, instances and counts). */
int shray_trace_instances_all_hits(shray_instance_set *set, const shray_multihit_params *mp, const shray_ray *rays, int64_t count,
                                   shray_hit *hits, int32_t *instances, int32_t *counts);

/* Blocking, host arrays, with the work counters of the form that skips nothing, summed over a ray's walks: node_visits,
 * leaf_visits, triangle_tests; traversals counts walks; bad_hits = 0; samples = count; shaded_hits and env_lookups are 0.  A
 * set of one instance never culls, so its counters are shray_trace_all_hits_counters' own. */
int shray_trace_instances_all_hits_counters(shray_instance_set *set, const shray_multihit_params *mp, const shray_ray *rays,
                                            int64_t count, shray_hit *hits, int32_t *instances, int32_t *counts,
                                            shray_counters *out);

#ifdef __cplusplus
}
#endif

#endif /* SHADER_RAY_INSTANCE_MULTIHIT_H */
