/*
 * shader_ray_instance_intersect.h -- instanced triangle-intersection queries: world triangles, or the triangles of one placed
 * instance, against a set of placed scenes; per query triangle, how many triangles of how many instances it intersects, and
 * the K smallest (instance, triangle) pairs in order.  Collisions over a set: an assembly's interference check, a cutting
 * sheet through a world of parts, contact detection after the instances moved.
 *
 * libshray_instance_intersect.so implements it, a client of libshray_hip.so (include/shader_ray_hip.h) and of
 * libshray_instance.so (include/shader_ray_instance.h): the scenes are created in the first, the set in the second, and
 * errors are read with shray_last_error().  It needs neither libshray_intersect.so nor libshray_instance_overlap.so nor
 * libshray_instance_point.so: their headers are read for the types and the formulas only.  DESIGN section 24.
 *
 * Contract.  It adds no new arithmetic: include/shader_ray_instance_point.h's world triangles, include/shader_ray_intersect.h's
 * per-pair test, set, order and SHRAY_INTERSECT_ANY.
 *   - Input.  shray_triangle in world space and shray_intersect_params, both unchanged from include/shader_ray_intersect.h.
 *     (A caller that does not link libshray_intersect.so fills the params itself: struct_size, K = max_triangles, flags,
 *     reserved = 0.)
 *   - Per pair (instance i, triangle t).
 *       The three corners are mapped by include/shader_ray_instance_point.h's formula.
 *       That formula uses nonzero entries only, adds left to right, in fp32, with no contraction.
 *       Then include/shader_ray_intersect.h's per-pair test runs on the three world corners and the query.  Its stages:
 *         stage 0;
 *         the shared-corner rule (SHRAY_INTERSECT_SKIP_SHARED), on world corners, three == per corner pair;
 *         translation by the query's first corner;
 *         the degenerate rule, on the world triangle;
 *         the seventeen axes in their order.
 *   - The set.  S = { (i, t) : no stage rejects }, over every triangle of every instance.  It is independent of the top
 *     level, of any tree and of the visit order.
 *   - The key.  (instance, triangle) ascending.  This is the merged scene's index order.
 *   - Per query.
 *       n = |S| as int32, when counts are asked for.
 *       K int32 at out[query * K + k]: the triangles of the min(n, K) smallest members, then -1.
 *       Unless d_instances is NULL, K int32 at instances[query * K + k]: their instances, then -1.
 *       K is a prefix of any larger K.
 *       query * K is indexed in 64 bits.
 *   - Unwalked queries are include/shader_ray_intersect.h's, judged on the world query: a non-finite coordinate or an all-zero
 *     nq gives n = 0, all -1, and no walk.
 *   - SHRAY_INTERSECT_ANY needs K = 0 and counts.  It writes 1 or 0.  A lane stops at its first member.
 *   - There is no cap of any kind.  The scenes' kernel ids are ignored.  The query is not symmetric, as
 *     include/shader_ray_intersect.h says: the translation is by the query's corner.
 *
 * The instance form.  The queries are the set's own geometry.
 *   - Query j is triangle first + j of instance q's scene.  It is read from that scene's positions on the device when the
 *     kernel runs, so after a refit on the same stream it is the moved mesh.
 *   - Its corners are mapped by instance q's current map with the same formula, so they are bit for bit that instance's world
 *     corners.
 *   - SHRAY_INTERSECT_SKIP_OWN_INSTANCE = 4 is defined here.  Only the instance form accepts it.  With it, a pair whose
 *     instance index equals q is not a member.
 *   - "Own" is the instance index, not the scene: a duplicate instance at the same place is found.
 *   - Without the flag, every non-degenerate triangle finds itself and its neighbours, as in include/shader_ray_intersect.h's
 *     self form.
 *   - The item forms, and libshray_intersect.so, refuse bit 4 as an unknown flag.
 *
 * Consequences.
 *   1. One identity instance returns shray_intersect_triangles' indices and counts, with instance 0 on every held slot, and
 *      its three counters.
 *   2. The answer equals shray_intersect_triangles on the merged scene of mapped corners in instance order.  The merged index
 *      is split into (instance, triangle).
 *   3. The indices (and instances) for K are a prefix of those for any larger K.
 *   4. A duplicate instance contributes every one of its pairs again, the lower instance first.
 *   5. SHRAY_INTERSECT_ANY's count equals n > 0.
 *   6. The instance form equals the item form fed with instance q's rows of the merged scene.  With
 *      SHRAY_INTERSECT_SKIP_OWN_INSTANCE the pairs of instance q are removed and n is less by their number.
 *   7. On one identity instance without the new flag, the instance form equals shray_intersect_self.
 *
 * The walk is exact.  An instance's walk skips a node of the member's tree only when the node's IMAGE box
 * (include/shader_ray_instance_point.h) misses the query's vertex box (min3 / max3 of its world corners) on some axis:
 * image.hi_j < lo_j or image.lo_j > hi_j, six comparisons with no margin; touching enters, and a NaN end compares false and
 * culls less.  The image box holds every fp32 world corner below the node, bit for bit, and stage 0 is the same comparison on
 * the triangle's own world corners, so such a node holds no triangle that passes stage 0.  The set's top level skips a node or
 * an instance only when its STORED box misses the query's vertex box on some axis by the same comparison, and there an axis
 * may separate only when the stored float and the query float it is compared with are not both below 2^-109 in magnitude
 * (include/shader_ray_instance_overlap.h's guard, unchanged).  The top level's root is not tested, so a set of one instance
 * culls nothing there.  Without counts (and K > 0) a query that holds K pairs skips every instance above the K-th held pair's:
 * the key leads with the instance, so the indices are the same.  Nothing else prunes.
 *
 * Coordinate range.  include/shader_ray_intersect.h's range applies to the WORLD coordinates: the mapped corners and the
 * queries.  Outside it the definition above still holds bit for bit.
 *
 * Errors, in this order: shray_intersect_params misuse (NULL, a wrong struct_size, K outside [0, SHRAY_INTERSECT_MAX], unknown
 * flag bits -- SHRAY_INTERSECT_SKIP_OWN_INSTANCE is one in the item forms --, a nonzero reserved field, then
 * SHRAY_INTERSECT_ANY with K != 0 or without counts); in the instance form a negative first, then an instance outside the set
 * (judged when the set is not NULL); a negative count; a NULL set or triangle pointer; a NULL out pointer with K > 0; K == 0
 * together with no counts (nothing is asked for; with K == 0 the out and instance pointers are neither read nor written); a
 * triangle pointer that is not 16-byte aligned, or an out, instance or count pointer that is not 4-byte aligned.  All fail with
 * SHRAY_ERR_INVALID_ARGUMENT before any device is touched.  Then, in the instance form, first + count beyond the instance's
 * triangle count fails with it before any launch; count == 0 is then a no-op.  A member scene whose tree is higher than
 * SHRAY_POINT_MAX_HEIGHT fails with SHRAY_ERR_BAD_TREE before any launch (a member without a packed tree is refused when the
 * set is created).  Counts beyond one launch (2^24 queries) are split over launches.
 *
 * The device forms are stream-ordered: after a refit of a member scene and after shray_instance_set_update_device on the same
 * stream they see the new geometry and the new set, and after a blocking shray_instance_set_update they see the new maps
 * (their upload is staged on the query's stream).  With K > 8 and d_instances NULL they take count * K int32 of scratch from
 * the stream's memory pool (hipMallocAsync) and give it back in stream order (hipFreeAsync).  They never synchronise with the
 * host, except that a member scene's first query by this library or another that walks the packed tree reads the tree's
 * height back once (they share that per-scene state; a refit never changes it).
 */
#ifndef SHADER_RAY_INSTANCE_INTERSECT_H
#define SHADER_RAY_INSTANCE_INTERSECT_H

#include <stdint.h>

#include "shader_ray_instance.h"
#include "shader_ray_intersect.h"
#include "shader_ray_point.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
    SHRAY_INTERSECT_SKIP_OWN_INSTANCE = 4   /* flags, the instance form only: a pair of the query's own instance is not a member */
};

/* Asynchronous: `count` world triangles at d_triangles (device memory of the set's device, 16-byte aligned) -> count * K
 * triangle indices at d_out (NULL iff K == 0), unless d_instances is NULL count * K instance indices there, and unless d_counts
 * is NULL `count` intersection counts there, on `hip_stream` (NULL: the null stream).  With d_counts NULL a query that holds K
 * pairs skips the instances that cannot reach them: the same indices, and less work wherever it has more than K members. */
int shray_intersect_triangles_instances_device(shray_instance_set *set, const shray_intersect_params *op,
                                               const shray_triangle *d_triangles, int64_t count, int32_t *d_out, int32_t *d_instances,
                                               int32_t *d_counts, void *hip_stream);

/* Blocking, host arrays (the same rules for indices, instances and counts). */
int shray_intersect_triangles_instances(shray_instance_set *set, const shray_intersect_params *op, const shray_triangle *triangles,
                                        int64_t count, int32_t *out, int32_t *instances, int32_t *counts);

/* Blocking, host arrays, with the work counters of the walk that does not prune by K (whatever K), summed over a query's
 * walks: node_visits (image-box tests evaluated in the members' trees; the top level is not counted), leaf_visits and
 * triangle_tests as in include/shader_ray_intersect.h; traversals counts the instance walks begun; samples = count; the other
 * fields are 0.  A set of one instance never culls at the top level, so one identity instance gives
 * shray_intersect_triangles_counters' own three counters. */
int shray_intersect_triangles_instances_counters(shray_instance_set *set, const shray_intersect_params *op,
                                                 const shray_triangle *triangles, int64_t count, int32_t *out, int32_t *instances,
                                                 int32_t *counts, shray_counters *counters);

/* Asynchronous, the instance form: the queries are the triangles [first, first + count) of instance `instance`'s scene under
 * that instance's map, query j at d_out[j * K], d_instances[j * K] and d_counts[j]; device memory of the set's device, on
 * `hip_stream`. */
int shray_intersect_instance_device(shray_instance_set *set, const shray_intersect_params *op, int32_t instance, int64_t first,
                                    int64_t count, int32_t *d_out, int32_t *d_instances, int32_t *d_counts, void *hip_stream);

/* Blocking, the instance form into host arrays. */
int shray_intersect_instance(shray_instance_set *set, const shray_intersect_params *op, int32_t instance, int64_t first, int64_t count,
                             int32_t *out, int32_t *instances, int32_t *counts);

#ifdef __cplusplus
}
#endif

#endif /* SHADER_RAY_INSTANCE_INTERSECT_H */
