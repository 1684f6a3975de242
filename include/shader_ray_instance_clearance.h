/*
 * shader_ray_instance_clearance.h -- instanced triangle-distance queries: world triangles, or the triangles of one placed
 * instance, against a set of placed scenes; per query triangle, how many triangles of how many instances lie within a squared
 * distance of it, and the K nearest of them in order with the instances they belong to, each with its squared distance and a
 * witness point on either triangle.  Clearance over a set: how far apart the placed parts of an assembly are, which triangles
 * of which instances come within a tolerance of a tool, and where.
 *
 * libshray_instance_clearance.so implements it, a client of libshray_hip.so (include/shader_ray_hip.h) and of
 * libshray_instance.so (include/shader_ray_instance.h): the scenes are created in the first, the set in the second, and
 * errors are read with shray_last_error().  It needs neither libshray_clearance.so nor libshray_instance_point.so nor
 * libshray_instance_intersect.so: their headers are read for the types and the formulas only.  DESIGN section 30.
 *
 * Contract.  It adds no new arithmetic: include/shader_ray_instance_point.h's world triangles, include/shader_ray_clearance.h's
 * per-pair record, member set, order and SHRAY_CLEARANCE_ANY.
 *   - Input.  shray_triangle in world space and shray_clearance_params, both unchanged from include/shader_ray_clearance.h.
 *     (A caller that does not link libshray_clearance.so fills the params itself: struct_size, K = max_pairs, flags,
 *     max_dist2.)
 *   - Per pair (instance i, triangle t).
 *       The three corners are mapped by include/shader_ray_instance_point.h's formula.
 *       That formula uses the caller's own object_to_world floats, nonzero entries only, added left to right, in fp32, with no
 *       contraction.
 *       Then include/shader_ray_clearance.h's per-pair definition runs on the three world corners and the world query:
 *         SHRAY_CLEARANCE_SKIP_SHARED first, by float == on world corners, three per corner pair;
 *         the fifteen features in their order, against a running minimum;
 *         the intersecting stage last, with its degenerate rule judged on the world triangles.  It sets dist2 = +0 and
 *         feature = 15 and leaves the witnesses as the feature minimum's.
 *   - The set.  S = { (i, t) : dist2 <= max_dist2 }, over every triangle of every instance.  It is independent of the top
 *     level, of any tree and of the visit order.
 *   - The key.  (dist2 by float <, instance, triangle), a total order on S.
 *   - Per query.
 *       n = |S| as int32, when counts are asked for.
 *       K 48-byte shray_pair_distance records at out[query * K + k]: the min(n, K) smallest members in key order, then
 *       include/shader_ray_clearance.h's miss records { 0, 0, 0, dist2 = max_dist2 as given, 0, 0, 0, -1, -1, 0, 0, 0 }.
 *       Unless d_instances is NULL, K int32 at instances[query * K + k]: the member's instance, -1 behind a miss.
 *       triangle is the member scene's own triangle index.
 *       The witnesses and dist2 are in world space.
 *       reserved stays 0.
 *       The records for K are a prefix of those for any larger K.
 *       query * K is indexed in 64 bits.
 *   - Unwalked queries are include/shader_ray_clearance.h's, judged on the world query: a non-finite coordinate, or a NaN or
 *     negative max_dist2, gives n = 0, all miss records (instances -1), and no walk.
 *   - SHRAY_CLEARANCE_ANY is include/shader_ray_clearance.h's: it needs K = 0 and counts, writes 1 or 0, and a lane stops at its
 *     first member.
 *   - max_dist2 = +inf means every pair.
 *   - There is no cap of any kind.  The scenes' kernel ids are ignored.  The query is not symmetric, as
 *     include/shader_ray_clearance.h says.
 *
 * The instance form.  The queries are the set's own geometry.
 *   - Query j is triangle first + j of instance q's scene.  It is read from that scene's positions on the device when the
 *     kernel runs.
 *   - Its corners are mapped by instance q's current map with the same formula, so they are bit for bit that instance's world
 *     corners.
 *   - So after a refit of that scene and shray_instance_set_update_device on the same stream the queries are the moved part.
 *   - SHRAY_CLEARANCE_SKIP_OWN_INSTANCE = 4 is defined here.  Only the instance form accepts it.  With it, a pair whose
 *     instance index equals q is not a member.
 *   - "Own" is the instance index, not the scene: a duplicate instance at the same place is found at distance 0.
 *   - Without the flag, every triangle finds itself and its neighbours at distance 0, as in include/shader_ray_clearance.h's
 *     self form.
 *   - The item forms, and libshray_clearance.so, refuse bit 4 as an unknown flag.
 *
 * Consequences.
 *   1. One identity instance returns shray_clearance_triangles' bytes and counts, with instance 0 on every held slot, and its
 *      three counters.
 *   2. The answer equals shray_clearance_triangles on the merged scene of mapped corners in instance order.  The merged index
 *      is split into (instance, triangle).
 *   3. The records (and instances) for K are a prefix of those for any larger K.
 *   4. An exact duplicate instance contributes every one of its pairs again at the same dist2, the lower instance first.
 *   5. SHRAY_CLEARANCE_ANY's count equals n > 0.
 *   6. The instance form equals the item form fed with instance q's rows of the merged scene.  With
 *      SHRAY_CLEARANCE_SKIP_OWN_INSTANCE the pairs of instance q are removed and n is less by their number.
 *   7. On one identity instance without the new flag, the instance form equals shray_clearance_self.
 *
 * The walk is exact, with no margin.  An instance's walk skips a node of the member's tree only when
 * lb > reach, where lb = dot(g, g) and per axis g = qlo > hi ? qlo - hi : (lo > qhi ? lo - qhi : 0), [qlo, qhi] being the
 * query's vertex box (min3 / max3 of its world corners) and [lo, hi] the node's IMAGE box (include/shader_ray_instance_point.h);
 * reach is max_dist2, or in the form that writes no counts the K-th smallest dist2 held, which starts at max_dist2.  A node with
 * lb == reach is entered (a lower instance or triangle wins a tie).  The image box holds every fp32 world corner below the
 * node, bit for bit, so include/shader_ray_clearance.h's argument carries over with "the node's box" read as "the image box":
 * every witness x is clamped into the query's vertex box and every witness y into the world triangle's vertex box, which lies
 * inside the image box; rounding, squaring and the sum are monotone; an intersecting pair passed the vertex-box stage, so
 * lb = 0.  The same bound on a world triangle's own vertex box skips a pair before its arithmetic.  The set's top level skips a
 * node or an instance only when the same bound on its STORED box is above the reach, and the root is not tested, so a set of
 * one instance culls nothing there.  A stored box holds every fp32 world corner below it unless all of its coordinates and the
 * corner's are below 2^-109 in magnitude; there the bound's term on an axis either squares to 0 (a query end below 2^-75) or
 * equals the query end, which the witness on that side is not below.  So lb <= dist2 for every pair below any node, stored or
 * image, and the counting form skips no member.
 *
 * Coordinate range.  include/shader_ray_clearance.h's range applies to the WORLD coordinates: the mapped corners and the
 * queries.  Outside it the definition above still holds bit for bit.
 *
 * Errors, in this order: shray_clearance_params misuse (NULL, a wrong struct_size, K outside [0, SHRAY_CLEARANCE_MAX], unknown
 * flag bits -- SHRAY_CLEARANCE_SKIP_OWN_INSTANCE is one in the item forms --, then SHRAY_CLEARANCE_ANY with K != 0 or without
 * counts); in the instance form a negative first, then an instance outside the set (judged when the set is not NULL); a
 * negative count; a NULL set or triangle pointer; a NULL out pointer with K > 0; K == 0 together with no counts (nothing is
 * asked for; with K == 0 the out and instance pointers are neither read nor written); a triangle or record pointer that is not
 * 16-byte aligned, or an instance or count pointer that is not 4-byte aligned.  All fail with SHRAY_ERR_INVALID_ARGUMENT before
 * any device is touched.  Then, in the instance form, first + count beyond the instance's triangle count fails with it before
 * any launch; count == 0 is then a no-op.  A member scene whose tree is higher than SHRAY_POINT_MAX_HEIGHT fails with
 * SHRAY_ERR_BAD_TREE before any launch (a member without a packed tree is refused when the set is created).  Counts beyond one
 * launch (2^24 queries) are split over launches.
 *
 * The device forms are stream-ordered: after a refit of a member scene and after shray_instance_set_update_device on the same
 * stream they see the new geometry and the new set, and after a blocking shray_instance_set_update they see the new maps
 * (their upload is staged on the query's stream).  With K > 8 and d_instances NULL they take count * K int32 of scratch from
 * the stream's memory pool (hipMallocAsync) and give it back in stream order (hipFreeAsync).  They never synchronise with the
 * host, except that a member scene's first query by this library or another that walks the packed tree reads the tree's
 * height back once (they share that per-scene state; a refit never changes it).
 */
#ifndef SHADER_RAY_INSTANCE_CLEARANCE_H
#define SHADER_RAY_INSTANCE_CLEARANCE_H

#include <stdint.h>

#include "shader_ray_clearance.h"
#include "shader_ray_instance.h"
#include "shader_ray_point.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
    SHRAY_CLEARANCE_SKIP_OWN_INSTANCE = 4   /* flags, the instance form only: a pair of the query's own instance is not a member */
};

/* Asynchronous: `count` world triangles at d_triangles (device memory of the set's device, 16-byte aligned) -> count * K
 * records at d_out (NULL iff K == 0), unless d_instances is NULL count * K instance indices there, and unless d_counts is NULL
 * `count` member counts there, on `hip_stream` (NULL: the null stream).  With d_counts NULL the walk skips what cannot reach
 * the nearest K: the same records, and less work wherever more than K pairs lie within max_dist2. */
int shray_clearance_triangles_instances_device(shray_instance_set *set, const shray_clearance_params *op,
                                               const shray_triangle *d_triangles, int64_t count, shray_pair_distance *d_out,
                                               int32_t *d_instances, int32_t *d_counts, void *hip_stream);

/* Blocking, host arrays (the same rules for records, instances and counts). */
int shray_clearance_triangles_instances(shray_instance_set *set, const shray_clearance_params *op, const shray_triangle *triangles,
                                        int64_t count, shray_pair_distance *out, int32_t *instances, int32_t *counts);

/* Blocking, host arrays, with the work counters of the walk that prunes only by max_dist2 (whatever K), summed over a query's
 * walks: node_visits (image-box bounds evaluated in the members' trees; the top level is not counted), leaf_visits and
 * triangle_tests as in include/shader_ray_clearance.h; traversals counts the instance walks begun; samples = count; the other
 * fields are 0.  A set of one instance never culls at the top level, so one identity instance gives
 * shray_clearance_triangles_counters' own three counters. */
int shray_clearance_triangles_instances_counters(shray_instance_set *set, const shray_clearance_params *op,
                                                 const shray_triangle *triangles, int64_t count, shray_pair_distance *out,
                                                 int32_t *instances, int32_t *counts, shray_counters *counters);

/* Asynchronous, the instance form: the queries are the triangles [first, first + count) of instance `instance`'s scene under
 * that instance's map, query j at d_out[j * K], d_instances[j * K] and d_counts[j]; device memory of the set's device, on
 * `hip_stream`. */
int shray_clearance_instance_device(shray_instance_set *set, const shray_clearance_params *op, int32_t instance, int64_t first,
                                    int64_t count, shray_pair_distance *d_out, int32_t *d_instances, int32_t *d_counts, void *hip_stream);

/* Blocking, the instance form into host arrays. */
int shray_clearance_instance(shray_instance_set *set, const shray_clearance_params *op, int32_t instance, int64_t first, int64_t count,
                             shray_pair_distance *out, int32_t *instances, int32_t *counts);

#ifdef __cplusplus
}
#endif

#endif /* SHADER_RAY_INSTANCE_CLEARANCE_H */
