/*
 * shader_ray_instance_overlap.h -- instanced box-overlap queries: axis-aligned world boxes against a set of placed scenes;
 * per box, how many triangles of how many instances touch it, and the K smallest (instance, triangle) pairs in order.
 *
 * libshray_instance_overlap.so implements it, a client of libshray_hip.so (include/shader_ray_hip.h) and of
 * libshray_instance.so (include/shader_ray_instance.h): the scenes are created in the first, the set in the second, and
 * errors are read with shray_last_error().  It needs neither libshray_overlap.so nor libshray_instance_point.so: their
 * headers are read for the types and the formulas only.  DESIGN section 23.
 *
 * Contract.  It adds no new arithmetic: include/shader_ray_instance_point.h's world triangles, include/shader_ray_overlap.h's
 * 13-axis test, set, order and SHRAY_OVERLAP_ANY.
 *   - Input.  shray_box in world space and shray_overlap_params, both unchanged from include/shader_ray_overlap.h.  (A caller
 *     that does not link libshray_overlap.so fills the params itself: struct_size, K = max_triangles, flags, reserved = 0.)
 *   - Per pair (instance i, triangle t).
 *       The three corners are mapped by include/shader_ray_instance_point.h's formula.
 *       That formula uses nonzero entries only, adds left to right, in fp32, with no contraction.
 *       Then include/shader_ray_overlap.h's 13-axis test runs on the three world corners and the box.
 *   - The set.  S = { (i, t) : no axis separates }, over every triangle of every instance.  It is independent of the top
 *     level, of any tree and of the visit order.
 *   - The key.  (instance, triangle) ascending.  This is the merged scene's index order.
 *   - Per box.
 *       n = |S| as int32, when counts are asked for.
 *       K int32 at out[box * K + k]: the triangles of the min(n, K) smallest members, then -1.
 *       Unless d_instances is NULL, K int32 at instances[box * K + k]: their instances, then -1.
 *       K is a prefix of any larger K.
 *       box * K is indexed in 64 bits.
 *   - Unwalked boxes are as in include/shader_ray_overlap.h: a non-finite coordinate, or lo > hi, gives n = 0, all -1, no walk.
 *   - SHRAY_OVERLAP_ANY needs K = 0 and counts.  It writes 1 or 0.  A lane stops at its first touching pair.
 *   - There is no cap of any kind.  The scenes' kernel ids are ignored.
 *
 * Consequences.
 *   1. One identity instance returns shray_overlap_triangles' indices and counts.  Instance 0 is on every held slot.
 *   2. The answer equals shray_overlap_triangles on the merged scene of mapped corners in instance order.  The merged index is
 *      split into (instance, triangle).
 *   3. The indices (and instances) for K are a prefix of those for any larger K.
 *   4. A duplicate instance contributes every one of its pairs again, the lower instance first.
 *   5. SHRAY_OVERLAP_ANY's count equals n > 0.
 *
 * The walk is exact.  An instance's walk skips a node of the member's tree only when the node's IMAGE box
 * (include/shader_ray_instance_point.h) misses the query box on some axis: image.hi_j < lo_j or image.lo_j > hi_j, six
 * comparisons with no margin; touching enters, and a NaN end compares false and culls less.  The image box holds every fp32
 * world corner below the node, bit for bit, so such a node holds no triangle that passes stage 0.  The set's top level skips
 * a node or an instance only when its STORED box misses the query box on some axis by the same comparison, and there an axis
 * may separate only when the stored float and the query float it is compared with are not both below 2^-109 in magnitude:
 * the stored box holds an instance's fp32 world corners wherever the world coordinates are normal or 0, and a corner that a
 * subnormal rounding put outside it, the stored end it passed and a query end between the two are all below that threshold.
 * The top level's root is not tested, so a set of one instance culls nothing there.  Without counts (and K > 0) a box that
 * holds K pairs skips every instance above the K-th held pair's: the key leads with the instance, so the indices are the same.
 *
 * Coordinate range.  include/shader_ray_overlap.h's range applies to the WORLD coordinates: the mapped corners and the boxes.
 * Outside it the definition above still holds bit for bit.
 *
 * Errors, in this order: shray_overlap_params misuse (NULL, a wrong struct_size, K outside [0, SHRAY_OVERLAP_MAX], unknown
 * flag bits, a nonzero reserved field, then SHRAY_OVERLAP_ANY with K != 0 or without counts); a negative count; a NULL set or
 * box pointer; a NULL out pointer with K > 0; K == 0 together with no counts (nothing is asked for; with K == 0 the out and
 * instance pointers are neither read nor written); a box pointer that is not 16-byte aligned, or an out, instance or count
 * pointer that is not 4-byte aligned.  All fail with SHRAY_ERR_INVALID_ARGUMENT before any device is touched; count == 0 is
 * then a no-op.  A member scene whose tree is higher than SHRAY_POINT_MAX_HEIGHT fails with SHRAY_ERR_BAD_TREE before any
 * launch (a member without a packed tree is refused when the set is created).  Counts beyond one launch (2^24 boxes) are
 * split over launches.
 *
 * The device form is stream-ordered: after a refit of a member scene and after shray_instance_set_update_device on the same
 * stream it sees the new geometry and the new set, and after a blocking shray_instance_set_update it sees the new maps (their
 * upload is staged on the query's stream).  With K > 8 and d_instances NULL it takes count * K int32 of scratch from the
 * stream's memory pool (hipMallocAsync) and gives it back in stream order (hipFreeAsync).  It never synchronises with the
 * host, except that a member scene's first query by this library or another that walks the packed tree reads the tree's
 * height back once (they share that per-scene state; a refit never changes it).
 */
#ifndef SHADER_RAY_INSTANCE_OVERLAP_H
#define SHADER_RAY_INSTANCE_OVERLAP_H

#include <stdint.h>

#include "shader_ray_instance.h"
#include "shader_ray_overlap.h"
#include "shader_ray_point.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Asynchronous: `count` world boxes at d_boxes (device memory of the set's device, 16-byte aligned) -> count * K triangle
 * indices at d_out (NULL iff K == 0), unless d_instances is NULL count * K instance indices there, and unless d_counts is NULL
 * `count` overlap counts there, on `hip_stream` (NULL: the null stream).  With d_counts NULL a box that holds K pairs skips
 * the instances that cannot reach them: the same indices, and less work wherever more than K pairs touch the box. */
int shray_overlap_triangles_instances_device(shray_instance_set *set, const shray_overlap_params *op, const shray_box *d_boxes,
                                             int64_t count, int32_t *d_out, int32_t *d_instances, int32_t *d_counts,
                                             void *hip_stream);

/* Blocking, host arrays (the same rules for indices, instances and counts). */
int shray_overlap_triangles_instances(shray_instance_set *set, const shray_overlap_params *op, const shray_box *boxes, int64_t count,
                                      int32_t *out, int32_t *instances, int32_t *counts);

/* Blocking, host arrays, with the work counters of the walk that does not prune by K (whatever K), summed over a box's
 * walks: node_visits (image-box tests evaluated in the members' trees; the top level is not counted), leaf_visits and
 * triangle_tests as in include/shader_ray_overlap.h; traversals counts the instance walks begun; samples = count; the other
 * fields are 0.  A set of one instance never culls at the top level, so one identity instance gives
 * shray_overlap_triangles_counters' own three counters. */
int shray_overlap_triangles_instances_counters(shray_instance_set *set, const shray_overlap_params *op, const shray_box *boxes,
                                               int64_t count, int32_t *out, int32_t *instances, int32_t *counts,
                                               shray_counters *counters);

#ifdef __cplusplus
}
#endif

#endif /* SHADER_RAY_INSTANCE_OVERLAP_H */
