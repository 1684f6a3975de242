/*
 * shader_ray_instance_pairs.h -- the instance-pair collision matrix of a set of placed scenes: for every ordered pair of
 * instances (a, b), how many triangle pairs (a triangle of a, a triangle of b) intersect, and the smallest such pair.  Which
 * parts of an assembly collide, with which other part, and where: one launch for the whole set.
 *
 * libshray_instance_pairs.so implements it, a client of libshray_hip.so (include/shader_ray_hip.h) and of
 * libshray_instance.so (include/shader_ray_instance.h): the scenes are created in the first, the set in the second, and
 * errors are read with shray_last_error().  It needs neither libshray_intersect.so nor libshray_instance_intersect.so nor
 * libshray_instance_point.so: their headers are read for the formulas only.  DESIGN section 31.
 *
 * Contract.  It adds no new arithmetic: include/shader_ray_instance_point.h's world triangles and
 * include/shader_ray_instance_intersect.h's per-pair test.
 *   - Pair.  For a set of n instances, a pair is (a, ta, b, tb).
 *       The query is triangle ta of instance a's scene, mapped by instance a's current map with
 *       include/shader_ray_instance_point.h's formula.  It is read from that scene's positions on the device when the kernel
 *       runs, so after a refit on the same stream it is the moved mesh.
 *       The scene triangle is triangle tb of instance b's scene, mapped the same way by instance b's map.
 *   - Membership.  M(a, ta, b, tb) is include/shader_ray_instance_intersect.h's per-pair test on those world corners, the
 *     query first: its unwalked-query rule (a query with a non-finite world coordinate or an all-zero nq has no members) and
 *     SHRAY_PAIRS_SKIP_SHARED judged on world corners, three == per corner pair.
 *       A pair with b == a is never a member.  "Own" is the instance index, not the scene: a duplicate instance at the same
 *       place is found.
 *       With SHRAY_PAIRS_UPPER only pairs with b > a are members.
 *   - Rows.  The rows are the instances [first_row, first_row + row_count).  Cell (a, b) lives at index
 *     (a - first_row) * n + b, indexed in 64 bits, and holds
 *       count, an int64:  |{(ta, tb) : M(a, ta, b, tb)}|.  There is no cap of any kind.
 *       first, a uint64_t: the smallest key (ta << 32) | tb over the members, SHRAY_PAIRS_NONE where there are none.  That is
 *       the lexicographically smallest (ta, tb): a definite witness of where the two parts meet.
 *   - Either of first and counts may be NULL, not both.  With counts NULL the walk may skip what cannot lower a cell's key.
 *   - SHRAY_PAIRS_ANY needs first == NULL and counts; a cell's count is then 1 or 0, and the walk stops wherever a cell is
 *     already known to be 1.
 *   - The library itself sets the row_count * n cells on the stream before its launch (all-ones bytes for first, zero for
 *     counts), so the caller's buffers need no preparation.  row_count == 0 writes nothing.
 *   - The matrix is ordered and need not be symmetric: the per-pair test translates by the query's first corner, as
 *     include/shader_ray_intersect.h says, so M(a, ta, b, tb) and M(b, tb, a, ta) can differ in fp32.
 *   - The answer is independent of the top level, of any tree, of the order in which the device runs the workgroups, and of
 *     the row range asked for.
 *
 * Consequences.
 *   1. counts[a][b] equals the instance form's membership of include/shader_ray_instance_intersect.h (instance a, with
 *      SHRAY_INTERSECT_SKIP_OWN_INSTANCE) summed over the columns of instance b.
 *   2. first[a][b] is that membership's smallest (row, column of instance b) in row-major order.
 *   3. SHRAY_PAIRS_ANY's cell equals counts > 0.
 *   4. The diagonal is SHRAY_PAIRS_NONE / 0.
 *   5. SHRAY_PAIRS_UPPER clears the cells with b <= a and changes no other.
 *   6. The rows of a sub-range equal the same rows of the full matrix.
 *   7. "Some count of row a is positive" equals the instance form's SHRAY_INTERSECT_ANY over instance a's triangles.
 *   8. A duplicate instance meets its twin in both directions with equal counts.
 *   9. The matrix need not be symmetric.
 *
 * The walk is exact (DESIGN sections 24 and 31): include/shader_ray_instance_intersect.h's, with the same two culls (a member
 * node by its image box, a top-level node by its stored box under the guard; the root is not tested).  Beside them only two
 * skips prune, both by what a cell already holds: under SHRAY_PAIRS_ANY an instance b is not walked by a wave that reads 1 in
 * cell (a, b), and a lane stops at its first member; with counts NULL the lane of triangle ta does not enter b when the cell's
 * key has a high word below ta.  A cell only ever moves one way and every value it holds is a member's, so neither skip
 * changes the final value.  The counts form skips nothing.
 *
 * Errors, in this order: shray_pairs_params misuse (NULL, a wrong struct_size, unknown flag bits); SHRAY_PAIRS_ANY with first
 * != NULL or without counts; a negative first_row or row_count; a NULL set; rows beyond the set's instances; both outputs
 * NULL; an output pointer that is not 8-byte aligned.  All fail with SHRAY_ERR_INVALID_ARGUMENT before any device is touched.
 * (The counters form refuses a NULL counters pointer first.)  row_count == 0 is then a no-op.  A member scene whose tree is
 * higher than SHRAY_POINT_MAX_HEIGHT fails with SHRAY_ERR_BAD_TREE before any launch.  One launch serves the rows: one
 * 64-lane workgroup per 64 triangles of each row's instance, at most SHRAY_PAIRS_MAX_WORKGROUPS = 2^24 of them (2^30 lanes,
 * the grid the sibling queries' launches keep to); rows that need more are refused with SHRAY_ERR_INVALID_ARGUMENT before any
 * launch -- take fewer rows per call.
 *
 * The device form is stream-ordered: after a refit of a member scene and after shray_instance_set_update_device on the same
 * stream it sees the new geometry and the new set, and after a blocking shray_instance_set_update the new maps (their upload
 * is staged on the query's stream).  It takes (row_count + 1) uint32 of scratch from the stream's memory pool for the table
 * that tells a workgroup its instance, filled through pinned host memory, and gives it back in stream order.  It never
 * synchronises with the host, except that a member scene's first query by a library that walks the packed tree reads the
 * tree's height back once.
 */
#ifndef SHADER_RAY_INSTANCE_PAIRS_H
#define SHADER_RAY_INSTANCE_PAIRS_H

#include <stdint.h>

#include "shader_ray_instance.h"
#include "shader_ray_point.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
    SHRAY_PAIRS_ANY = 1,         /* flags: a cell's count is 1 or 0; needs first == NULL and counts */
    SHRAY_PAIRS_SKIP_SHARED = 2, /* flags: a pair whose world triangles share a corner is not a member */
    SHRAY_PAIRS_UPPER = 4        /* flags: only pairs with b > a are members */
};

#define SHRAY_PAIRS_NONE UINT64_MAX               /* first: the cell has no member */
#define SHRAY_PAIRS_MAX_WORKGROUPS (1u << 24)     /* the largest grid of the one launch */

typedef struct shray_pairs_params {
    uint32_t struct_size; /* sizeof(shray_pairs_params) */
    uint32_t flags;
    int32_t first_row;    /* the rows are the instances [first_row, first_row + row_count) */
    int32_t row_count;
} shray_pairs_params;

/* Asynchronous: row_count * n keys at d_first and row_count * n counts at d_counts (device memory of the set's device, 8-byte
 * aligned; either may be NULL), on `hip_stream` (NULL: the null stream).  The cells are initialised by the call. */
int shray_instance_pairs_intersect_device(shray_instance_set *set, const shray_pairs_params *op, uint64_t *d_first, int64_t *d_counts,
                                          void *hip_stream);

/* Blocking, host arrays (the same rules). */
int shray_instance_pairs_intersect(shray_instance_set *set, const shray_pairs_params *op, uint64_t *first, int64_t *counts);

/* Blocking, host arrays, with the work counters of the walk that skips nothing by what a cell already holds (under
 * SHRAY_PAIRS_ANY a lane still stops at its first member of an instance), summed over the query triangles' walks: node_visits
 * (image-box tests evaluated in the members' trees; the top level is not counted), leaf_visits and triangle_tests as in
 * include/shader_ray_intersect.h; traversals counts the instance walks begun; samples = the query triangles of the rows; the
 * other fields are 0. */
int shray_instance_pairs_intersect_counters(shray_instance_set *set, const shray_pairs_params *op, uint64_t *first, int64_t *counts,
                                            shray_counters *counters);

#ifdef __cplusplus
}
#endif

#endif /* SHADER_RAY_INSTANCE_PAIRS_H */
