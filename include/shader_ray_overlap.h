/*
 * shader_ray_overlap.h -- box-overlap queries on a resident scene: caller-supplied axis-aligned boxes in; per box, how many
 * triangles touch it and the K smallest of their indices in order.
 *
 * libshray_overlap.so implements it, a client of libshray_hip.so (include/shader_ray_hip.h): a scene created there is
 * queried here, and errors are read with shray_last_error().  DESIGN section 17.
 *
 * Contract.
 *   - Input: shray_box { float lo[3]; float pad0; float hi[3]; float pad1; }, 32 bytes, 16-byte aligned.  The pads are never
 *     read.
 *   - Params: shray_overlap_params { struct_size, max_triangles, flags, reserved }, 16 bytes.  max_triangles = K lies in
 *     [0, SHRAY_OVERLAP_MAX = 64]; shray_overlap_params_init sets K = 8.  flags is 0 or SHRAY_OVERLAP_ANY.
 *   - Per-triangle test.  Triangle i has corners a, b, c at positions + 9 i.  The test is IEEE fp32 with no contraction.
 *     Every sum is evaluated left to right.  min(x, y) is x < y ? x : y, max(x, y) is x > y ? x : y, min3(x, y, z) is
 *     min(min(x, y), z) and max3(x, y, z) is max(max(x, y), z).
 *       Stage 0, box axes, on the untranslated coordinates.  On axis j the triangle is separated if
 *         min3(a_j, b_j, c_j) > hi_j  or  max3(a_j, b_j, c_j) < lo_j.
 *       These are comparisons only, so there is no rounding.
 *       Translation.
 *         m_j = 0.5f*lo_j + 0.5f*hi_j  and  h_j = 0.5f*hi_j - 0.5f*lo_j.
 *         v0 = a - m, v1 = b - m, v2 = c - m.
 *         e0 = v1 - v0, e1 = v2 - v1, e2 = v0 - v2.
 *       Stage 1, the plane.
 *         n = (e0.y*e1.z - e0.z*e1.y, e0.z*e1.x - e0.x*e1.z, e0.x*e1.y - e0.y*e1.x).
 *         d = (n.x*v0.x + n.y*v0.y) + n.z*v0.z.
 *         r = (h.x*|n.x| + h.y*|n.y|) + h.z*|n.z|.
 *         The triangle is separated if d > r or d < -r.
 *       Stage 2, nine edge axes.  Take edge e = e0, e1, e2 in that order, then axis x, y, z.  Take all three corners
 *       v = v0, v1, v2 (p0, p1, p2 in that order).
 *         x: p = e.y*v.z - e.z*v.y, r = h.y*|e.z| + h.z*|e.y|.
 *         y: p = e.z*v.x - e.x*v.z, r = h.x*|e.z| + h.z*|e.x|.
 *         z: p = e.x*v.y - e.y*v.x, r = h.x*|e.y| + h.y*|e.x|.
 *         The triangle is separated if min3(p0, p1, p2) > r or max3(p0, p1, p2) < -r.
 *     The triangle overlaps the box iff no axis separates it.  Every comparison is written so that a NaN (inf - inf on a huge
 *     input) does not separate.  Touching counts as overlapping.  Point and segment triangles are handled by the same 13 axes.
 *   - The set is S = { i : triangle i overlaps }.  It is defined over every triangle of the scene and is independent of the
 *     tree and of the visit order.  The order of the stages changes the work, not the set.
 *   - Outputs, per box:
 *       n = |S|, as an int32;
 *       K int32 indices at out[box * K + k]: the min(n, K) smallest members of S in ascending order, then SHRAY_HIT_MISS (-1).
 *     The indices for K are a prefix of the indices for any larger K.  box * K is indexed in 64 bits.
 *   - Unwalked boxes.  A box with a non-finite coordinate, or with lo_j > hi_j on any axis, has n = 0 and all of its indices
 *     -1.  Nothing is walked for it.  A zero-extent box is a valid box: a point, a segment or a rectangle.
 *   - SHRAY_OVERLAP_ANY needs K = 0 and a counts pointer.  The count written is 1 if S is non-empty and 0 otherwise.  The walk
 *     stops at the first overlapping triangle.  The result is still independent of the visit order.
 *   - There is no leaf-test cap and no iteration cap.
 *
 * The walk is exact, with no margin: stage 0 compares a triangle's own vertex box with the query box, and
 * a node's box is the exact min/max of the vertex coordinates below it, so a node whose box misses the query box on some axis
 * (node.hi_j < lo_j or node.lo_j > hi_j) holds no triangle that passes stage 0.  The cull compares stored floats only.
 *
 * Coordinate range.  Measured on meshes whose largest coordinate is 1.7, scaled with their boxes by S = 2^k
 * (tests/test_overlap_reference.py): the set of every box is the unscaled one for -27 <= k <= 44.  Below,
 * the products of the plane and edge stages (the cube of a coordinate difference) lose bits to underflow; above, they
 * overflow.  Outside the range the contract above still holds bit for bit: the set is what the arithmetic above gives
 * (tests/test_gpu_overlap_scale.py runs it from 2^-90 to 2^67).  What a caller then sees, on those meshes: the set stays
 * within stage 0's (the triangles whose vertex box meets the box), and it is NOT conservative: pairs are both gained and lost
 * at 2^-70, 2^-40 and 2^45 (products that lost bits, or one overflowed product beside a finite one, do separate) and from
 * 2^66 up, where the edge products overflow too.  It is a superset of the in-range set only where the plane alone has dropped
 * out (its products are 0, or infinite and NaN) and the edge axes work as before: at 2^-64, and at 2^50 and 2^64; and at
 * 2^-90, where every product of stages 1 and 2 is 0 and the set is exactly stage 0's.
 *
 * Errors: count == 0 is a no-op.  A wrong struct_size, K outside [0, SHRAY_OVERLAP_MAX], unknown flag bits, a nonzero
 * reserved field, SHRAY_OVERLAP_ANY with K != 0 or without counts, K == 0 together with no counts (nothing is asked for; with
 * K == 0 the out pointer is neither read nor written), a negative count, a NULL scene, params or box pointer, a NULL out
 * pointer with K > 0, a box pointer that is not 16-byte aligned or an out or counts pointer that is not 4-byte aligned fail
 * with SHRAY_ERR_INVALID_ARGUMENT before any device is touched.  A scene without a packed tree, or one with a tree higher
 * than SHRAY_POINT_MAX_HEIGHT, fails with SHRAY_ERR_BAD_TREE before any launch.  Counts beyond one launch (2^24 boxes) are
 * split over launches.  The device form is stream-ordered (after a refit on the same stream it sees the new geometry) and
 * never synchronises with the host, except that a scene's first query by this library, the closest-point library, the
 * within-radius library or the all-hits library reads the tree's height back once (they share that per-scene state; a refit
 * never changes it).
 */
#ifndef SHADER_RAY_OVERLAP_H
#define SHADER_RAY_OVERLAP_H

#include <stdint.h>

#include "shader_ray_point.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { SHRAY_OVERLAP_MAX = 64 };
enum { SHRAY_OVERLAP_ANY = 1 };   /* flags: only whether any triangle touches the box */

typedef struct shray_box {
    float lo[3];
    float pad0;   /* never read */
    float hi[3];
    float pad1;   /* never read */
} shray_box;

typedef struct shray_overlap_params {
    uint32_t struct_size;    /* sizeof(shray_overlap_params) */
    int32_t max_triangles;   /* K: 0 (counts only) .. SHRAY_OVERLAP_MAX */
    uint32_t flags;          /* 0 or SHRAY_OVERLAP_ANY */
    int32_t reserved;        /* 0 */
} shray_overlap_params;

/* max_triangles = 8, flags = 0, struct_size set */
void shray_overlap_params_init(shray_overlap_params *op);

/* Asynchronous: `count` boxes at d_boxes (device memory of the scene's device) -> count * K indices at d_out (NULL iff
 * K == 0) and, unless d_counts is NULL, `count` overlap counts at d_counts, on `hip_stream` (NULL: the null stream). */
int shray_overlap_triangles_device(shray_scene *scene, const shray_overlap_params *op, const shray_box *d_boxes, int64_t count,
                                   int32_t *d_out, int32_t *d_counts, void *hip_stream);

/* Blocking, host arrays (the same rules for indices and counts). */
int shray_overlap_triangles(shray_scene *scene, const shray_overlap_params *op, const shray_box *boxes, int64_t count, int32_t *out,
                            int32_t *counts);

/* Blocking, host arrays, with the work counters of the walk: node_visits (box tests evaluated), leaf_visits,
 * triangle_tests; samples = count; the other fields are 0. */
int shray_overlap_triangles_counters(shray_scene *scene, const shray_overlap_params *op, const shray_box *boxes, int64_t count,
                                     int32_t *out, int32_t *counts, shray_counters *counters);

#ifdef __cplusplus
}
#endif

#endif /* SHADER_RAY_OVERLAP_H */
