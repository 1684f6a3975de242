/*
 * shader_ray_intersect.h -- triangle-intersection queries on a resident scene: triangles in (caller-supplied, or the scene's
 * own); per query triangle, how many scene triangles it intersects and the K smallest of their indices in order.  Mesh against
 * mesh, a cutting sheet against a mesh, and whether and where a mesh passes through itself.
 *
 * libshray_intersect.so implements it, a client of libshray_hip.so (include/shader_ray_hip.h): a scene created there is
 * queried here, and errors are read with shray_last_error().  DESIGN section 19.
 *
 * Contract.
 *   - Input: shray_triangle { float a[3]; float pad0; float b[3]; float pad1; float c[3]; float pad2; }, 48 bytes, 16-byte
 *     aligned.  The pads are never read.
 *   - Params: shray_intersect_params { struct_size, max_triangles, flags, reserved }, 16 bytes.  max_triangles = K lies in
 *     [0, SHRAY_INTERSECT_MAX = 64]; shray_intersect_params_init sets K = 8.  flags is any combination of
 *     SHRAY_INTERSECT_ANY = 1 and SHRAY_INTERSECT_SKIP_SHARED = 2.
 *   - Per-pair test.  The query triangle Q has corners p0, p1, p2.  Scene triangle T (index i) has corners a, b, c at
 *     positions + 9 i.  The test is IEEE fp32 with no contraction.  min(x, y) is x < y ? x : y, max(x, y) is x > y ? x : y,
 *     min3(x, y, z) is min(min(x, y), z) and max3(x, y, z) is max(max(x, y), z).  Every comparison is written so that a NaN
 *     does not separate.  Touching counts as intersecting.
 *       Stage 0, the two vertex boxes, on the untranslated coordinates.  On axis j the pair is separated if
 *         min3(a_j, b_j, c_j) > max3(p0_j, p1_j, p2_j)  or  max3(a_j, b_j, c_j) < min3(p0_j, p1_j, p2_j).
 *       These are comparisons only, so there is no rounding.
 *       Shared corners, only with SHRAY_INTERSECT_SKIP_SHARED.  T is not a member if some corner of T equals some corner of
 *       Q.  "Equals" is three float == comparisons (x, y and z), so -0 equals +0 and a NaN equals nothing.  This removes the
 *       triangle itself and every neighbour over a vertex or an edge, which is what makes a self-intersection query
 *       meaningful.
 *       Translation by o = p0.
 *         q_i = p_i - o (q0 is exactly 0).  v0 = a - o, v1 = b - o, v2 = c - o.
 *         Query edges  f0 = q1 - q0, f1 = q2 - q1, f2 = q0 - q2.
 *         Scene edges  e0 = v1 - v0, e1 = v2 - v1, e2 = v0 - v2.
 *         x cross y = (x.y*y.z - x.z*y.y, x.z*y.x - x.x*y.z, x.x*y.y - x.y*y.x).
 *         x dot y = (x.x*y.x + x.y*y.y) + x.z*y.z.
 *         nq = f0 cross f1, nt = e0 cross e1.
 *       Degenerate triangles.  A query whose nq has all three components == 0 is not walked (n = 0, every index -1).  A
 *       scene triangle whose nt has all three components == 0 is not a member.  Seventeen axes do not decide segments and
 *       points; ray queries (shader_ray_query.h) serve segments.
 *       Seventeen axes, in this order:
 *          1      nq
 *          2      nt
 *          3-11   f_i cross e_j  (i outer, j inner)
 *         12-14   nq cross f_i
 *         15-17   nt cross e_j
 *       On axis A the pair is separated if
 *         min3(A dot v0, A dot v1, A dot v2) > max3(A dot q0, A dot q1, A dot q2)  or
 *         max3(A dot v0, A dot v1, A dot v2) < min3(A dot q0, A dot q1, A dot q2).
 *       The last six axes are what decide coplanar pairs.
 *   - The set is S = { i : no stage rejects T_i }.  It is defined over every triangle of the scene and is independent of the
 *     tree, of the visit order and of the order of the stages.
 *   - Outputs, per query:
 *       n = |S|, as an int32;
 *       K int32 indices at out[query * K + k]: the min(n, K) smallest members of S in ascending order, then SHRAY_HIT_MISS
 *       (-1).
 *     The indices for K are a prefix of the indices for any larger K.  query * K is indexed in 64 bits.
 *   - Unwalked queries.  A query with a non-finite coordinate, or a degenerate one (above), has n = 0 and all of its indices
 *     -1.  Nothing is walked for it.
 *   - SHRAY_INTERSECT_ANY needs K = 0 and a counts pointer.  The count written is 1 if S is non-empty and 0 otherwise.  The
 *     walk stops at the first member.  The result is still independent of the visit order.
 *   - There is no leaf-test cap and no iteration cap.
 *   - Not symmetric.  The translation is by the query's corner, so outside exact inputs i in S(Q_j) does not guarantee
 *     j in S(Q_i): the two tests round differently.
 *
 * The self form takes its queries from the scene: query j is the scene's own triangle first + j, read from the scene's
 * positions on the device at the time the kernel runs (nothing is repacked; after a refit on the same stream it is the moved
 * mesh).  It does not imply SHRAY_INTERSECT_SKIP_SHARED: without the flag every non-degenerate triangle finds itself and its
 * neighbours.
 *
 * The walk is exact, with no margin: stage 0 compares a triangle's own vertex box with the query's vertex
 * box, and a node's box is the exact min/max of the vertex coordinates below it, so a node whose box misses the query's vertex
 * box on some axis holds no triangle that passes stage 0.  The cull compares stored floats only, and it is the only cull.
 *
 * Coordinate range.  Measured on meshes whose largest coordinate is 1.7, scaled with their query triangles by S = 2^k
 * (tests/test_intersect_reference.py): the set of every query is the unscaled one for -33 <= k <= 29,
 * narrower than the box-overlap query's -27 .. 44 at the top.  Projections on nq cross f and nt cross e are fourth powers of a
 * coordinate difference: above the range they overflow (and an infinite or NaN projection stops separating), below it they
 * lose bits to underflow.  Outside the range the contract above still holds bit for bit: the set is what the arithmetic above
 * gives, and it always stays within stage 0's (tests/test_intersect_scale_reference.py and tests/test_gpu_intersect_scale.py:
 * 2^-80 to 2^64, on the scenes as loaded the sets are kept for -33 <= k <= 29 as well).
 *
 * Errors: count == 0 is a no-op.  A wrong struct_size, K outside [0, SHRAY_INTERSECT_MAX], unknown flag bits, a nonzero
 * reserved field, SHRAY_INTERSECT_ANY with K != 0 or without counts, K == 0 together with no counts (nothing is asked for;
 * with K == 0 the out pointer is neither read nor written), a negative count, a NULL scene, params or triangle pointer, a
 * NULL out pointer with K > 0, a triangle pointer that is not 16-byte aligned or an out or counts pointer that is not 4-byte
 * aligned, and in the self form a negative first, fail with SHRAY_ERR_INVALID_ARGUMENT before any device is touched; the
 * self form's first + count > the scene's triangle count fails with it before any launch.  A scene without a packed tree,
 * or one with a tree higher than SHRAY_POINT_MAX_HEIGHT, fails with SHRAY_ERR_BAD_TREE before any launch.  Counts beyond one
 * launch (2^24 queries) are split over launches.  The device forms are stream-ordered (after a refit on the same stream they
 * see the new geometry) and never synchronise with the host, except that a scene's first query by this library, the
 * closest-point library, the within-radius library, the box-overlap library or the all-hits library reads the tree's height
 * back once (they share that per-scene state; a refit never changes it).
 */
#ifndef SHADER_RAY_INTERSECT_H
#define SHADER_RAY_INTERSECT_H

#include <stdint.h>

#include "shader_ray_point.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { SHRAY_INTERSECT_MAX = 64 };
enum {
    SHRAY_INTERSECT_ANY = 1,          /* flags: only whether any triangle intersects the query */
    SHRAY_INTERSECT_SKIP_SHARED = 2   /* flags: a scene triangle that shares a corner with the query is not a member */
};

typedef struct shray_triangle {
    float a[3];
    float pad0;   /* never read */
    float b[3];
    float pad1;   /* never read */
    float c[3];
    float pad2;   /* never read */
} shray_triangle;

typedef struct shray_intersect_params {
    uint32_t struct_size;    /* sizeof(shray_intersect_params) */
    int32_t max_triangles;   /* K: 0 (counts only) .. SHRAY_INTERSECT_MAX */
    uint32_t flags;          /* SHRAY_INTERSECT_ANY | SHRAY_INTERSECT_SKIP_SHARED */
    int32_t reserved;        /* 0 */
} shray_intersect_params;

/* max_triangles = 8, flags = 0, struct_size set */
void shray_intersect_params_init(shray_intersect_params *op);

/* Asynchronous: `count` triangles at d_triangles (device memory of the scene's device) -> count * K indices at d_out (NULL
 * iff K == 0) and, unless d_counts is NULL, `count` intersection counts at d_counts, on `hip_stream` (NULL: the null
 * stream). */
int shray_intersect_triangles_device(shray_scene *scene, const shray_intersect_params *op, const shray_triangle *d_triangles,
                                     int64_t count, int32_t *d_out, int32_t *d_counts, void *hip_stream);

/* Blocking, host arrays (the same rules for indices and counts). */
int shray_intersect_triangles(shray_scene *scene, const shray_intersect_params *op, const shray_triangle *triangles, int64_t count,
                              int32_t *out, int32_t *counts);

/* Blocking, host arrays, with the work counters of the walk: node_visits (box tests evaluated), leaf_visits,
 * triangle_tests; samples = count; the other fields are 0. */
int shray_intersect_triangles_counters(shray_scene *scene, const shray_intersect_params *op, const shray_triangle *triangles,
                                       int64_t count, int32_t *out, int32_t *counts, shray_counters *counters);

/* Asynchronous, the self form: the queries are the scene's own triangles [first, first + count), query j at out[j * K] and
 * counts[j]; device memory of the scene's device, on `hip_stream`. */
int shray_intersect_self_device(shray_scene *scene, const shray_intersect_params *op, int64_t first, int64_t count, int32_t *d_out,
                                int32_t *d_counts, void *hip_stream);

/* Blocking, the self form into host arrays. */
int shray_intersect_self(shray_scene *scene, const shray_intersect_params *op, int64_t first, int64_t count, int32_t *out,
                         int32_t *counts);

#ifdef __cplusplus
}
#endif

#endif /* SHADER_RAY_INTERSECT_H */
