/*
 * shader_ray_multihit.h -- all-hits ray queries on a resident scene: caller-supplied rays in; per ray, how many surfaces it
 * crosses and the first K crossings in order.
 *
 * libshray_multihit.so implements it, a client of libshray_hip.so (include/shader_ray_hip.h): a scene created there is
 * queried here, and errors are read with shray_last_error().  DESIGN section 14.
 *
 * Contract.  Rays are shray_ray, hits are shray_hit; arithmetic is the ray query's (include/shader_ray_query.h: the shader's
 * range_intersect_box with true IEEE divisions over [0, 1e8], the shader's triangle_intersect, fp32, no FMA contraction).
 *
 * For one ray with tmax > 0 (else: no walk, zero hits), let B = tmax.  The crossing set S is defined without reference to any
 * visit order:
 *   - A node is entered iff its parent is entered (the root always is) and its own slab range satisfies
 *     !(r0 >= r1) && r0 < B.  These are exactly `enter` in ray_query_ref.trace with t held at tmax and never lowered.
 *   - A triangle at position j < max_leaf_tests of an entered leaf is in S iff the shader's test accepts it with bound B and
 *     that leaf's r0, r1 (the `ok` of ray_query_ref.trace: the determinant band, !(dist > B || dist < r0 || dist > r1), the
 *     u, w tests) and dist < tmax.
 *       - The last clause is the ray query's own report rule (t < tmax).
 *       - It also drops the NaN candidates that the comparison chain lets through.
 *   - Its record is {t = dist, u, v, triangle}, computed as the closest-hit walk computes it.
 *
 * Output per ray:
 *   - n = |S| as an int32 (the crossing count, which may exceed K);
 *   - K records in ray-major order, hits[ray * K + k];
 *   - the min(n, K) members of S with the smallest keys, sorted ascending by the key (t as a float comparison, then triangle
 *     index);
 *   - the remaining slots filled with {tmax, 0, 0, SHRAY_HIT_MISS}.
 *
 * There is no iteration cap: max_bvh_iterations does not exist in this query's params, and SHRAY_HIT_CAP never appears.
 * max_leaf_tests is honoured as in the ray query (default 10).
 *
 * Because S is a set and the order is a total order on it, the answer is independent of traversal order.  Consequences:
 *   - without counts, max_hits = 1 returns for every ray exactly the first record of the max_hits = 8 answer;
 *   - record 0 is the closest-hit query's record (uncapped) whenever the two smallest keys differ in t and the closest-hit
 *     walk accepted no NaN candidate (a closest-hit walk lowers its bound as it goes, so among equal t it keeps the first
 *     triangle in ITS visit order, and a NaN candidate it accepts poisons its bound).
 *
 * Errors: count == 0 is a no-op.  A negative count, a NULL scene, params or ray pointer, a NULL hit pointer with
 * max_hits > 0, both outputs NULL (max_hits == 0 counts as a NULL hit pointer: d_hits is then neither read nor written),
 * max_hits outside [0, SHRAY_MULTIHIT_MAX], max_leaf_tests outside [0, 2^24], a nonzero reserved, a wrong struct_size, a ray
 * or hit pointer that is not 16-byte aligned or a count pointer that is not 4-byte aligned fail with
 * SHRAY_ERR_INVALID_ARGUMENT before any device is touched.  A scene without a packed tree, or one with a tree higher than
 * SHRAY_POINT_MAX_HEIGHT, fails with SHRAY_ERR_BAD_TREE before any launch.  Counts beyond one launch (2^24 rays) are split
 * over launches.  The device form is stream-ordered (after a refit on the same stream it sees the new geometry) and never
 * synchronises with the host, except that a scene's first query by this library or by the closest-point library reads the tree's
 * height back once (they share that per-scene state; a refit never changes it).
 */
#ifndef SHADER_RAY_MULTIHIT_H
#define SHADER_RAY_MULTIHIT_H

#include <stdint.h>

#include "shader_ray_point.h"
#include "shader_ray_query.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { SHRAY_MULTIHIT_MAX = 64 };

typedef struct shray_multihit_params {
    uint32_t struct_size;     /* sizeof(shray_multihit_params) */
    int32_t max_hits;         /* K: 0 (counts only) .. SHRAY_MULTIHIT_MAX */
    int32_t max_leaf_tests;   /* triangles tested per leaf (10, the shader's) */
    int32_t reserved;         /* 0 */
} shray_multihit_params;

/* max_hits = 8, max_leaf_tests = 10, struct_size set */
void shray_multihit_params_init(shray_multihit_params *mp);

/* Asynchronous: `count` rays at d_rays (device memory of the scene's device) -> count * K hits at d_hits (NULL iff K == 0) and,
 * unless d_counts is NULL, `count` crossing counts at d_counts, on `hip_stream` (NULL: the null stream).  With d_counts NULL
 * the walk skips what cannot reach the first K: the same records, and less work wherever rays cross more than K surfaces. */
int shray_trace_all_hits_device(shray_scene *scene, const shray_multihit_params *mp, const shray_ray *d_rays, int64_t count,
                                shray_hit *d_hits, int32_t *d_counts, void *hip_stream);

/* Blocking, host arrays (the same rules for hits and counts). */
int shray_trace_all_hits(shray_scene *scene, const shray_multihit_params *mp, const shray_ray *rays, int64_t count,
                         shray_hit *hits, int32_t *counts);

/* Blocking, host arrays, with the work counters of the walk that skips nothing (every entered node, whatever K):
 * node_visits, leaf_visits, triangle_tests, traversals; bad_hits = 0; samples = count; shaded_hits and env_lookups are 0. */
int shray_trace_all_hits_counters(shray_scene *scene, const shray_multihit_params *mp, const shray_ray *rays, int64_t count,
                                  shray_hit *hits, int32_t *counts, shray_counters *out);

#ifdef __cplusplus
}
#endif

#endif /* SHADER_RAY_MULTIHIT_H */
