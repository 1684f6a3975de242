/*
 * shader_ray_query.h -- ray queries on a resident scene: caller-supplied rays in, one hit record per ray out.
 *
 * libshray_query.so implements it, a client of libshray_hip.so (include/shader_ray_hip.h): a scene created there is
 * queried here, and errors are read with shray_last_error().  The query is the shader's group_intersect
 * (raytracer.es.fs:386-443) with the same arithmetic, visits and caps as the renderer's traversals.
 *
 * Semantics:
 *   - A ray is {origin[3], tmax, direction[3], reserved}, 32 bytes, in scene (object) space: the space of the scene's
 *     vertex_positions.  The direction is not normalised by the library.
 *   - The query is group_intersect over the range [0, 1e8] (the shader's range, fs:491), except that the running
 *     closest-hit bound starts at the ray's tmax instead of infinitely_far (1e7).  With tmax = 1e7 the hit and every
 *     work counter equal what the shader's primary traversal does for that ray.
 *   - A hit is reported iff the walk ends with t < tmax.  tmax <= 0 or NaN: a miss, with no traversal.  +inf is
 *     allowed.  (The walk starts from min(tmax, 1e8): no triangle beyond the range's end is ever accepted, so the two
 *     starting values give the same walk; the node stage of the stack kernel relies on the bound being at most 1e8.)
 *   - The hit is {t, u, v, triangle}, 16 bytes.  u, v are uvw.y and uvw.z of the shader's surface_hit; triangle is the
 *     scene's triangle index (the order of vertex_positions triples).  A miss is triangle = SHRAY_HIT_MISS with
 *     t, u, v as the walk left them: t = tmax (or a triangle's t accepted at exactly tmax); the iteration cap's bad hit
 *     (t == -1, fs:436-438) is triangle = SHRAY_HIT_CAP with t = -1.
 *   - any_hit: the walk stops at the first leaf that produced a hit (the renderer's shadow rays do the same).
 *     (any.triangle == SHRAY_HIT_MISS) == (closest.triangle == SHRAY_HIT_MISS) for every ray; when any.triangle >= 0,
 *     (t, u, v) are that triangle's own test result for the ray, with t < tmax.  Which triangle is not otherwise
 *     specified.
 *   - Kernel selection follows the renderer: a scene with a packed tree runs the packed stack traversal (kernel id 0,
 *     and every other id but 1); kernel id 1 (shray_scene_set_kernel), or a scene whose tables are not a canonical
 *     threaded tree, runs the literal threaded traversal.
 *
 * Errors: count == 0 is a no-op.  A negative count, a NULL pointer, a device pointer that is not 16-byte aligned or a
 * wrong struct_size fail with SHRAY_ERR_INVALID_ARGUMENT.  Counts beyond one launch's grid are split over launches.
 */
#ifndef SHADER_RAY_QUERY_H
#define SHADER_RAY_QUERY_H

#include <stdint.h>

#include "shader_ray_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct shray_ray {
    float origin[3];
    float tmax;
    float direction[3];
    float reserved;
} shray_ray;

typedef struct shray_hit {
    float t, u, v;
    int32_t triangle;   /* >= 0: the triangle hit; SHRAY_HIT_MISS; SHRAY_HIT_CAP */
} shray_hit;

enum { SHRAY_HIT_MISS = -1, SHRAY_HIT_CAP = -2 };

typedef struct shray_query_params {
    uint32_t struct_size;          /* sizeof(shray_query_params) */
    int32_t max_bvh_iterations;    /* node visits before the bad hit; 0 = no cap (400, the shader's) */
    int32_t max_leaf_tests;        /* triangles tested per leaf (10, the shader's) */
    int32_t any_hit;               /* 0: the closest hit; 1: any hit */
} shray_query_params;

/* the shader's defaults, struct_size set */
void shray_query_params_init(shray_query_params *qp);

/* Asynchronous: `count` rays at d_rays (device memory) -> `count` hits at d_hits, on `hip_stream` (NULL: the null stream). */
int shray_trace_rays_device(shray_scene *scene, const shray_query_params *qp, const shray_ray *d_rays, int64_t count,
                            shray_hit *d_hits, void *hip_stream);

/* Blocking, host arrays. */
int shray_trace_rays(shray_scene *scene, const shray_query_params *qp, const shray_ray *rays, int64_t count, shray_hit *hits);

/* Blocking, host arrays, with the walk's work counters: node_visits, leaf_visits, triangle_tests, traversals and bad_hits
 * are the full closest-hit walk's (any-hit rays are walked to their end here, as the renderer's counting twins walk their
 * shadow rays); samples = count; shaded_hits and env_lookups are 0.  `hits` may be NULL. */
int shray_trace_rays_counters(shray_scene *scene, const shray_query_params *qp, const shray_ray *rays, int64_t count,
                              shray_hit *hits, shray_counters *out);

/* One hit per pixel of a width x height frame (row 0 = the bottom row, render's layout): the 1-spp pixel-centre ray that
 * shray_render shades, in object space (object_matrix / object_normal_matrix, as the shader transforms it), tmax = 1e7.
 * params->which is ignored (always the which == 0 primary ray); max_bvh_iterations and max_leaf_tests are the frame's.
 * Asynchronous, on device memory: width * height hits at d_hits. */
int shray_primary_hits_device(shray_scene *scene, const shray_frame_params *params, int width, int height, shray_hit *d_hits,
                              void *hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* SHADER_RAY_QUERY_H */
