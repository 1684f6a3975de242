/*
 * shader_ray_clearance.h -- triangle-distance queries on a resident scene: triangles in (caller-supplied, or the scene's
 * own); per query triangle, how many scene triangles lie within a squared distance of it and the K nearest of them in order,
 * each with its squared distance and a witness point on either triangle.  How far apart two meshes are (clearance), whether
 * anything comes within a tolerance, and how thin a mesh's walls are (self-proximity).
 *
 * libshray_clearance.so implements it, a client of libshray_hip.so (include/shader_ray_hip.h): a scene created there is
 * queried here, and errors are read with shray_last_error().  DESIGN section 29.
 *
 * Contract.
 *   All arithmetic is IEEE fp32 with no contraction.
 *     dot(x,y) = (x.x*y.x + x.y*y.y) + x.z*y.z.
 *     pick_min(x,y) = x<y ? x : y, pick_max(x,y) = x>y ? x : y.
 *     clamp01(s) maps a non-finite s to 0, then s<0 to 0 and s>1 to 1.
 *   The query triangle Q has corners p0,p1,p2 (shray_triangle, pads never read).  The scene triangle T_i has corners a,b,c at
 *   positions + 9 i.
 *
 *   Fifteen features, evaluated in this order.  Each yields a witness x on Q, a witness y on T, and a dist2.
 *     Features 0-2.  Corner p_i against T through closest_on_triangle(p_i, T) (include/shader_ray_point.h), unchanged.
 *       x = p_i, y is its q, and dist2 is that function's own value.
 *     Features 3-5.  Scene corner a, b or c against Q through the same function with Q as the triangle.  y is the corner,
 *       x is its q, and dist2 is the function's own value.
 *     Features 6 + 3 i + j.  Query edge i (P = p_i, Qe = p_{(i+1)%3}) against scene edge j (R, S likewise over a,b,c).  This
 *       is Ericson 5.1.9 with zero thresholds:
 *         d1 = Qe-P, d2 = S-R, r = P-R;
 *         A = dot(d1,d1), E = dot(d2,d2), f = dot(d2,r), c = dot(d1,r), b = dot(d1,d2).
 *         If !(A>0) and !(E>0): s = t = 0.
 *         Else if !(A>0): s = 0, t = clamp01(f/E).
 *         Else if !(E>0): t = 0, s = clamp01((-c)/A).
 *         Otherwise:
 *           den = A*E - b*b;
 *           s = den != 0 ? clamp01((b*f - c*E)/den) : 0;
 *           t = (b*s + f)/E, with a non-finite t set to 0;
 *           if t<0: t = 0, s = clamp01((-c)/A);
 *           else if t>1: t = 1, s = clamp01((b-c)/A).
 *         x = P + d1*s, clamped per axis to the min/max of its segment's two endpoints with pick_max then pick_min.
 *         y = R + d2*t, clamped the same way to its own segment's endpoints.
 *         dist2 = dot(x-y, x-y).
 *   The pair's (dist2, feature, x, y) comes from the feature with the smallest dist2.  A tie goes to the lowest feature
 *   number.  (The features are taken in order against a running minimum that a later feature replaces only when its dist2 is
 *   less, by a float <.)
 *
 *   Intersecting stage.  The stage applies when Q's nq is not all zero and the 17-axis test of shader_ray_intersect.h does
 *   not reject T.  It is run without its shared-corner stage, and T's nt must not be all zero.  The pair then has
 *   dist2 = +0 and feature = SHRAY_PAIR_INTERSECTING (15).  The witnesses stay those of the feature minimum: they are points
 *   of the two triangles, not a contact point.  A degenerate Q or T never takes this stage, so points and segments passed as
 *   triangles are served by the features alone.
 *
 *   SHRAY_CLEARANCE_SKIP_SHARED.  With this flag, T is not a member if any of its corners == any of Q's, by three float ==
 *   per corner.  This check comes before everything else.
 *
 *   Members.  S = { i : dist2_i <= max_dist2 }.  max_dist2 is one value per call, carried in the params, and +inf is
 *   allowed.  S is defined over every triangle of the scene.
 *
 *   Outputs per query.
 *     n = |S|.
 *     The min(n,K) members with the smallest (dist2, triangle), as 48-byte records, 16-byte aligned:
 *       shray_pair_distance { float on_query[3]; float dist2; float on_scene[3]; int32_t triangle; int32_t feature;
 *                             int32_t reserved[3] (0) }.
 *     Miss records fill the rest: on_query = on_scene = 0, dist2 = max_dist2 as given, triangle = feature = -1.
 *     K lies in [0, 64].  The records for K are a prefix of those for any larger K.
 *
 *   Unwalked queries.  A non-finite coordinate in Q, or a NaN or negative max_dist2, gives n = 0 and all miss records.
 *   There is no leaf cap and no iteration cap.
 *
 *   SHRAY_CLEARANCE_ANY.  This is the tolerance query.  It needs K = 0 and a counts pointer.  It writes 1 or 0 and stops at
 *   the first member.
 *
 *   Not symmetric.  The intersecting stage translates by the query's corner, so outside exact inputs the answer for
 *   (Q, T) is not guaranteed to be the answer for (T, Q): the two tests round differently, and the features are numbered
 *   from the query's side.
 *
 *   Params.  shray_clearance_params { struct_size, max_pairs (K, init 1), flags, max_dist2 (init +inf) }, 16 bytes.
 *
 * The self form takes its queries from the scene: query j is the scene's own triangle first + j, read from the scene's
 * positions on the device at the time the kernel runs (nothing is repacked; after a refit on the same stream it is the moved
 * mesh).  It does not imply SHRAY_CLEARANCE_SKIP_SHARED: without the flag every triangle finds itself and its neighbours at
 * distance 0.
 *
 * The walk is exact, with no margin.  A node is skipped only when lb > reach, where lb = dot(g,g) and per
 * axis g = qlo > hi ? qlo - hi : (lo > qhi ? lo - qhi : 0), [qlo, qhi] being Q's vertex box and [lo, hi] the node's; reach is
 * max_dist2, or in the form that writes no counts the K-th smallest dist2 held.  lb <= dist2(Q,T) bit for bit for every T
 * below the node: every witness x is clamped into Q's vertex box, every witness y into T's vertex box, which lies inside the
 * node's exact min/max box; rounding, squaring and the sum are monotone; and an intersecting pair passed the vertex-box stage,
 * so its boxes overlap and lb = 0.  A node with lb == reach is entered.
 *
 * Errors: count == 0 is a no-op.  A wrong struct_size, K outside [0, SHRAY_CLEARANCE_MAX], unknown flag bits,
 * SHRAY_CLEARANCE_ANY with K != 0 or without counts, K == 0 together with no counts (nothing is asked for; with K == 0 the out
 * pointer is neither read nor written), a negative count, a NULL scene, params or triangle pointer, a NULL out pointer with
 * K > 0, a triangle or record pointer that is not 16-byte aligned or a counts pointer that is not 4-byte aligned, and in the
 * self form a negative first, fail with SHRAY_ERR_INVALID_ARGUMENT before any device is touched; the self form's
 * first + count > the scene's triangle count fails with it before any launch.  A scene without a packed tree, or one with a
 * tree higher than SHRAY_POINT_MAX_HEIGHT, fails with SHRAY_ERR_BAD_TREE before any launch.  Counts beyond one launch (2^24
 * queries) are split over launches.  The device forms are stream-ordered (after a refit on the same stream they see the new
 * geometry) and never synchronise with the host, except that a scene's first query by this library or by another that walks
 * the packed tree reads the tree's height back once (they share that per-scene state; a refit never changes it).
 */
#ifndef SHADER_RAY_CLEARANCE_H
#define SHADER_RAY_CLEARANCE_H

#include <stdint.h>

#include "shader_ray_intersect.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { SHRAY_CLEARANCE_MAX = 64 };
enum {
    SHRAY_CLEARANCE_ANY = 1,          /* flags: only whether any triangle is within max_dist2 of the query */
    SHRAY_CLEARANCE_SKIP_SHARED = 2   /* flags: a scene triangle that shares a corner with the query is not a member */
};
enum { SHRAY_PAIR_INTERSECTING = 15 };   /* feature: the pair intersects (dist2 = +0); 0 .. 14 are the contract's features */

typedef struct shray_pair_distance {
    float on_query[3];     /* the witness x on the query triangle */
    float dist2;
    float on_scene[3];     /* the witness y on the scene triangle */
    int32_t triangle;      /* SHRAY_HIT_MISS (-1): a miss record */
    int32_t feature;       /* 0 .. 14, SHRAY_PAIR_INTERSECTING, or -1 in a miss record */
    int32_t reserved[3];   /* 0 */
} shray_pair_distance;

typedef struct shray_clearance_params {
    uint32_t struct_size;   /* sizeof(shray_clearance_params) */
    int32_t max_pairs;      /* K: 0 (counts only) .. SHRAY_CLEARANCE_MAX */
    uint32_t flags;         /* SHRAY_CLEARANCE_ANY | SHRAY_CLEARANCE_SKIP_SHARED */
    float max_dist2;        /* members have dist2 <= max_dist2; +inf: every triangle */
} shray_clearance_params;

/* max_pairs = 1, flags = 0, max_dist2 = +inf, struct_size set */
void shray_clearance_params_init(shray_clearance_params *op);

/* Asynchronous: `count` triangles at d_triangles (device memory of the scene's device) -> count * K records at d_out (NULL
 * iff K == 0) and, unless d_counts is NULL, `count` member counts at d_counts, on `hip_stream` (NULL: the null stream). */
int shray_clearance_triangles_device(shray_scene *scene, const shray_clearance_params *op, const shray_triangle *d_triangles,
                                     int64_t count, shray_pair_distance *d_out, int32_t *d_counts, void *hip_stream);

/* Blocking, host arrays (the same rules for records and counts). */
int shray_clearance_triangles(shray_scene *scene, const shray_clearance_params *op, const shray_triangle *triangles, int64_t count,
                              shray_pair_distance *out, int32_t *counts);

/* Blocking, host arrays, with the work counters of the walk that skips nothing within max_dist2: node_visits (box bounds
 * evaluated), leaf_visits, triangle_tests (pairs whose features were evaluated); samples = count; the other fields are 0. */
int shray_clearance_triangles_counters(shray_scene *scene, const shray_clearance_params *op, const shray_triangle *triangles,
                                       int64_t count, shray_pair_distance *out, int32_t *counts, shray_counters *counters);

/* Asynchronous, the self form: the queries are the scene's own triangles [first, first + count), query j at out[j * K] and
 * counts[j]; device memory of the scene's device, on `hip_stream`. */
int shray_clearance_self_device(shray_scene *scene, const shray_clearance_params *op, int64_t first, int64_t count,
                                shray_pair_distance *d_out, int32_t *d_counts, void *hip_stream);

/* Blocking, the self form into host arrays. */
int shray_clearance_self(shray_scene *scene, const shray_clearance_params *op, int64_t first, int64_t count, shray_pair_distance *out,
                         int32_t *counts);

#ifdef __cplusplus
}
#endif

#endif /* SHADER_RAY_CLEARANCE_H */
