/*
 * shader_ray_refit.h -- refit a resident scene's BVH on the device after its vertices move.
 *
 * libshray_refit.so implements it, a client of libshray_hip.so (include/shader_ray_hip.h): a scene created there is refit
 * here, and errors are read with shray_last_error().  A refit keeps the tree and recomputes every coordinate the scene
 * derived from its vertices: the corners, the node boxes and what the renderer's kernels read of them.  A node's box is the
 * reference's box3d::add fold over the triangles of its contiguous range (bvh.cpp:304-309), each triangle's box its three
 * positions bumped out by 1e-5 (vectormath.h:189-195); min and max of finite floats do not depend on order, so the result
 * is pinned bit for bit.
 *
 * Semantics:
 *   - What stays the same.  The topology, the triangle order, the triangle indices in hits, the environment, the kernel id
 *     and the learnt dispatch order all stay as they were.
 *   - New positions.  Each scene triangle t gets new corner positions from vertex_data[triangle_vertices[3t+j]], or from
 *     corner 3t+j.  Its normals are set the same way, or kept when normal_offset_floats is -1.
 *   - New boxes.  Every node's box becomes the box3d::add fold of its range's triangle boxes.  This includes box3d's initial
 *     box for an empty range, if one exists.
 *   - Bit-for-bit result.  After the call, every array the scene holds equals what shray_scene_create would derive from the
 *     reference's get_shader_data arrays for the same tree with the new vertices.  That covers the literal arrays, the fp16
 *     normals, the octant copies, the pair records, the packed triangles and exact_div_ok.
 *   - Errors leave the scene unchanged.  The call returns SHRAY_ERR_INVALID_ARGUMENT in these cases, and the scene is left
 *     byte-for-byte unchanged: a NULL pointer; a wrong struct_size; a stride below 3; a normal offset that does not fit in
 *     the stride; an index outside [0, vertex_count); a corner count that does not match the scene; any non-finite position
 *     or normal.  This means the call validates before it writes.  Non-finite values are refused because a NaN would make
 *     the min/max fold depend on order.  (Every vertex at vertex_data is checked, used or not; colours are not read.)
 *   - The device form also refuses, with SHRAY_ERR_INVALID_ARGUMENT and before any launch, an array that is not device
 *     memory of the scene's device (a host pointer, another GPU's buffer) or whose allocation ends before the array does
 *     (vertex_count * vertex_stride_floats floats, 3 * triangles indices).
 *   - Scenes without a packed tree.  These fail with SHRAY_ERR_BAD_TREE.  packed_ok is false for them, so their topology
 *     was never proved.
 *   - Device and streams.  The refit runs on the scene's device.  Work on other streams that reads the scene (renders,
 *     queries) must be ordered by the caller.  The refit writes in place.
 *   - Why the call is blocking.  exact_div_ok sits in the host-side SceneView that every launch passes by value, so the call
 *     reads a few bytes back: once after the validation pass, once at the end.
 *   - sah_cost is computed in double from the float boxes: area(b) = 2(dx*dy + dx*dz + dy*dz) with dx = max(0, max.x - min.x)
 *     (box3d::dim's clamp at 0; the difference taken in double); interior nodes contribute area(n)/area(root) * SAH_CTRAV,
 *     leaves area(n)/area(root) * SAH_CISEC * count, with the reference defaults SAH_CTRAV = 1 and SAH_CISEC = 4
 *     (bvh.cpp:28-58).  Callers compare it with the value at creation to decide when a refit has degraded the tree enough to
 *     rebuild.  A zero-length-diagonal root gives 0.
 *
 * Cost: one validation pass, one pass per triangle, one per leaf, then the interior boxes bottom-up by node height -- one
 * launch per height while more than 1024 nodes share it, the rest in a single one-workgroup launch that steps through the
 * remaining heights behind workgroup barriers -- and one pass per node that writes the boxes out.  The first refit of a
 * scene also downloads its packed tree once to order the nodes by height.  A degenerate deep tree (BVH_MAX_DEPTH in the
 * thousands) costs at most node_count / 1024 height launches, plus one barrier step per remaining height in the
 * one-workgroup launch (not measured for such trees).
 */
#ifndef SHADER_RAY_REFIT_H
#define SHADER_RAY_REFIT_H

#include <stdint.h>

#include "shader_ray_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct shray_refit_input {
    uint32_t struct_size;              /* sizeof(shray_refit_input) */
    int32_t vertex_count;              /* vertices at vertex_data */
    int32_t vertex_stride_floats;      /* >= 3; the position first (geometry.h:34-38 layout: 9) */
    int32_t normal_offset_floats;      /* -1: the scene's normals are kept; else the normal's offset in a vertex (6 for geometry.h) */
    const float *vertex_data;
    const int32_t *triangle_vertices;  /* 3 vertex indices per triangle, in the SCENE's triangle order (post-build order);
                                          NULL: vertex_data holds the corners themselves, vertex_count == 3 * triangles */
} shray_refit_input;

typedef struct shray_refit_stats {
    double sah_cost;                   /* the tree's SAH cost over its new boxes (definition above) */
    int32_t exact_div_ok;              /* every new box coordinate is 0 or in [2^-70, 2^60) */
    int32_t reserved;
} shray_refit_stats;

/* host arrays; blocking */
int shray_scene_refit(shray_scene *scene, const shray_refit_input *in, shray_refit_stats *stats /* may be NULL */);
/* device arrays; ordered after earlier work on hip_stream, returns when the scene is updated */
int shray_scene_refit_device(shray_scene *scene, const shray_refit_input *in, shray_refit_stats *stats, void *hip_stream);
/* the scene's reference-layout geometry as it is now (any pointer may be NULL): vertex_positions, vertex_normals (3 floats per
 * corner), group_boxmin, group_boxmax (3 floats per node, the flattener's node numbering) */
int shray_scene_geometry_download(const shray_scene *scene, float *positions, float *normals, float *boxmin, float *boxmax);
/* the sizes of those arrays: corners (3 per triangle) and nodes */
int shray_scene_geometry_counts(const shray_scene *scene, int32_t *corners, int32_t *nodes);

#ifdef __cplusplus
}
#endif

#endif /* SHADER_RAY_REFIT_H */
