// scene_access_internal.h -- what libshray_query.so (query/) reads of a scene that scene_create.hip created: the device views the
// kernels take, and the FrameView a render would build; what libshray_refit.so (refit/) rewrites in place; and the slots where
// libshray_point.so (point/), libshray_sdf.so (sdf/) and libshray_winding.so (winding/) keep what they learn of a scene.  Host-only,
// internal to the libraries; not part of the C ABI.
#pragma once

#include <memory>

#include "device_types.h"
#include "shader_ray_hip.h"

struct ShrayQueryScene {
    shray::SceneView view;   // the scene's arrays on its device (reference layout, and the packed tree when packed_ok)
    int stack_levels;        // the deepest stack the packed tree asks for
    bool packed_ok;          // the packed tree exists: the stack traversal can run
    int kernel_id;           // shray_scene_set_kernel's choice
    int device;
};

extern "C" int shrayi_scene_query_view(const shray_scene *scene, ShrayQueryScene *out);
// shray_render's checks of (params, width, height) at one sample per pixel, then the FrameView it would launch, untiled
extern "C" int shrayi_frame_view(const shray_frame_params *params, int width, int height, shray::FrameView *out);

// The scene's arrays as the refit rewrites them (include/shader_ray_refit.h): mutable device pointers.  The packed tree's
// pointers and flat_of_packed are null unless packed_ok.
struct ShrayRefitScene {
    float *positions, *normals32;      // 3 floats per corner (reference layout)
    uint16_t *normals16;               // 3 halves per corner
    float *boxmin, *boxmax;            // 3 floats per node, the flattener's node numbering
    void *packed_nodes;                // DeviceNode[8][node_count] (packed_layout.h)
    void *packed_tris;                 // PackedTri[triangle_count + 1]
    void *pair_nodes;                  // PackedPair[node_count], or null
    const int32_t *flat_of_packed;     // [node_count]: packed node k is node flat_of_packed[k] of boxmin / boxmax
    uint32_t node_count, triangle_count;
    uint32_t packed_root;              // the root's packed index
    uint32_t exact_div_ok;
    bool packed_ok;
    int device;
    std::shared_ptr<void> *state;      // the refit library's own per-scene data (tree_order.h's height order, scratch); destroyed with the scene
};

extern "C" int shrayi_scene_refit_view(shray_scene *scene, ShrayRefitScene *out);
// the host-side flag every launch passes by value (SceneView::exact_div_ok): set after a refit from its new boxes
extern "C" int shrayi_scene_set_exact_div_ok(shray_scene *scene, uint32_t ok);

// libshray_point.so's own per-scene data (include/shader_ray_point.h: the tree's height), destroyed with the scene
extern "C" int shrayi_scene_point_state(shray_scene *scene, std::shared_ptr<void> **out);

// libshray_sdf.so's own per-scene data (include/shader_ray_sdf.h: the sign data), destroyed with the scene, and the scene's
// geometry generation: a host-side count of the refits that wrote new positions, which client_internal.h's make_current
// compares with the one the data was derived at.  Host-only, no device work.
extern "C" int shrayi_scene_sdf_state(shray_scene *scene, std::shared_ptr<void> **out, uint64_t *generation);
// libshray_winding.so's own per-scene data (include/shader_ray_winding.h: the node records and tree_order.h's height order),
// destroyed with the scene, and the same geometry generation.  Host-only, no device work.
extern "C" int shrayi_scene_winding_state(shray_scene *scene, std::shared_ptr<void> **out, uint64_t *generation);
// called by a refit (host or device form) once its validation has passed, before it enqueues the writes of new positions
extern "C" int shrayi_scene_geometry_changed(shray_scene *scene);
