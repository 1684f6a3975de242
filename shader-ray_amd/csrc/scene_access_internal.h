// scene_access_internal.h -- what libshray_query.so (query/) reads of a scene that capi.hip created: the device views the
// kernels take, and the FrameView a render would build.  Host-only, internal to the two libraries; not part of the C ABI.
#pragma once

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
