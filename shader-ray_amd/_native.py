"""ctypes mirror of include/shader_ray_hip.h and include/shader_ray_host.h.

Plumbing only: structure layouts, library loading, error translation.  There is no
CPU fallback -- if a shared library is missing the loaders raise, loudly.
"""
from __future__ import annotations

import ctypes as C
import os

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
# SHRAY_HOST_LIB selects another build of the host layer (the sanitizer build, `make -C shader-ray_amd sanitize`: tests/test_sanitizers.py)
HOST_LIB = os.environ.get("SHRAY_HOST_LIB") or os.path.join(PKG_DIR, "libshray_host.so")
DIST_LIB = os.path.join(PKG_DIR, "libshray_dist.so")
QUERY_LIB = os.path.join(PKG_DIR, "libshray_query.so")
REFIT_LIB = os.path.join(PKG_DIR, "libshray_refit.so")
INSTANCE_LIB = os.path.join(PKG_DIR, "libshray_instance.so")
POINT_LIB = os.path.join(PKG_DIR, "libshray_point.so")
SDF_LIB = os.path.join(PKG_DIR, "libshray_sdf.so")
WINDING_LIB = os.path.join(PKG_DIR, "libshray_winding.so")
MULTIHIT_LIB = os.path.join(PKG_DIR, "libshray_multihit.so")
INSTANCE_MULTIHIT_LIB = os.path.join(PKG_DIR, "libshray_instance_multihit.so")
INSTANCE_POINT_LIB = os.path.join(PKG_DIR, "libshray_instance_point.so")
# SHRAY_INSTANCE_NEAR_LIB selects an experiment build of the same library (the stack entry); unset in normal use
INSTANCE_NEAR_LIB = os.environ.get("SHRAY_INSTANCE_NEAR_LIB") or os.path.join(PKG_DIR, "libshray_instance_near.so")
# SHRAY_NEAR_LIB selects an experiment build of the same library (profiles/near_bench.py --ab); unset in normal use
NEAR_LIB = os.environ.get("SHRAY_NEAR_LIB") or os.path.join(PKG_DIR, "libshray_near.so")
OVERLAP_LIB = os.path.join(PKG_DIR, "libshray_overlap.so")
INSTANCE_OVERLAP_LIB = os.path.join(PKG_DIR, "libshray_instance_overlap.so")
INTERSECT_LIB = os.path.join(PKG_DIR, "libshray_intersect.so")
INSTANCE_INTERSECT_LIB = os.path.join(PKG_DIR, "libshray_instance_intersect.so")
CLEARANCE_LIB = os.path.join(PKG_DIR, "libshray_clearance.so")
INSTANCE_CLEARANCE_LIB = os.path.join(PKG_DIR, "libshray_instance_clearance.so")
INSTANCE_PAIRS_LIB = os.path.join(PKG_DIR, "libshray_instance_pairs.so")
INSTANCE_SDF_LIB = os.path.join(PKG_DIR, "libshray_instance_sdf.so")
INSTANCE_WINDING_LIB = os.path.join(PKG_DIR, "libshray_instance_winding.so")
# SHRAY_HIP_LIB selects an experiment build of the same library (profiles/variant_sweep.sh); unset in normal use
HIP_LIB = os.environ.get("SHRAY_HIP_LIB") or os.path.join(PKG_DIR, "libshray_hip.so")

c_float_p = C.POINTER(C.c_float)
ENV_FLOAT32, ENV_UNORM8 = 0, 1
ABI_VERSION = 4   # SHRAY_ABI_VERSION of the header these structures mirror (tests/test_abi.py compares the two)


class SceneDesc(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("data_texture_width", C.c_uint32),
        ("vertex_count", C.c_uint32), ("vertex_data_rows", C.c_uint32),
        ("vertex_positions", c_float_p), ("vertex_normals", c_float_p), ("vertex_colors", c_float_p),
        ("group_count", C.c_int32), ("group_data_rows", C.c_int32), ("tree_root", C.c_int32),
        ("group_boxmin", c_float_p), ("group_boxmax", c_float_p),
        ("group_directions", c_float_p), ("group_children", c_float_p),
        ("group_hitmiss", c_float_p), ("group_objects", c_float_p),
    ]


class FrameParams(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("which", C.c_int32),
        ("camera_matrix", C.c_float * 16), ("camera_normal_matrix", C.c_float * 16),
        ("object_matrix", C.c_float * 16), ("object_inverse", C.c_float * 16),
        ("object_normal_matrix", C.c_float * 16), ("object_normal_inverse", C.c_float * 16),
        ("image_plane_width", C.c_float), ("aspect", C.c_float),
        ("right", C.c_float * 3), ("up", C.c_float * 3), ("light_dir", C.c_float * 3),
        ("specular_color", C.c_float * 3), ("diffuse_color", C.c_float * 3),
        ("bounce_count", C.c_int32), ("max_bvh_iterations", C.c_int32), ("max_leaf_tests", C.c_int32),
        ("cast_shadows", C.c_int32), ("tonemap", C.c_int32), ("normals_fp16", C.c_int32),
    ]

    def copy(self) -> "FrameParams":
        other = FrameParams()
        C.memmove(C.byref(other), C.byref(self), C.sizeof(FrameParams))
        return other


class TileSet(C.Structure):
    _fields_ = [("tile_w", C.c_int32), ("tile_h", C.c_int32), ("tile_stride", C.c_int32), ("tile_phase", C.c_int32),
                ("tile_phase_count", C.c_int32)]


class Counters(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in (
        "node_visits", "leaf_visits", "triangle_tests", "shaded_hits", "env_lookups",
        "traversals", "bad_hits", "samples")]

    def as_dict(self) -> dict:
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class TreeDesc(C.Structure):
    """shray_tree_desc (include/shader_ray_hip.h): the BVH as pre-order arrays, input of the GPU flattener."""
    _fields_ = [
        ("struct_size", C.c_uint32), ("node_count", C.c_int32),
        ("node_parent", C.POINTER(C.c_int32)), ("node_negative", C.POINTER(C.c_int32)), ("node_positive", C.POINTER(C.c_int32)),
        ("node_box", C.POINTER(C.c_float)), ("node_direction", C.POINTER(C.c_float)),
        ("node_start", C.POINTER(C.c_int32)), ("node_triangles", C.POINTER(C.c_int32)),
        ("triangle_count", C.c_int32), ("triangle_vertices", C.POINTER(C.c_int32)),
        ("vertex_count", C.c_int32), ("vertex_data", C.POINTER(C.c_float)),
    ]


class HostView(C.Structure):
    _fields_ = [
        ("fov", C.c_float), ("zoom", C.c_float), ("object_rotation", C.c_float * 4),
        ("object_position", C.c_float * 3), ("light_rotation", C.c_float * 4),
        ("which", C.c_int32), ("which_material", C.c_int32), ("which_diffuse_color", C.c_int32),
    ]


class HostWorldInfo(C.Structure):
    _fields_ = [
        ("triangle_count", C.c_int32), ("independent_vertex_count", C.c_int32),
        ("scene_center", C.c_float * 3), ("scene_extent", C.c_float),
        ("node_count", C.c_int32), ("leaf_count", C.c_int32), ("max_level", C.c_int32),
        ("large_leaves", C.c_int32), ("parse_seconds", C.c_double), ("build_seconds", C.c_double),
    ]


class BvhOptions(C.Structure):
    """shray_bvh_options (include/shader_ray_hip.h): the reference's build parameters (bvh.cpp:28-58)."""
    _fields_ = [("struct_size", C.c_uint32), ("max_depth", C.c_int32), ("leaf_max", C.c_int32), ("sah_ctrav", C.c_float), ("sah_cisec", C.c_float)]


class BvhStats(C.Structure):
    _fields_ = [("node_count", C.c_int32), ("leaf_count", C.c_int32), ("max_level", C.c_int32), ("large_leaves", C.c_int32),
                ("device_seconds", C.c_double)]


# Every symbol include/shader_ray_hip.h declares: (name, restype, argtypes)
HIP_SYMBOLS = [
    ("shray_abi_version", C.c_int, []),
    ("shray_last_error", C.c_char_p, []),
    ("shray_device_count", C.c_int, [C.POINTER(C.c_int)]),
    ("shray_set_device", C.c_int, [C.c_int]),
    ("shray_frame_params_init", None, [C.POINTER(FrameParams)]),
    ("shray_scene_create", C.c_int, [C.POINTER(SceneDesc), C.POINTER(C.c_void_p)]),
    ("shray_scene_set_environment", C.c_int, [C.c_void_p, c_float_p, C.c_int, C.c_int]),
    ("shray_scene_set_environment_storage", C.c_int, [C.c_void_p, c_float_p, C.c_int, C.c_int, C.c_int]),
    ("shray_scene_destroy", C.c_int, [C.c_void_p]),
    ("shray_scene_device", C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    ("shray_scene_set_kernel", C.c_int, [C.c_void_p, C.c_int]),
    ("shray_render", C.c_int, [C.c_void_p, C.POINTER(FrameParams), C.c_int, C.c_int, C.c_int, c_float_p]),
    ("shray_render_host_async", C.c_int, [C.c_void_p, C.POINTER(FrameParams), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    ("shray_pinned_alloc", C.c_int, [C.c_size_t, C.POINTER(C.c_void_p)]),
    ("shray_pinned_free", C.c_int, [C.c_void_p]),
    ("shray_flatten_device", C.c_int, [C.POINTER(TreeDesc), C.c_uint32, C.POINTER(C.c_void_p)]),
    ("shray_device_flat_describe", C.c_int, [C.c_void_p, C.POINTER(SceneDesc)]),
    ("shray_device_flat_download", C.c_int, [C.c_void_p, C.POINTER(SceneDesc)]),
    ("shray_device_flat_destroy", C.c_int, [C.c_void_p]),
    ("shray_bvh_build_device", C.c_int, [C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_float), C.c_int32, C.c_int32, C.POINTER(BvhOptions),
                                         C.POINTER(C.c_void_p)]),
    ("shray_device_tree_download", C.c_int, [C.c_void_p, C.POINTER(TreeDesc), C.POINTER(C.POINTER(C.c_int32))]),
    ("shray_device_tree_stats", C.c_int, [C.c_void_p, C.POINTER(BvhStats)]),
    ("shray_device_tree_destroy", C.c_int, [C.c_void_p]),
    ("shray_flatten_device_tree", C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]),
    ("shray_scene_create_from_device", C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    ("shray_scene_derived_sizes", C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                            C.POINTER(C.c_uint64), C.POINTER(C.c_int32)]),
    ("shray_scene_derived_download", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("shray_render_device", C.c_int, [C.c_void_p, C.POINTER(FrameParams), C.c_int, C.c_int, C.c_int,
                                      C.POINTER(TileSet), C.c_void_p, C.c_void_p]),
    ("shray_render_batch_device", C.c_int, [C.c_void_p, C.POINTER(FrameParams), C.c_int, C.c_int, C.c_int, C.c_int,
                                            C.POINTER(TileSet), C.c_void_p, C.c_int64, C.c_void_p]),
    ("shray_tile_buffer_bytes", C.c_int64, [C.c_int, C.c_int, C.POINTER(TileSet)]),
    ("shray_assemble_tiles_device", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64,
                                              C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    ("shray_assemble_tiles_split_device", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64,
                                                    C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    ("shray_render_counters", C.c_int, [C.c_void_p, C.POINTER(FrameParams), C.c_int, C.c_int, C.c_int,
                                        c_float_p, C.POINTER(Counters)]),
    ("shray_render_counters_timed", C.c_int, [C.c_void_p, C.POINTER(FrameParams), C.c_int, C.c_int, C.c_int, C.c_int,
                                              c_float_p, C.POINTER(Counters)]),
    ("shray_scene_dispatch_order", C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_uint32)]),
    ("shray_scene_set_view_cache", C.c_int, [C.c_void_p, C.c_int]),
    ("shray_scene_view_cache_stats", C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    ("shray_selftest_division", C.c_int, [C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64)]),
    ("shray_selftest_reciprocal", C.c_int, [C.POINTER(C.c_uint64)]),
    ("shray_probe_vector_cache", C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
]

HOST_SYMBOLS = [
    ("shray_host_load_world", C.c_int, [C.c_char_p, C.POINTER(C.c_void_p)]),
    ("shray_host_free_world", None, [C.c_void_p]),
    ("shray_host_load_triangles", C.c_int, [C.c_char_p, C.POINTER(C.c_void_p)]),
    ("shray_host_triangles", C.c_int, [C.c_void_p, C.POINTER(C.POINTER(C.c_int32)), C.POINTER(C.c_int32), C.POINTER(C.POINTER(C.c_float)),
                                       C.POINTER(C.c_int32)]),
    ("shray_host_adopt_tree", C.c_int, [C.c_void_p, C.POINTER(TreeDesc), C.POINTER(C.c_int32), C.c_double]),
    ("shray_host_bvh_options", C.c_int, [C.POINTER(BvhOptions)]),
    ("shray_host_get_world_info", C.c_int, [C.c_void_p, C.POINTER(HostWorldInfo)]),
    ("shray_host_flatten", C.c_int, [C.c_void_p, C.c_uint, C.POINTER(SceneDesc)]),
    ("shray_host_export_tree", C.c_int, [C.c_void_p, C.POINTER(TreeDesc)]),
    ("shray_host_default_view", C.c_int, [C.c_void_p, C.POINTER(HostView)]),
    ("shray_host_frame_params", C.c_int, [C.c_void_p, C.POINTER(HostView), C.c_int, C.c_int, C.POINTER(FrameParams)]),
    ("shray_host_trackball_motion", C.c_int, [C.POINTER(C.c_float), C.c_float, C.c_float, C.POINTER(C.c_float)]),
    ("shray_host_load_background", C.c_int, [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(c_float_p)]),
    ("shray_host_free_background", None, [c_float_p]),
    ("shray_host_set_quiet", None, [C.c_int]),
]

# include/shader_ray_dist.h ------------------------------------------------------------------------------
DIST_ROOT0, DIST_ROTATE = 0, 1
DIST_RCCL, DIST_LOOPBACK, DIST_CALLBACK = 0, 1, 2
DIST_UNIQUE_ID_BYTES = 128
MAX_BATCH = 64
DIST_MAX_WORLD = 64


class DistConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("rank", C.c_int32), ("world", C.c_int32),
                ("width", C.c_int32), ("height", C.c_int32), ("spp", C.c_int32),
                ("tile_w", C.c_int32), ("tile_h", C.c_int32), ("max_frames", C.c_int32), ("root_mode", C.c_int32),
                ("rank0_phases", C.c_int32), ("other_phases", C.c_int32), ("rgb_wire", C.c_int32),
                ("transport", C.c_int32), ("buffer_sets", C.c_int32)]


class DistXfer(C.Structure):
    _fields_ = [("peer", C.c_int32), ("frame", C.c_int32), ("offset_bytes", C.c_int64), ("bytes", C.c_int64)]


class DistPlan(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("tiles", TileSet), ("rank0_phases", C.c_int32), ("other_phases", C.c_int32),
                ("channels", C.c_int32), ("max_assembled", C.c_int32), ("owned_tiles", C.c_int64), ("max_tiles", C.c_int64),
                ("render_frame_stride_bytes", C.c_int64), ("wire_frame_stride_bytes", C.c_int64),
                ("gather_rank_stride_bytes", C.c_int64), ("gather_frame_stride_bytes", C.c_int64)]


DIST_EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.POINTER(DistXfer), C.c_int, C.c_void_p, C.POINTER(DistXfer),
                               C.c_int, C.c_void_p)


class DistCallbacks(C.Structure):
    _fields_ = [("user", C.c_void_p), ("exchange", DIST_EXCHANGE_FN)]


DIST_SYMBOLS = [
    ("shray_dist_last_error", C.c_char_p, []),
    ("shray_dist_balanced_shares", C.c_int, [C.c_int, C.c_double, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    ("shray_dist_make_plan", C.c_int, [C.POINTER(DistConfig), C.POINTER(DistPlan)]),
    ("shray_dist_frame_owner", C.c_int, [C.POINTER(DistConfig), C.c_int]),
    ("shray_dist_step_xfers", C.c_int, [C.POINTER(DistConfig), C.c_int, C.POINTER(DistXfer), C.POINTER(C.c_int),
                                        C.POINTER(DistXfer), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                        C.POINTER(C.c_int)]),
    ("shray_dist_unique_id", C.c_int, [C.c_void_p]),
    ("shray_dist_hub_create", C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    ("shray_dist_hub_destroy", C.c_int, [C.c_void_p]),
    ("shray_dist_create", C.c_int, [C.c_void_p, C.POINTER(DistConfig), C.c_void_p, C.POINTER(C.c_void_p)]),
    ("shray_dist_destroy", C.c_int, [C.c_void_p]),
    ("shray_dist_world", C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    ("shray_dist_step", C.c_int, [C.c_void_p, C.c_int, C.POINTER(FrameParams), C.c_int, C.c_void_p]),
    ("shray_dist_set_timing", C.c_int, [C.c_void_p, C.c_int]),
    ("shray_dist_step_times", C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    ("shray_dist_output", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                    C.POINTER(C.c_void_p)]),
    ("shray_dist_copy_output", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    ("shray_dist_copy_to_host", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    ("shray_dist_copy_to_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
]

# include/shader_ray_query.h ------------------------------------------------------------------------------
HIT_MISS, HIT_CAP = -1, -2


class Ray(C.Structure):
    """shray_ray: object-space origin, tmax, direction, one reserved float (32 bytes)."""
    _fields_ = [("origin", C.c_float * 3), ("tmax", C.c_float), ("direction", C.c_float * 3), ("reserved", C.c_float)]


class Hit(C.Structure):
    """shray_hit: t, u, v, triangle (HIT_MISS, HIT_CAP or the scene's triangle index)."""
    _fields_ = [("t", C.c_float), ("u", C.c_float), ("v", C.c_float), ("triangle", C.c_int32)]


class QueryParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("max_bvh_iterations", C.c_int32), ("max_leaf_tests", C.c_int32), ("any_hit", C.c_int32)]


QUERY_SYMBOLS = [
    ("shray_query_params_init", None, [C.POINTER(QueryParams)]),
    ("shray_trace_rays_device", C.c_int, [C.c_void_p, C.POINTER(QueryParams), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    ("shray_trace_rays", C.c_int, [C.c_void_p, C.POINTER(QueryParams), C.c_void_p, C.c_int64, C.c_void_p]),
    ("shray_trace_rays_counters", C.c_int, [C.c_void_p, C.POINTER(QueryParams), C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(Counters)]),
    ("shray_primary_hits_device", C.c_int, [C.c_void_p, C.POINTER(FrameParams), C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
]

# include/shader_ray_refit.h ------------------------------------------------------------------------------


class RefitInput(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("vertex_count", C.c_int32), ("vertex_stride_floats", C.c_int32),
                ("normal_offset_floats", C.c_int32), ("vertex_data", C.c_void_p), ("triangle_vertices", C.c_void_p)]


class RefitStats(C.Structure):
    _fields_ = [("sah_cost", C.c_double), ("exact_div_ok", C.c_int32), ("reserved", C.c_int32)]

    def as_dict(self) -> dict:
        return {"sah_cost": float(self.sah_cost), "exact_div_ok": int(self.exact_div_ok)}


REFIT_SYMBOLS = [
    ("shray_scene_refit", C.c_int, [C.c_void_p, C.POINTER(RefitInput), C.POINTER(RefitStats)]),
    ("shray_scene_refit_device", C.c_int, [C.c_void_p, C.POINTER(RefitInput), C.POINTER(RefitStats), C.c_void_p]),
    ("shray_scene_geometry_download", C.c_int, [C.c_void_p, c_float_p, c_float_p, c_float_p, c_float_p]),
    ("shray_scene_geometry_counts", C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
]

# include/shader_ray_instance.h ---------------------------------------------------------------------------
INSTANCE_MAX = 1 << 20


class Instance(C.Structure):
    """shray_instance: a resident scene and its row-major 3 x 4 object-to-world map."""
    _fields_ = [("scene", C.c_void_p), ("object_to_world", C.c_float * 12)]


INSTANCE_SYMBOLS = [
    ("shray_instance_set_create", C.c_int, [C.POINTER(Instance), C.c_int32, C.POINTER(C.c_void_p)]),
    ("shray_instance_set_update", C.c_int, [C.c_void_p, c_float_p]),
    ("shray_instance_set_destroy", None, [C.c_void_p]),
    ("shray_instance_set_count", C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    ("shray_instance_set_world_to_object", C.c_int, [C.c_void_p, c_float_p]),
    ("shray_instance_set_update_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("shray_instance_set_update_status", C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    ("shray_trace_instances_device", C.c_int, [C.c_void_p, C.POINTER(QueryParams), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                               C.c_void_p]),
    ("shray_trace_instances", C.c_int, [C.c_void_p, C.POINTER(QueryParams), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    ("shray_trace_instances_counters", C.c_int, [C.c_void_p, C.POINTER(QueryParams), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                                 C.POINTER(Counters)]),
]
# exported for the tests, not in the header: the set's top-level nodes and records as the next query reads them
INSTANCE_INTERNAL_SYMBOLS = [
    ("shrayi_instance_set_arrays", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]),
]

# include/shader_ray_point.h ------------------------------------------------------------------------------
REGION_A, REGION_B, REGION_C, REGION_AB, REGION_AC, REGION_BC, REGION_FACE, REGION_NONE = 0, 1, 2, 3, 4, 5, 6, -1
POINT_MAX_HEIGHT = 128


class Point(C.Structure):
    """shray_point: an object-space point and its squared search radius (16 bytes)."""
    _fields_ = [("p", C.c_float * 3), ("max_dist2", C.c_float)]


class Closest(C.Structure):
    """shray_closest: the nearest surface point, its squared distance, the weights of corners b and c, the triangle
    (HIT_MISS or the scene's triangle index) and the region (REGION_*) (32 bytes)."""
    _fields_ = [("q", C.c_float * 3), ("dist2", C.c_float), ("u", C.c_float), ("v", C.c_float), ("triangle", C.c_int32),
                ("region", C.c_int32)]


POINT_SYMBOLS = [
    ("shray_closest_points_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    ("shray_closest_points", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    ("shray_closest_points_counters", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(Counters)]),
]

# include/shader_ray_sdf.h --------------------------------------------------------------------------------
SIGN_DATA_FLOATS = 21


class SurfaceInfo(C.Structure):
    """shray_surface_info: the welded topology of a scene (56 bytes)."""
    _fields_ = [("vertices", C.c_int64), ("edges", C.c_int64), ("boundary_edges", C.c_int64), ("nonmanifold_edges", C.c_int64),
                ("misoriented_edges", C.c_int64), ("degenerate_triangles", C.c_int64), ("closed", C.c_int32), ("reserved", C.c_int32)]

    def as_dict(self) -> dict:
        return {n: int(getattr(self, n)) for n, _ in self._fields_ if n != "reserved"}


SDF_SYMBOLS = [
    ("shray_signed_distance_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("shray_signed_distance", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    ("shray_scene_surface_info", C.c_int, [C.c_void_p, C.POINTER(SurfaceInfo)]),
    ("shray_scene_sign_data_download", C.c_int, [C.c_void_p, C.c_void_p]),
]

# include/shader_ray_winding.h -----------------------------------------------------------------------------
WINDING_DATA_FLOATS = 20

WINDING_SYMBOLS = [
    ("shray_winding_number_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_void_p, C.c_void_p]),
    ("shray_winding_number", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_void_p]),
    ("shray_winding_signed_distance_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_void_p, C.c_void_p,
                                                       C.c_void_p]),
    ("shray_winding_signed_distance", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_void_p, C.c_void_p]),
    ("shray_scene_winding_data_download", C.c_int, [C.c_void_p, C.c_void_p]),
]

# include/shader_ray_multihit.h ----------------------------------------------------------------------------
MULTIHIT_MAX = 64


class MultihitParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("max_hits", C.c_int32), ("max_leaf_tests", C.c_int32), ("reserved", C.c_int32)]


MULTIHIT_SYMBOLS = [
    ("shray_multihit_params_init", None, [C.POINTER(MultihitParams)]),
    ("shray_trace_all_hits_device", C.c_int, [C.c_void_p, C.POINTER(MultihitParams), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                              C.c_void_p]),
    ("shray_trace_all_hits", C.c_int, [C.c_void_p, C.POINTER(MultihitParams), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    ("shray_trace_all_hits_counters", C.c_int, [C.c_void_p, C.POINTER(MultihitParams), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                                C.POINTER(Counters)]),
]

# include/shader_ray_near.h --------------------------------------------------------------------------------
NEAR_MAX = 64


class NearParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("max_near", C.c_int32), ("reserved", C.c_int32 * 2)]


NEAR_SYMBOLS = [
    ("shray_near_params_init", None, [C.POINTER(NearParams)]),
    ("shray_near_triangles_device", C.c_int, [C.c_void_p, C.POINTER(NearParams), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                              C.c_void_p]),
    ("shray_near_triangles", C.c_int, [C.c_void_p, C.POINTER(NearParams), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    ("shray_near_triangles_counters", C.c_int, [C.c_void_p, C.POINTER(NearParams), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                                C.POINTER(Counters)]),
]

# include/shader_ray_overlap.h -----------------------------------------------------------------------------
OVERLAP_MAX = 64
OVERLAP_ANY = 1


class Box(C.Structure):
    """shray_box: an axis-aligned box, lo and hi with a pad after each (32 bytes)."""
    _fields_ = [("lo", C.c_float * 3), ("pad0", C.c_float), ("hi", C.c_float * 3), ("pad1", C.c_float)]


class OverlapParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("max_triangles", C.c_int32), ("flags", C.c_uint32), ("reserved", C.c_int32)]


OVERLAP_SYMBOLS = [
    ("shray_overlap_params_init", None, [C.POINTER(OverlapParams)]),
    ("shray_overlap_triangles_device", C.c_int, [C.c_void_p, C.POINTER(OverlapParams), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                                 C.c_void_p]),
    ("shray_overlap_triangles", C.c_int, [C.c_void_p, C.POINTER(OverlapParams), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    ("shray_overlap_triangles_counters", C.c_int, [C.c_void_p, C.POINTER(OverlapParams), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                                   C.POINTER(Counters)]),
]

# include/shader_ray_intersect.h ---------------------------------------------------------------------------
INTERSECT_MAX = 64
INTERSECT_ANY = 1
INTERSECT_SKIP_SHARED = 2


class Triangle(C.Structure):
    """shray_triangle: three corners with a pad after each (48 bytes)."""
    _fields_ = [("a", C.c_float * 3), ("pad0", C.c_float), ("b", C.c_float * 3), ("pad1", C.c_float), ("c", C.c_float * 3),
                ("pad2", C.c_float)]


class IntersectParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("max_triangles", C.c_int32), ("flags", C.c_uint32), ("reserved", C.c_int32)]


INTERSECT_SYMBOLS = [
    ("shray_intersect_params_init", None, [C.POINTER(IntersectParams)]),
    ("shray_intersect_triangles_device", C.c_int, [C.c_void_p, C.POINTER(IntersectParams), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                                   C.c_void_p]),
    ("shray_intersect_triangles", C.c_int, [C.c_void_p, C.POINTER(IntersectParams), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    ("shray_intersect_triangles_counters", C.c_int, [C.c_void_p, C.POINTER(IntersectParams), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                                     C.POINTER(Counters)]),
    ("shray_intersect_self_device", C.c_int, [C.c_void_p, C.POINTER(IntersectParams), C.c_int64, C.c_int64, C.c_void_p, C.c_void_p,
                                              C.c_void_p]),
    ("shray_intersect_self", C.c_int, [C.c_void_p, C.POINTER(IntersectParams), C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]),
]

# include/shader_ray_clearance.h ---------------------------------------------------------------------------
CLEARANCE_MAX = 64
CLEARANCE_ANY = 1
CLEARANCE_SKIP_SHARED = 2
PAIR_INTERSECTING = 15


class PairDistance(C.Structure):
    """shray_pair_distance: a witness on either triangle, the squared distance, the scene triangle and the feature (48 bytes)."""
    _fields_ = [("on_query", C.c_float * 3), ("dist2", C.c_float), ("on_scene", C.c_float * 3), ("triangle", C.c_int32),
                ("feature", C.c_int32), ("reserved", C.c_int32 * 3)]


class ClearanceParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("max_pairs", C.c_int32), ("flags", C.c_uint32), ("max_dist2", C.c_float)]


CLEARANCE_SYMBOLS = [
    ("shray_clearance_params_init", None, [C.POINTER(ClearanceParams)]),
    ("shray_clearance_triangles_device", C.c_int, [C.c_void_p, C.POINTER(ClearanceParams), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                                   C.c_void_p]),
    ("shray_clearance_triangles", C.c_int, [C.c_void_p, C.POINTER(ClearanceParams), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    ("shray_clearance_triangles_counters", C.c_int, [C.c_void_p, C.POINTER(ClearanceParams), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                                     C.POINTER(Counters)]),
    ("shray_clearance_self_device", C.c_int, [C.c_void_p, C.POINTER(ClearanceParams), C.c_int64, C.c_int64, C.c_void_p, C.c_void_p,
                                              C.c_void_p]),
    ("shray_clearance_self", C.c_int, [C.c_void_p, C.POINTER(ClearanceParams), C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]),
]

# include/shader_ray_instance_multihit.h -------------------------------------------------------------------
INSTANCE_MULTIHIT_SYMBOLS = [
    ("shray_trace_instances_all_hits_device", C.c_int, [C.c_void_p, C.POINTER(MultihitParams), C.c_void_p, C.c_int64, C.c_void_p,
                                                        C.c_void_p, C.c_void_p, C.c_void_p]),
    ("shray_trace_instances_all_hits", C.c_int, [C.c_void_p, C.POINTER(MultihitParams), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                                 C.c_void_p]),
    ("shray_trace_instances_all_hits_counters", C.c_int, [C.c_void_p, C.POINTER(MultihitParams), C.c_void_p, C.c_int64, C.c_void_p,
                                                          C.c_void_p, C.c_void_p, C.POINTER(Counters)]),
]

# include/shader_ray_instance_point.h ----------------------------------------------------------------------
INSTANCE_POINT_SYMBOLS = [
    ("shray_closest_points_instances_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("shray_closest_points_instances", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    ("shray_closest_points_instances_counters", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                                          C.POINTER(Counters)]),
]

# include/shader_ray_instance_near.h -----------------------------------------------------------------------
INSTANCE_NEAR_SYMBOLS = [
    ("shray_near_triangles_instances_device", C.c_int, [C.c_void_p, C.POINTER(NearParams), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                                        C.c_void_p, C.c_void_p]),
    ("shray_near_triangles_instances", C.c_int, [C.c_void_p, C.POINTER(NearParams), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                                 C.c_void_p]),
    ("shray_near_triangles_instances_counters", C.c_int, [C.c_void_p, C.POINTER(NearParams), C.c_void_p, C.c_int64, C.c_void_p,
                                                          C.c_void_p, C.c_void_p, C.POINTER(Counters)]),
]

# include/shader_ray_instance_overlap.h --------------------------------------------------------------------
INSTANCE_OVERLAP_SYMBOLS = [
    ("shray_overlap_triangles_instances_device", C.c_int, [C.c_void_p, C.POINTER(OverlapParams), C.c_void_p, C.c_int64, C.c_void_p,
                                                           C.c_void_p, C.c_void_p, C.c_void_p]),
    ("shray_overlap_triangles_instances", C.c_int, [C.c_void_p, C.POINTER(OverlapParams), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                                    C.c_void_p]),
    ("shray_overlap_triangles_instances_counters", C.c_int, [C.c_void_p, C.POINTER(OverlapParams), C.c_void_p, C.c_int64, C.c_void_p,
                                                             C.c_void_p, C.c_void_p, C.POINTER(Counters)]),
]

# include/shader_ray_instance_intersect.h ------------------------------------------------------------------
INTERSECT_SKIP_OWN_INSTANCE = 4   # the instance form only

INSTANCE_INTERSECT_SYMBOLS = [
    ("shray_intersect_triangles_instances_device", C.c_int, [C.c_void_p, C.POINTER(IntersectParams), C.c_void_p, C.c_int64, C.c_void_p,
                                                             C.c_void_p, C.c_void_p, C.c_void_p]),
    ("shray_intersect_triangles_instances", C.c_int, [C.c_void_p, C.POINTER(IntersectParams), C.c_void_p, C.c_int64, C.c_void_p,
                                                      C.c_void_p, C.c_void_p]),
    ("shray_intersect_triangles_instances_counters", C.c_int, [C.c_void_p, C.POINTER(IntersectParams), C.c_void_p, C.c_int64, C.c_void_p,
                                                               C.c_void_p, C.c_void_p, C.POINTER(Counters)]),
    ("shray_intersect_instance_device", C.c_int, [C.c_void_p, C.POINTER(IntersectParams), C.c_int32, C.c_int64, C.c_int64, C.c_void_p,
                                                  C.c_void_p, C.c_void_p, C.c_void_p]),
    ("shray_intersect_instance", C.c_int, [C.c_void_p, C.POINTER(IntersectParams), C.c_int32, C.c_int64, C.c_int64, C.c_void_p,
                                           C.c_void_p, C.c_void_p]),
]

# include/shader_ray_instance_clearance.h ------------------------------------------------------------------
CLEARANCE_SKIP_OWN_INSTANCE = 4   # the instance form only

INSTANCE_CLEARANCE_SYMBOLS = [
    ("shray_clearance_triangles_instances_device", C.c_int, [C.c_void_p, C.POINTER(ClearanceParams), C.c_void_p, C.c_int64, C.c_void_p,
                                                             C.c_void_p, C.c_void_p, C.c_void_p]),
    ("shray_clearance_triangles_instances", C.c_int, [C.c_void_p, C.POINTER(ClearanceParams), C.c_void_p, C.c_int64, C.c_void_p,
                                                      C.c_void_p, C.c_void_p]),
    ("shray_clearance_triangles_instances_counters", C.c_int, [C.c_void_p, C.POINTER(ClearanceParams), C.c_void_p, C.c_int64, C.c_void_p,
                                                               C.c_void_p, C.c_void_p, C.POINTER(Counters)]),
    ("shray_clearance_instance_device", C.c_int, [C.c_void_p, C.POINTER(ClearanceParams), C.c_int32, C.c_int64, C.c_int64, C.c_void_p,
                                                  C.c_void_p, C.c_void_p, C.c_void_p]),
    ("shray_clearance_instance", C.c_int, [C.c_void_p, C.POINTER(ClearanceParams), C.c_int32, C.c_int64, C.c_int64, C.c_void_p,
                                           C.c_void_p, C.c_void_p]),
]

# include/shader_ray_instance_pairs.h ----------------------------------------------------------------------
PAIRS_ANY = 1
PAIRS_SKIP_SHARED = 2
PAIRS_UPPER = 4
PAIRS_NONE = 0xFFFFFFFFFFFFFFFF
PAIRS_MAX_WORKGROUPS = 1 << 24


class PairsParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("first_row", C.c_int32), ("row_count", C.c_int32)]


INSTANCE_PAIRS_SYMBOLS = [
    ("shray_instance_pairs_intersect_device", C.c_int, [C.c_void_p, C.POINTER(PairsParams), C.c_void_p, C.c_void_p, C.c_void_p]),
    ("shray_instance_pairs_intersect", C.c_int, [C.c_void_p, C.POINTER(PairsParams), C.c_void_p, C.c_void_p]),
    ("shray_instance_pairs_intersect_counters", C.c_int, [C.c_void_p, C.POINTER(PairsParams), C.c_void_p, C.c_void_p,
                                                          C.POINTER(Counters)]),
]

# include/shader_ray_instance_sdf.h ------------------------------------------------------------------------
INSTANCE_SDF_SYMBOLS = [
    ("shray_signed_distance_instances_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                                         C.c_void_p]),
    ("shray_signed_distance_instances", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("shray_signed_distance_instances_counters", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                                           C.POINTER(Counters)]),
]

# include/shader_ray_instance_winding.h --------------------------------------------------------------------
INSTANCE_WINDING_SYMBOLS = [
    ("shray_winding_number_instances_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_void_p, C.c_void_p,
                                                        C.c_void_p]),
    ("shray_winding_number_instances", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_void_p, C.c_void_p]),
    ("shray_winding_signed_distance_instances_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_void_p, C.c_void_p,
                                                                 C.c_void_p, C.c_void_p]),
    ("shray_winding_signed_distance_instances", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_void_p, C.c_void_p,
                                                          C.c_void_p]),
    ("shray_instance_set_orientations", C.c_int, [C.c_void_p, C.c_void_p]),
]

_host = None
_hip = None
_clients = {}   # path -> the loaded client library of libshray_hip.so


def _bind(lib, table):
    for name, restype, argtypes in table:
        fn = getattr(lib, name)          # AttributeError here = header/library mismatch
        fn.restype = restype
        fn.argtypes = argtypes
    return lib


def load_host():
    global _host
    if _host is None:
        if not os.path.exists(HOST_LIB):
            raise RuntimeError(f"{HOST_LIB} is not built; run `python __graft_entry__.py build` (or `make -C shader-ray_amd`)")
        _host = _bind(C.CDLL(HOST_LIB), HOST_SYMBOLS)
    return _host


def load_hip():
    """Loads the HIP layer.  torch (when installed) is imported first so that both share
    one HIP runtime: torch bundles its own libamdhip64 under the same SONAME."""
    global _hip
    if _hip is None:
        if not os.path.exists(HIP_LIB):
            raise RuntimeError(f"{HIP_LIB} is not built; run `python __graft_entry__.py build` (or `make -C shader-ray_amd`). "
                               "There is no CPU fallback for the tracer.")
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        _hip = _bind(C.CDLL(HIP_LIB), HIP_SYMBOLS)
        if _hip.shray_abi_version() != ABI_VERSION:
            raise RuntimeError(f"libshray_hip.so reports ABI version {_hip.shray_abi_version()}, these bindings mirror "
                               f"version {ABI_VERSION} of include/shader_ray_hip.h: rebuild the library")
    return _hip


def _load_client(path, symbols):
    """Loads a library that is a client of libshray_hip.so: the HIP layer first (torch, then it: one HIP runtime), then the
    library."""
    if path not in _clients:
        load_hip()
        if not os.path.exists(path):
            raise RuntimeError(f"{path} is not built; run `python __graft_entry__.py build` (or `make -C shader-ray_amd`)")
        _clients[path] = _bind(C.CDLL(path), symbols)
    return _clients[path]


# The client libraries of libshray_hip.so in the order load_all loads them: (name, path, symbols, what it is).  Each has a loader
# of its own, load_<name>(); all but the first report their errors through shray_last_error.  The instanced ones depend on
# libshray_instance.so too, the instanced signed-distance and winding-number ones also on libshray_instance_point.so and on
# libshray_sdf.so / libshray_winding.so.
CLIENT_LIBRARIES = (
    ("dist", DIST_LIB, DIST_SYMBOLS, "the multi-GPU frame loop (depends on RCCL too; torch bundles it)"),
    ("query", QUERY_LIB, QUERY_SYMBOLS, "the ray-query library"),
    ("refit", REFIT_LIB, REFIT_SYMBOLS, "the refit library"),
    ("instance", INSTANCE_LIB, INSTANCE_SYMBOLS + INSTANCE_INTERNAL_SYMBOLS, "the instanced-query library, with its test accessor"),
    ("point", POINT_LIB, POINT_SYMBOLS, "the closest-point library"),
    ("sdf", SDF_LIB, SDF_SYMBOLS, "the signed-distance library"),
    ("winding", WINDING_LIB, WINDING_SYMBOLS, "the winding-number library"),
    ("multihit", MULTIHIT_LIB, MULTIHIT_SYMBOLS, "the all-hits ray-query library"),
    ("near", NEAR_LIB, NEAR_SYMBOLS, "the within-radius query library"),
    ("overlap", OVERLAP_LIB, OVERLAP_SYMBOLS, "the box-overlap query library"),
    ("intersect", INTERSECT_LIB, INTERSECT_SYMBOLS, "the triangle-intersection query library"),
    ("clearance", CLEARANCE_LIB, CLEARANCE_SYMBOLS, "the triangle-distance query library"),
    ("instance_multihit", INSTANCE_MULTIHIT_LIB, INSTANCE_MULTIHIT_SYMBOLS, "the instanced all-hits library"),
    ("instance_point", INSTANCE_POINT_LIB, INSTANCE_POINT_SYMBOLS, "the instanced closest-point library"),
    ("instance_near", INSTANCE_NEAR_LIB, INSTANCE_NEAR_SYMBOLS, "the instanced within-radius library"),
    ("instance_overlap", INSTANCE_OVERLAP_LIB, INSTANCE_OVERLAP_SYMBOLS, "the instanced box-overlap library"),
    ("instance_intersect", INSTANCE_INTERSECT_LIB, INSTANCE_INTERSECT_SYMBOLS, "the instanced triangle-intersection library"),
    ("instance_clearance", INSTANCE_CLEARANCE_LIB, INSTANCE_CLEARANCE_SYMBOLS, "the instanced triangle-distance library"),
    ("instance_pairs", INSTANCE_PAIRS_LIB, INSTANCE_PAIRS_SYMBOLS, "the instance-pair collision-matrix library"),
    ("instance_sdf", INSTANCE_SDF_LIB, INSTANCE_SDF_SYMBOLS, "the instanced signed-distance library"),
    ("instance_winding", INSTANCE_WINDING_LIB, INSTANCE_WINDING_SYMBOLS, "the instanced winding-number library"),
)


def _loader(name, path, symbols, what):
    def load():
        return _load_client(path, symbols)
    load.__name__ = load.__qualname__ = f"load_{name}"
    load.__doc__ = f"Loads {what} ({os.path.basename(path)})."
    return load


for _entry in CLIENT_LIBRARIES:   # load_dist(), load_query(), ..., load_instance_winding()
    globals()[f"load_{_entry[0]}"] = _loader(*_entry)
del _entry


def load_all():
    """Loads the host library, the HIP layer and every client library, so a missing or mismatched one raises here."""
    load_host()
    load_hip()
    for name, *_ in CLIENT_LIBRARIES:
        globals()[f"load_{name}"]()


def check_dist(code: int):
    if code != 0:
        msg = load_dist().shray_dist_last_error()
        raise ShrayError(code, msg.decode() if msg else "")


class ShrayError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"shray error {code}: {message}")
        self.code = code


def check(code: int):
    if code != 0:
        msg = load_hip().shray_last_error()
        raise ShrayError(code, msg.decode() if msg else "")
