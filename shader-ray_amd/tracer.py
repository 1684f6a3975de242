"""Python face of the HIP layer (include/shader_ray_hip.h): upload a flattened scene and
an environment, render frames.  Device memory and streams are plumbing (torch tensors
/ the current torch stream when torch is used); every pixel is produced by the gfx950
kernels behind the C ABI.  There is no CPU fallback."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from . import _native as N

KERNEL_STACK = 0      # per-ray LDS stack over the packed BVH (default)
KERNEL_THREADED = 1   # literal hit/miss-table traversal over the reference arrays


class Scene:
    """One scene resident on one GPU (replaces the reference's texture upload,
    ray.cpp:470-510)."""

    def __init__(self, desc: N.SceneDesc, environment: np.ndarray | None = None, device: int | None = None):
        self._lib = N.load_hip()
        if device is not None:
            N.check(self._lib.shray_set_device(device))
        handle = C.c_void_p()
        N.check(self._lib.shray_scene_create(C.byref(desc), C.byref(handle)))
        self._handle = handle
        if environment is not None:
            self.set_environment(environment)

    @classmethod
    def from_device(cls, tree_handle, flat_handle, environment: np.ndarray | None = None):
        """A scene from a tree that never left the device (shray_scene_create_from_device): `tree_handle` from
        shray_bvh_build_device, `flat_handle` from shray_flatten_device_tree (both may be destroyed afterwards)."""
        self = cls.__new__(cls)
        self._lib = N.load_hip()
        handle = C.c_void_p()
        N.check(self._lib.shray_scene_create_from_device(tree_handle, flat_handle, C.byref(handle)))
        self._handle = handle
        if environment is not None:
            self.set_environment(environment)
        return self

    def derived_arrays(self) -> dict:
        """What scene creation derived, read back (tests): packed_nodes uint32 [8, nodes, 8], packed_tris uint32 [triangles, 9],
        normals16 uint16 [corners * 3], pair_nodes uint32 [nodes, 16], stack_levels."""
        a, b, c, d, levels = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_int32()
        N.check(self._lib.shray_scene_derived_sizes(self._handle, C.byref(a), C.byref(b), C.byref(c), C.byref(d), C.byref(levels)))
        nodes, tris = np.zeros(a.value // 4, np.uint32), np.zeros(b.value // 4, np.uint32)
        halves, pairs = np.zeros(c.value // 2, np.uint16), np.zeros(d.value // 4, np.uint32)
        N.check(self._lib.shray_scene_derived_download(self._handle, nodes.ctypes.data_as(C.c_void_p), tris.ctypes.data_as(C.c_void_p),
                                                       halves.ctypes.data_as(C.c_void_p), pairs.ctypes.data_as(C.c_void_p)))
        return {"packed_nodes": nodes.reshape(8, -1, 8), "packed_tris": tris.reshape(-1, 9), "normals16": halves,
                "pair_nodes": pairs.reshape(-1, 16), "stack_levels": levels.value}

    def close(self):
        if getattr(self, "_handle", None):
            self._lib.shray_scene_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_environment(self, rgb: np.ndarray, storage: int = N.ENV_FLOAT32):
        """`rgb` is [height, width, 3] float32, row 0 = straight down (texture t = 0).  storage = ENV_UNORM8 keeps
        it the way most drivers keep the reference's unsized GL_RGB upload (ray.cpp:508): 8 bits, clamped to [0, 1]."""
        rgb = np.ascontiguousarray(rgb, dtype=np.float32)
        h, w, c = rgb.shape
        assert c == 3
        N.check(self._lib.shray_scene_set_environment_storage(self._handle, rgb.ctypes.data_as(N.c_float_p), w, h, storage))

    def set_kernel(self, kernel_id: int):
        N.check(self._lib.shray_scene_set_kernel(self._handle, kernel_id))

    def render(self, params: N.FrameParams, width: int, height: int, spp: int = 1, out: np.ndarray | None = None) -> np.ndarray:
        """Blocking render to host memory: RGBA float32 [height, width, 4], row 0 = bottom.  `out`: a C-contiguous
        float32 array of that shape to fill (a frame loop reuses one: a fresh 33 MB array costs its page faults)."""
        if out is None:
            out = np.empty((height, width, 4), dtype=np.float32)
        elif out.shape != (height, width, 4) or out.dtype != np.float32 or not out.flags.c_contiguous:
            raise ValueError("out must be a C-contiguous float32 array of shape (height, width, 4)")
        N.check(self._lib.shray_render(self._handle, C.byref(params), width, height, spp,
                                       out.ctypes.data_as(N.c_float_p)))
        return out

    def render_to_pinned(self, params: N.FrameParams, width: int, height: int, spp: int, pinned: "PinnedFrame",
                         stream_ptr: int = 0, wait: bool = True):
        """Render + DMA into pinned host memory on a HIP stream (shray_render_host_async).  With wait=False
        the caller synchronises the stream before reading `pinned.array`."""
        N.check(self._lib.shray_render_host_async(self._handle, C.byref(params), width, height, spp, C.c_void_p(pinned.ptr), _ptr(stream_ptr)))
        if wait:
            import torch
            torch.cuda.synchronize()
        return pinned.array

    def render_counters(self, params: N.FrameParams, width: int, height: int, spp: int = 1, want_image: bool = True):
        out = np.empty((height, width, 4), dtype=np.float32) if want_image else None
        counters = N.Counters()
        N.check(self._lib.shray_render_counters(
            self._handle, C.byref(params), width, height, spp,
            out.ctypes.data_as(N.c_float_p) if want_image else None, C.byref(counters)))
        return out, counters.as_dict()

    def render_counters_timed(self, params: N.FrameParams, width: int, height: int, spp: int = 1, frames_per_launch: int = 1,
                              want_image: bool = True):
        """Tallies of the instance the timed launches run (shadow rays stop at their first hit, samples in neighbouring
        lanes): shray_render_counters_timed."""
        out = np.empty((height, width, 4), dtype=np.float32) if want_image else None
        counters = N.Counters()
        N.check(self._lib.shray_render_counters_timed(
            self._handle, C.byref(params), width, height, spp, frames_per_launch,
            out.ctypes.data_as(N.c_float_p) if want_image else None, C.byref(counters)))
        return out, counters.as_dict()

    def dispatch_order(self) -> np.ndarray:
        """The patch permutation the next batch launch of the current shape would read (shray_scene_dispatch_order);
        empty while the identity is in use."""
        n = C.c_uint32(0)
        N.check(self._lib.shray_scene_dispatch_order(self._handle, None, 0, C.byref(n)))
        out = np.empty(n.value, dtype=np.uint32)
        if n.value:
            N.check(self._lib.shray_scene_dispatch_order(self._handle, out.ctypes.data_as(C.POINTER(C.c_uint32)), n.value, C.byref(n)))
        return out

    def set_view_cache(self, on: bool):
        """Turns the scene's view cache on or off (shray_scene_set_view_cache); off drops its entries."""
        N.check(self._lib.shray_scene_set_view_cache(self._handle, 1 if on else 0))

    def view_cache_stats(self) -> dict:
        """{"entries_built", "launches_cached", "bytes_held"} of the scene's view cache (shray_scene_view_cache_stats)."""
        built, cached, held = C.c_uint64(), C.c_uint64(), C.c_uint64()
        N.check(self._lib.shray_scene_view_cache_stats(self._handle, C.byref(built), C.byref(cached), C.byref(held)))
        return {"entries_built": built.value, "launches_cached": cached.value, "bytes_held": held.value}

    def render_into(self, params: N.FrameParams, width: int, height: int, spp: int, out_ptr: int,
                    stream_ptr: int = 0, tiles: N.TileSet | None = None):
        """Asynchronous render into device memory (`out_ptr`, e.g. tensor.data_ptr()) on a
        HIP stream (`stream_ptr`, e.g. torch.cuda.current_stream().cuda_stream)."""
        N.check(self._lib.shray_render_device(
            self._handle, C.byref(params), width, height, spp, C.byref(tiles) if tiles is not None else None, _ptr(out_ptr), _ptr(stream_ptr)))

    def trace_rays(self, rays, tmax=None, any_hit: bool = False, max_bvh_iterations: int = 400, max_leaf_tests: int = 10,
                   counters: bool = False):
        """Ray queries from host memory (shray_trace_rays, blocking).  `rays`: a RAY_DTYPE array, or [n, 6] / [n, 8] float32
        (origin, direction / the shray_ray layout); `tmax` (scalar or [n]) replaces the rays' own.  Returns a HIT_DTYPE array,
        and with counters=True also the walk's counters (shray_trace_rays_counters)."""
        rays = _host_rays(rays, tmax)
        qp = query_params(any_hit, max_bvh_iterations, max_leaf_tests)
        lib = N.load_query()
        out = _blocking(self._handle, lib.shray_trace_rays, lib.shray_trace_rays_counters, (C.byref(qp),), rays, (),
                        [_out(True, HIT_DTYPE, 4)], counters)
        return out if counters else out[0]

    def _items(self, kind: str, value=None):
        """_per_item's converters of an items argument of `kind`, for the scene's device"""
        return _converters(kind, self.device_index, "the scene", value)

    def trace_rays_into(self, rays_ptr: int, count: int, hits_ptr: int, stream_ptr: int = 0, any_hit: bool = False,
                        max_bvh_iterations: int = 400, max_leaf_tests: int = 10):
        """Asynchronous ray queries on device memory (shray_trace_rays_device): `count` shray_ray records at `rays_ptr`
        (e.g. a float32 [n, 8] tensor's data_ptr()) -> `count` shray_hit records at `hits_ptr` (e.g. [n, 4] float32 / int32),
        on a HIP stream (`stream_ptr`, e.g. torch.cuda.current_stream().cuda_stream)."""
        qp = query_params(any_hit, max_bvh_iterations, max_leaf_tests)
        N.check(N.load_query().shray_trace_rays_device(self._handle, C.byref(qp), _ptr(rays_ptr), count, _ptr(hits_ptr), _ptr(stream_ptr)))

    def closest_points(self, points, max_dist2=None, counters: bool = False):
        """Closest-point queries (include/shader_ray_point.h): the nearest point of the surface to each point.  `points`: a
        POINT_DTYPE array or [n, 3] / [n, 4] float32 (p / the shray_point layout), numpy (the blocking host path,
        shray_closest_points) or a float32 [n, 3] / [n, 4] GPU tensor on the scene's device (shray_closest_points_device, enqueued on the
        current torch stream); `max_dist2` (scalar or [n]) replaces the points' own (default for [n, 3]: +inf, no limit).  Returns
        a CLOSEST_DTYPE array for host points, an int32 [n, 8] tensor of shray_closest records (view it as float32 for q, dist2,
        u, v) for GPU points; with counters=True (host points only) also the walk's counters (shray_closest_points_counters)."""
        lib = N.load_point()
        out = _per_item(self._handle, (lib.shray_closest_points_device, lib.shray_closest_points, lib.shray_closest_points_counters), (),
                        points, self._items("points", max_dist2), (), [_out(True, CLOSEST_DTYPE, 8)], counters)
        return out if counters else out[0]

    def closest_points_into(self, points_ptr: int, count: int, out_ptr: int, stream_ptr: int = 0):
        """Asynchronous closest-point queries on device memory of the scene's device (shray_closest_points_device): `count`
        shray_point records at `points_ptr` (e.g. a float32 [n, 4] tensor's data_ptr()) -> `count` shray_closest records at
        `out_ptr` (e.g. [n, 8] int32 / float32), on a HIP stream (`stream_ptr`, e.g. torch.cuda.current_stream().cuda_stream)."""
        N.check(N.load_point().shray_closest_points_device(self._handle, _ptr(points_ptr), count, _ptr(out_ptr), _ptr(stream_ptr)))

    def signed_distance(self, points, max_dist2=None, closest: bool = False):
        """Signed distances to the surface (include/shader_ray_sdf.h): negative inside a closed, outward-wound mesh, NaN for a
        point with no triangle within its radius.  `points` and `max_dist2` as for closest_points: numpy (the blocking host path,
        shray_signed_distance) or a GPU tensor on the scene's device (shray_signed_distance_device, enqueued on the current torch
        stream).  Returns float32 [n] of the same kind; with closest=True also the closest-point records (a CLOSEST_DTYPE array,
        or an int32 [n, 8] tensor)."""
        lib = N.load_sdf()
        out = _per_item(self._handle, (lib.shray_signed_distance_device, lib.shray_signed_distance, None), (), points,
                        self._items("points", max_dist2), (), [_out(True, np.float32), _out(closest, CLOSEST_DTYPE, 8)])
        return out if closest else out[0]

    def signed_distance_into(self, points_ptr: int, count: int, out_ptr: int, closest_ptr: int = 0, stream_ptr: int = 0):
        """Asynchronous signed distance queries on device memory of the scene's device (shray_signed_distance_device): `count`
        shray_point records at `points_ptr` -> `count` float32 at `out_ptr` and, unless `closest_ptr` is 0, `count`
        shray_closest records there, on a HIP stream (`stream_ptr`, e.g. torch.cuda.current_stream().cuda_stream)."""
        N.check(N.load_sdf().shray_signed_distance_device(self._handle, _ptr(points_ptr), count, _ptr(out_ptr), _ptr(closest_ptr), _ptr(stream_ptr)))

    def surface_info(self) -> dict:
        """The welded topology (shray_scene_surface_info): vertices, edges, boundary_edges, nonmanifold_edges,
        misoriented_edges, degenerate_triangles, closed."""
        info = N.SurfaceInfo()
        N.check(N.load_sdf().shray_scene_surface_info(self._handle, C.byref(info)))
        return info.as_dict()

    def sign_data(self) -> np.ndarray:
        """The derived sign data (shray_scene_sign_data_download): float32 [triangles, 7, 3]: nhat, the pseudonormals of the
        vertices of corners a, b, c, and of the edges AB, AC, BC."""
        corners = C.c_int32()
        N.check(N.load_refit().shray_scene_geometry_counts(self._handle, C.byref(corners), None))
        out = np.zeros((corners.value // 3, 7, 3), np.float32)
        N.check(N.load_sdf().shray_scene_sign_data_download(self._handle, out.ctypes.data_as(C.c_void_p)))
        return out

    def winding_number(self, points, beta: float = 2.0):
        """Generalized winding numbers (include/shader_ray_winding.h): about 1 inside a closed outward-wound mesh and 0 outside,
        robust on open and self-intersecting meshes; NaN for a point with a non-finite coordinate.  `points` as for
        closest_points (a point's max_dist2 is ignored): numpy (the blocking host path, shray_winding_number) or a GPU tensor on
        the scene's device (shray_winding_number_device, on the current torch stream).  `beta`: the far-field accuracy
        parameter, float('inf') for the exact sum over every triangle.  Returns float32 [n] of the same kind."""
        lib = N.load_winding()
        return _per_item(self._handle, (lib.shray_winding_number_device, lib.shray_winding_number, None), (), points, self._items("points"),
                         (beta,), [_out(True, np.float32)])[0]

    def winding_number_into(self, points_ptr: int, count: int, out_ptr: int, beta: float = 2.0, stream_ptr: int = 0):
        """Asynchronous winding numbers on device memory of the scene's device (shray_winding_number_device): `count`
        shray_point records at `points_ptr` -> `count` float32 at `out_ptr`, on a HIP stream (`stream_ptr`)."""
        N.check(N.load_winding().shray_winding_number_device(self._handle, _ptr(points_ptr), count, beta, _ptr(out_ptr), _ptr(stream_ptr)))

    def winding_signed_distance(self, points, max_dist2=None, beta: float = 2.0, closest: bool = False):
        """Signed distances whose sign comes from the winding number (shray_winding_signed_distance): negative where w > 0.5,
        NaN for a point with no triangle within its radius.  Arguments and results as for signed_distance."""
        lib = N.load_winding()
        out = _per_item(self._handle, (lib.shray_winding_signed_distance_device, lib.shray_winding_signed_distance, None), (), points,
                        self._items("points", max_dist2), (beta,), [_out(True, np.float32), _out(closest, CLOSEST_DTYPE, 8)])
        return out if closest else out[0]

    def winding_signed_distance_into(self, points_ptr: int, count: int, out_ptr: int, closest_ptr: int = 0, beta: float = 2.0,
                                     stream_ptr: int = 0):
        """Asynchronous winding-signed distances on device memory (shray_winding_signed_distance_device), as
        signed_distance_into."""
        N.check(N.load_winding().shray_winding_signed_distance_device(self._handle, _ptr(points_ptr), count, beta, _ptr(out_ptr), _ptr(closest_ptr),
                                                                      _ptr(stream_ptr)))

    def winding_data(self) -> np.ndarray:
        """The derived node records (shray_scene_winding_data_download): float32 [nodes, 20] in packed pre-order: P, r, N, A,
        M row-major, three zeros."""
        nodes = C.c_int32()
        N.check(N.load_refit().shray_scene_geometry_counts(self._handle, None, C.byref(nodes)))
        out = np.zeros((nodes.value, N.WINDING_DATA_FLOATS), np.float32)
        N.check(N.load_winding().shray_scene_winding_data_download(self._handle, out.ctypes.data_as(C.c_void_p)))
        return out

    def trace_all_hits(self, rays, max_hits: int = 8, counts: bool = True, max_leaf_tests: int = 10, counters: bool = False):
        """All-hits ray queries (include/shader_ray_multihit.h): per ray the number of surfaces it crosses and its first
        `max_hits` crossings, sorted by (t, triangle), the other slots {tmax, 0, 0, HIT_MISS}.  `rays` as for trace_rays: a
        RAY_DTYPE array or [n, 6] / [n, 8] float32 takes the blocking host path (shray_trace_all_hits) and returns
        (hits: HIT_DTYPE [n, max_hits], counts: int32 [n]); a float32 [n, 8] GPU tensor on the scene's device takes the device
        path (shray_trace_all_hits_device) on the current torch stream and returns (int32 [n, max_hits, 4] tensor of shray_hit
        records, int32 [n] tensor).  counts=False returns None for the counts and lets the walk skip what cannot reach the
        first `max_hits` (the same records); max_hits = 0 returns None for the hits.  counters=True (host rays only) also
        returns the counters of the walk that skips nothing (shray_trace_all_hits_counters)."""
        lib = N.load_multihit()
        return _first_k(self._handle, (lib.shray_trace_all_hits_device, lib.shray_trace_all_hits, lib.shray_trace_all_hits_counters),
                        multihit_params(max_hits, max_leaf_tests), max_hits, "max_hits", rays, self._items("rays"), HIT_DTYPE, (4,), False,
                        counts, counters)

    def trace_all_hits_into(self, rays_ptr: int, count: int, hits_ptr: int, counts_ptr: int = 0, max_hits: int = 8, stream_ptr: int = 0,
                            max_leaf_tests: int = 10):
        """Asynchronous all-hits queries on device memory of the scene's device (shray_trace_all_hits_device): `count`
        shray_ray records at `rays_ptr` -> count * max_hits shray_hit records at `hits_ptr` (0 iff max_hits is 0) and, unless
        `counts_ptr` is 0, `count` int32 crossing counts there, on a HIP stream (`stream_ptr`)."""
        mp = multihit_params(max_hits, max_leaf_tests)
        N.check(N.load_multihit().shray_trace_all_hits_device(self._handle, C.byref(mp), _ptr(rays_ptr), count, _ptr(hits_ptr), _ptr(counts_ptr),
                                                              _ptr(stream_ptr)))

    def crossing_counts(self, rays, max_leaf_tests: int = 10):
        """How many surfaces each ray crosses before its tmax (trace_all_hits with max_hits = 0): int32 [n], numpy for host
        rays, a tensor for GPU rays."""
        return self.trace_all_hits(rays, max_hits=0, counts=True, max_leaf_tests=max_leaf_tests)[1]

    def triangles_within(self, points, max_near: int = 8, counts: bool = True, counters: bool = False):
        """Within-radius queries (include/shader_ray_near.h): per point the number of triangles whose closest point lies
        within its max_dist2 and the nearest `max_near` of them as shray_closest records, sorted by (dist2, triangle), the
        other slots miss records.  `points` as for closest_points: a POINT_DTYPE array or [n, 3] / [n, 4] float32 takes the
        blocking host path (shray_near_triangles) and returns (records: CLOSEST_DTYPE [n, max_near], counts: int32 [n]); a
        float32 [n, 3] / [n, 4] GPU tensor on the scene's device takes the device path (shray_near_triangles_device) on the
        current torch stream and returns (int32 [n, max_near, 8] tensor of shray_closest records, int32 [n] tensor).
        counts=False returns None for the counts and lets the walk skip what cannot reach the nearest `max_near` (the same
        records); max_near = 0 returns None for the records.  counters=True (host points only) also returns the counters of
        the walk that prunes only by max_dist2 (shray_near_triangles_counters)."""
        lib = N.load_near()
        return _first_k(self._handle, (lib.shray_near_triangles_device, lib.shray_near_triangles, lib.shray_near_triangles_counters),
                        near_params(max_near), max_near, "max_near", points, self._items("points"), CLOSEST_DTYPE, (8,), False, counts, counters)

    def triangles_within_into(self, points_ptr: int, count: int, out_ptr: int, counts_ptr: int = 0, max_near: int = 8, stream_ptr: int = 0):
        """Asynchronous within-radius queries on device memory of the scene's device (shray_near_triangles_device): `count`
        shray_point records at `points_ptr` -> count * max_near shray_closest records at `out_ptr` (0 iff max_near is 0) and,
        unless `counts_ptr` is 0, `count` int32 near counts there, on a HIP stream (`stream_ptr`)."""
        np_ = near_params(max_near)
        N.check(N.load_near().shray_near_triangles_device(self._handle, C.byref(np_), _ptr(points_ptr), count, _ptr(out_ptr), _ptr(counts_ptr),
                                                          _ptr(stream_ptr)))

    def near_counts(self, points):
        """How many triangles lie within each point's max_dist2 (triangles_within with max_near = 0): int32 [n], numpy for
        host points, a tensor for GPU points."""
        return self.triangles_within(points, max_near=0, counts=True)[1]

    def triangles_in_boxes(self, boxes, max_triangles: int = 8, counts: bool = True, counters: bool = False, any_only: bool = False):
        """Box-overlap queries (include/shader_ray_overlap.h): per axis-aligned box the number of triangles that touch it and
        the `max_triangles` smallest of their indices in ascending order, the other slots SHRAY_HIT_MISS (-1).  `boxes`: a
        BOX_DTYPE array or [n, 6] (lo, hi) / [n, 8] (the shray_box layout) float32 takes the blocking host path
        (shray_overlap_triangles) and returns (indices: int32 [n, max_triangles], counts: int32 [n]); a float32 [n, 6] / [n, 8]
        GPU tensor on the scene's device takes the device path (shray_overlap_triangles_device) on the current torch stream
        and returns tensors of the same shapes.  counts=False returns None for the counts; max_triangles = 0 returns None for
        the indices.  any_only=True (with max_triangles = 0) sets SHRAY_OVERLAP_ANY: the count is 1 or 0 and the walk stops at
        the first touching triangle.  counters=True (host boxes only) also returns the walk's counters
        (shray_overlap_triangles_counters)."""
        lib = N.load_overlap()
        return _first_k(self._handle, (lib.shray_overlap_triangles_device, lib.shray_overlap_triangles, lib.shray_overlap_triangles_counters),
                        overlap_params(max_triangles, any_only), max_triangles, "max_triangles", boxes, self._items("boxes"), np.int32, (), False,
                        counts, counters)

    def triangles_in_boxes_into(self, boxes_ptr: int, count: int, out_ptr: int, counts_ptr: int = 0, max_triangles: int = 8,
                                any_only: bool = False, stream_ptr: int = 0):
        """Asynchronous box-overlap queries on device memory of the scene's device (shray_overlap_triangles_device): `count`
        shray_box records at `boxes_ptr` -> count * max_triangles int32 indices at `out_ptr` (0 iff max_triangles is 0) and,
        unless `counts_ptr` is 0, `count` int32 counts there, on a HIP stream (`stream_ptr`)."""
        op = overlap_params(max_triangles, any_only)
        N.check(N.load_overlap().shray_overlap_triangles_device(self._handle, C.byref(op), _ptr(boxes_ptr), count, _ptr(out_ptr), _ptr(counts_ptr),
                                                                _ptr(stream_ptr)))

    def box_counts(self, boxes):
        """How many triangles touch each box (triangles_in_boxes with max_triangles = 0): int32 [n], numpy for host boxes, a
        tensor for GPU boxes."""
        return self.triangles_in_boxes(boxes, max_triangles=0, counts=True)[1]

    def boxes_touched(self, boxes):
        """Whether any triangle touches each box (SHRAY_OVERLAP_ANY: the walk stops at the first one): bool [n], numpy for
        host boxes, a tensor for GPU boxes."""
        return self.triangles_in_boxes(boxes, max_triangles=0, counts=True, any_only=True)[1] != 0

    def intersecting_triangles(self, triangles, max_triangles: int = 8, counts: bool = True, counters: bool = False, any_only: bool = False,
                               skip_shared: bool = False):
        """Triangle-intersection queries (include/shader_ray_intersect.h): per query triangle the number of scene triangles
        it intersects and the `max_triangles` smallest of their indices in ascending order, the other slots SHRAY_HIT_MISS
        (-1).  `triangles`: a TRIANGLE_DTYPE array or [n, 3, 3] / [n, 9] (a, b, c) / [n, 12] (the shray_triangle layout)
        float32 takes the blocking host path (shray_intersect_triangles) and returns (indices: int32 [n, max_triangles],
        counts: int32 [n]); a float32 [n, 9] / [n, 12] GPU tensor on the scene's device takes the device path
        (shray_intersect_triangles_device) on the current torch stream and returns tensors of the same shapes.  counts=False
        returns None for the counts; max_triangles = 0 returns None for the indices.  any_only=True (with max_triangles = 0)
        sets SHRAY_INTERSECT_ANY: the count is 1 or 0 and the walk stops at the first member.  skip_shared=True sets
        SHRAY_INTERSECT_SKIP_SHARED: a scene triangle with a corner equal to one of the query's is not a member.
        counters=True (host triangles only) also returns the walk's counters (shray_intersect_triangles_counters)."""
        lib = N.load_intersect()
        return _first_k(self._handle, (lib.shray_intersect_triangles_device, lib.shray_intersect_triangles,
                                       lib.shray_intersect_triangles_counters),
                        intersect_params(max_triangles, any_only, skip_shared), max_triangles, "max_triangles", triangles,
                        self._items("triangles"), np.int32, (), False, counts, counters)

    def intersecting_triangles_into(self, triangles_ptr: int, count: int, out_ptr: int, counts_ptr: int = 0, max_triangles: int = 8,
                                    any_only: bool = False, skip_shared: bool = False, stream_ptr: int = 0):
        """Asynchronous triangle-intersection queries on device memory of the scene's device
        (shray_intersect_triangles_device): `count` shray_triangle records at `triangles_ptr` -> count * max_triangles int32
        indices at `out_ptr` (0 iff max_triangles is 0) and, unless `counts_ptr` is 0, `count` int32 counts there, on a HIP
        stream (`stream_ptr`)."""
        op = intersect_params(max_triangles, any_only, skip_shared)
        N.check(N.load_intersect().shray_intersect_triangles_device(self._handle, C.byref(op), _ptr(triangles_ptr), count, _ptr(out_ptr),
                                                                    _ptr(counts_ptr), _ptr(stream_ptr)))

    def intersection_counts(self, triangles, skip_shared: bool = False):
        """How many scene triangles each query triangle intersects (intersecting_triangles with max_triangles = 0): int32 [n],
        numpy for host triangles, a tensor for GPU triangles."""
        return self.intersecting_triangles(triangles, max_triangles=0, counts=True, skip_shared=skip_shared)[1]

    def triangles_intersected(self, triangles, skip_shared: bool = False):
        """Whether each query triangle intersects any scene triangle (SHRAY_INTERSECT_ANY: the walk stops at the first one):
        bool [n], numpy for host triangles, a tensor for GPU triangles."""
        return self.intersecting_triangles(triangles, max_triangles=0, counts=True, any_only=True, skip_shared=skip_shared)[1] != 0

    def triangle_count(self) -> int:
        """The number of triangles of the scene."""
        corners = C.c_int32()
        N.check(N.load_refit().shray_scene_geometry_counts(self._handle, C.byref(corners), None))
        return corners.value // 3

    def self_intersections(self, max_triangles: int = 8, counts: bool = True, any_only: bool = False, skip_shared: bool = True,
                           first: int = 0, count: int | None = None, device: bool = False):
        """The scene's own triangles [first, first + count) as the queries (shray_intersect_self; count=None: up to the last
        one), read from the scene's positions as they are when the query runs.  Returns (indices: int32 [count, max_triangles],
        counts: int32 [count]) as numpy arrays from the blocking form, or with device=True as tensors on the scene's device
        enqueued on the current torch stream (shray_intersect_self_device).  skip_shared defaults to True here: without it
        every triangle finds itself and its neighbours.  max_triangles = 0 returns None for the indices, counts=False None
        for the counts; any_only as for intersecting_triangles."""
        lib = N.load_intersect()
        return _own_triangles(self._handle, (lib.shray_intersect_self_device, lib.shray_intersect_self),
                              intersect_params(max_triangles, any_only, skip_shared), None, first, count, self.triangle_count,
                              max_triangles, "max_triangles", np.int32, (), counts, device, self.device_index)

    def self_intersections_into(self, first: int, count: int, out_ptr: int, counts_ptr: int = 0, max_triangles: int = 8,
                                any_only: bool = False, skip_shared: bool = True, stream_ptr: int = 0):
        """Asynchronous self-intersection queries (shray_intersect_self_device): the scene's triangles [first, first + count)
        -> count * max_triangles int32 indices at `out_ptr` (0 iff max_triangles is 0) and, unless `counts_ptr` is 0, `count`
        int32 counts there, device memory of the scene's device, on a HIP stream (`stream_ptr`)."""
        op = intersect_params(max_triangles, any_only, skip_shared)
        N.check(N.load_intersect().shray_intersect_self_device(self._handle, C.byref(op), first, count, _ptr(out_ptr),
                                                               _ptr(counts_ptr), _ptr(stream_ptr)))

    def is_self_intersecting(self) -> bool:
        """Whether any triangle of the scene intersects one it shares no corner with (SHRAY_INTERSECT_ANY |
        SHRAY_INTERSECT_SKIP_SHARED over every triangle)."""
        return bool(self.self_intersections(max_triangles=0, counts=True, any_only=True, skip_shared=True)[1].any())

    def intersections_with(self, other: "Scene", max_triangles: int = 8, counts: bool = True, any_only: bool = False,
                           skip_shared: bool = False):
        """Mesh against mesh: the queries are the other scene's current triangles (other.geometry(), so after its refits), in
        its triangle order; the blocking host path of intersecting_triangles on this scene."""
        theirs = np.asarray(other.geometry()["vertex_positions"], np.float32).reshape(-1, 9)
        return self.intersecting_triangles(theirs, max_triangles=max_triangles, counts=counts, any_only=any_only, skip_shared=skip_shared)

    def triangle_distances(self, triangles, max_dist2: float = float("inf"), max_pairs: int = 1, counts: bool = True, counters: bool = False,
                           skip_shared: bool = False, any_only: bool = False):
        """Triangle-distance queries (include/shader_ray_clearance.h): per query triangle the number of scene triangles whose
        squared distance to it is at most `max_dist2` and the `max_pairs` nearest of them in (dist2, triangle) order as
        PAIR_DISTANCE_DTYPE records (a witness on either triangle, dist2, the scene triangle and the feature; an
        interpenetrating pair has dist2 0 and feature PAIR_INTERSECTING), the other slots miss records (triangle -1).
        `triangles` as for intersecting_triangles: host triangles take the blocking path (shray_clearance_triangles) and return
        (records: PAIR_DISTANCE_DTYPE [n, max_pairs], counts: int32 [n]); a float32 [n, 9] / [n, 12] GPU tensor on the scene's
        device takes the device path (shray_clearance_triangles_device) on the current torch stream and returns the records
        as an int32 [n, max_pairs, 12] tensor (the 48 bytes of each: view it as float32 for the coordinates) and the counts
        as a tensor.  counts=False returns None for the counts and lets the walk skip what cannot reach the nearest
        `max_pairs`; max_pairs = 0 returns None for the records.  skip_shared=True sets SHRAY_CLEARANCE_SKIP_SHARED, any_only=True
        (with max_pairs = 0) SHRAY_CLEARANCE_ANY.  counters=True (host triangles only) also returns the walk's counters."""
        lib = N.load_clearance()
        return _first_k(self._handle, (lib.shray_clearance_triangles_device, lib.shray_clearance_triangles,
                                       lib.shray_clearance_triangles_counters),
                        clearance_params(max_pairs, max_dist2, any_only, skip_shared), max_pairs, "max_pairs", triangles,
                        self._items("triangles"), PAIR_DISTANCE_DTYPE, (12,), False, counts, counters)

    def triangle_distances_into(self, triangles_ptr: int, count: int, out_ptr: int, counts_ptr: int = 0, max_dist2: float = float("inf"),
                                max_pairs: int = 1, any_only: bool = False, skip_shared: bool = False, stream_ptr: int = 0):
        """Asynchronous triangle-distance queries on device memory of the scene's device (shray_clearance_triangles_device):
        `count` shray_triangle records at `triangles_ptr` -> count * max_pairs shray_pair_distance records at `out_ptr` (0 iff
        max_pairs is 0) and, unless `counts_ptr` is 0, `count` int32 counts there, on a HIP stream (`stream_ptr`)."""
        op = clearance_params(max_pairs, max_dist2, any_only, skip_shared)
        N.check(N.load_clearance().shray_clearance_triangles_device(self._handle, C.byref(op), _ptr(triangles_ptr), count, _ptr(out_ptr),
                                                                    _ptr(counts_ptr), _ptr(stream_ptr)))

    def clearance_counts(self, triangles, max_dist2: float, skip_shared: bool = False):
        """How many scene triangles lie within `max_dist2` of each query triangle (triangle_distances with max_pairs = 0):
        int32 [n], numpy for host triangles, a tensor for GPU triangles."""
        return self.triangle_distances(triangles, max_dist2, max_pairs=0, counts=True, skip_shared=skip_shared)[1]

    def within_tolerance(self, triangles, max_dist2: float, skip_shared: bool = False):
        """Whether any scene triangle lies within `max_dist2` of each query triangle (SHRAY_CLEARANCE_ANY: the walk stops at
        the first one): bool [n], numpy for host triangles, a tensor for GPU triangles."""
        return self.triangle_distances(triangles, max_dist2, max_pairs=0, counts=True, skip_shared=skip_shared, any_only=True)[1] != 0

    def self_clearance(self, max_dist2: float = float("inf"), max_pairs: int = 1, skip_shared: bool = True, first: int = 0,
                       count: int | None = None, counts: bool = True, any_only: bool = False, device: bool = False):
        """The scene's own triangles [first, first + count) as the queries (shray_clearance_self; count=None: up to the last
        one), read from the scene's positions as they are when the query runs: how close the mesh comes to itself.  Returns
        (records: PAIR_DISTANCE_DTYPE [count, max_pairs], counts: int32 [count]) as numpy arrays from the blocking form, or
        with device=True as tensors on the scene's device (the records int32 [count, max_pairs, 12]) enqueued on the current
        torch stream (shray_clearance_self_device).  skip_shared defaults to True here: without it every triangle finds
        itself and its neighbours at distance 0.  max_pairs = 0 returns None for the records, counts=False None for the
        counts; any_only as for triangle_distances."""
        lib = N.load_clearance()
        return _own_triangles(self._handle, (lib.shray_clearance_self_device, lib.shray_clearance_self),
                              clearance_params(max_pairs, max_dist2, any_only, skip_shared), None, first, count, self.triangle_count,
                              max_pairs, "max_pairs", PAIR_DISTANCE_DTYPE, (12,), counts, device, self.device_index)

    def self_clearance_into(self, first: int, count: int, out_ptr: int, counts_ptr: int = 0, max_dist2: float = float("inf"),
                            max_pairs: int = 1, any_only: bool = False, skip_shared: bool = True, stream_ptr: int = 0):
        """Asynchronous self-proximity queries (shray_clearance_self_device): the scene's triangles [first, first + count) ->
        count * max_pairs shray_pair_distance records at `out_ptr` (0 iff max_pairs is 0) and, unless `counts_ptr` is 0,
        `count` int32 counts there, device memory of the scene's device, on a HIP stream (`stream_ptr`)."""
        op = clearance_params(max_pairs, max_dist2, any_only, skip_shared)
        N.check(N.load_clearance().shray_clearance_self_device(self._handle, C.byref(op), first, count, _ptr(out_ptr),
                                                               _ptr(counts_ptr), _ptr(stream_ptr)))

    def distance_to(self, other: "Scene", max_dist2: float = float("inf"), max_pairs: int = 1, counts: bool = True,
                    skip_shared: bool = False):
        """Mesh against mesh: the queries are the other scene's current triangles (other.geometry(), so after its refits), in
        its triangle order; the blocking host path of triangle_distances on this scene.  Returns (records, counts, minimum):
        the per-triangle records and counts of triangle_distances, and the smallest dist2 of any pair within `max_dist2` (0
        where the meshes interpenetrate, +inf where no pair is that near) -- the clearance of the two meshes, squared."""
        if max_pairs < 1:
            raise ValueError("distance_to needs max_pairs >= 1: the minimum is read from each query's first record")
        theirs = np.asarray(other.geometry()["vertex_positions"], np.float32).reshape(-1, 9)
        records, n = self.triangle_distances(theirs, max_dist2, max_pairs=max_pairs, counts=counts, skip_shared=skip_shared)
        found = records[:, 0][records[:, 0]["triangle"] >= 0]
        return records, n, float(found["dist2"].min()) if len(found) else float("inf")

    def surface_voxels(self, origin, cell, dims, device=None):
        """The occupancy grid of the surface: bool [nx, ny, nz], voxel (i, j, k) set iff a triangle touches the box
        lo = origin + (i, j, k) * cell, hi = origin + (i + 1, j + 1, k + 1) * cell.  Each bound is one fp32 multiply and one
        add, by the same expression for a face two voxels share, so neighbours share a bit-identical plane.  `cell`: a scalar
        or three floats.  device=None builds the boxes with numpy and takes the host path; a torch device (the scene's)
        builds them there with torch and returns a tensor.  The query is boxes_touched."""
        boxes = voxel_boxes(origin, cell, dims, device)
        nx, ny, nz = (int(d) for d in dims)
        return self.boxes_touched(boxes).reshape(nx, ny, nz)

    def primary_hits(self, params: N.FrameParams, width: int, height: int) -> np.ndarray:
        """The hit of every pixel's 1-spp primary ray (shray_primary_hits_device): HIT_DTYPE [height, width], row 0 = bottom."""
        import torch
        out = torch.empty((height * width, 4), dtype=torch.int32, device="cuda")
        N.check(N.load_query().shray_primary_hits_device(self._handle, C.byref(params), width, height, C.c_void_p(out.data_ptr()),
                                                         C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        return np.ascontiguousarray(out.cpu().numpy()).view(HIT_DTYPE).reshape(height, width)

    def refit(self, vertex_data, triangle_vertices=None, normal_offset: int | None = None, stream_ptr: int = 0) -> dict:
        """Refits the scene's BVH to moved vertices (include/shader_ray_refit.h): the tree, the triangle order and every triangle
        index stay; the corners, boxes and everything derived from them are rewritten in place.  `vertex_data` is [V, stride]
        float32 (stride >= 3, the position first); `triangle_vertices` [T, 3] int32 vertex indices in the scene's triangle order,
        or None: `vertex_data` holds the 3 T corners themselves.  `normal_offset`: the column of each vertex's normal, or None to
        keep the scene's normals.  numpy arrays and CPU tensors take the blocking host path (shray_scene_refit); GPU tensors, which
        must be on the scene's device, the device path (shray_scene_refit_device) on `stream_ptr` (e.g.
        torch.cuda.current_stream().cuda_stream), which also returns once the scene is updated.  Returns {"sah_cost", "exact_div_ok"}."""
        vertex_data, triangle_vertices = _host_if_cpu(vertex_data), _host_if_cpu(triangle_vertices)
        device = _is_torch(vertex_data)
        if triangle_vertices is not None and _is_torch(triangle_vertices) != device:
            raise TypeError("vertex_data and triangle_vertices must both be on the host or both GPU tensors")
        lib = N.load_refit()
        corners = C.c_int32()
        N.check(lib.shray_scene_geometry_counts(self._handle, C.byref(corners), None))
        if triangle_vertices is not None:
            count = triangle_vertices.numel() if device else np.size(triangle_vertices)
            if count != corners.value:
                raise ValueError(f"triangle_vertices holds {count} indices, the scene has {corners.value} corners (3 per triangle)")
        if device:
            here = self.device_index()
            for name, t in (("vertex_data", vertex_data), ("triangle_vertices", triangle_vertices)):
                if t is not None and t.device.index != here:
                    raise ValueError(f"{name} is on {t.device}, the scene on cuda:{here}")
        inp = N.RefitInput()
        inp.struct_size = C.sizeof(N.RefitInput)
        inp.normal_offset_floats = -1 if normal_offset is None else int(normal_offset)
        keep = []
        if device:
            import torch
            if vertex_data.dtype != torch.float32 or vertex_data.dim() != 2 or not vertex_data.is_contiguous():
                raise ValueError("vertex_data must be a contiguous float32 [V, stride] tensor")
            inp.vertex_count, inp.vertex_stride_floats = vertex_data.shape
            inp.vertex_data = vertex_data.data_ptr()
            if triangle_vertices is not None:
                if triangle_vertices.dtype != torch.int32 or not triangle_vertices.is_contiguous():
                    raise ValueError("triangle_vertices must be a contiguous int32 tensor")
                inp.triangle_vertices = triangle_vertices.data_ptr()
        else:
            vd = np.ascontiguousarray(vertex_data, dtype=np.float32)
            if vd.ndim != 2:
                raise ValueError("vertex_data must be [V, stride] float32")
            inp.vertex_count, inp.vertex_stride_floats = vd.shape
            inp.vertex_data = vd.ctypes.data
            keep.append(vd)
            if triangle_vertices is not None:
                tv = np.ascontiguousarray(triangle_vertices, dtype=np.int32)
                inp.triangle_vertices = tv.ctypes.data
                keep.append(tv)
        stats = N.RefitStats()
        if device:
            N.check(lib.shray_scene_refit_device(self._handle, C.byref(inp), C.byref(stats), _ptr(stream_ptr)))
        else:
            N.check(lib.shray_scene_refit(self._handle, C.byref(inp), C.byref(stats)))
        return stats.as_dict()

    def geometry(self) -> dict:
        """The scene's reference-layout geometry as it is now (shray_scene_geometry_download): vertex_positions and
        vertex_normals float32 [corners * 3], group_boxmin and group_boxmax float32 [nodes * 3] (the flattener's numbering)."""
        lib = N.load_refit()
        corners, nodes = C.c_int32(), C.c_int32()
        N.check(lib.shray_scene_geometry_counts(self._handle, C.byref(corners), C.byref(nodes)))
        out = {"vertex_positions": np.zeros(3 * corners.value, np.float32), "vertex_normals": np.zeros(3 * corners.value, np.float32),
               "group_boxmin": np.zeros(3 * nodes.value, np.float32), "group_boxmax": np.zeros(3 * nodes.value, np.float32)}
        N.check(lib.shray_scene_geometry_download(self._handle, *(out[k].ctypes.data_as(N.c_float_p) for k in
                                                                  ("vertex_positions", "vertex_normals", "group_boxmin", "group_boxmax"))))
        return out

    def device_index(self) -> int:
        d = C.c_int()
        N.check(self._lib.shray_scene_device(self._handle, C.byref(d)))
        return d.value

    def render_batch_into(self, params_list, width: int, height: int, spp: int, out_ptr: int, frame_stride_bytes: int,
                          stream_ptr: int = 0, tiles: N.TileSet | None = None):
        """`len(params_list)` frames in one launch; frame k goes to out_ptr + k * frame_stride_bytes
        (shray_render_batch_device)."""
        count = len(params_list)
        array = (N.FrameParams * count)(*params_list)
        N.check(self._lib.shray_render_batch_device(
            self._handle, array, count, width, height, spp, C.byref(tiles) if tiles is not None else None, _ptr(out_ptr), frame_stride_bytes,
            _ptr(stream_ptr)))


def _is_torch(a) -> bool:
    return type(a).__module__.startswith("torch") and hasattr(a, "data_ptr")


def _host_if_cpu(a):
    """a torch tensor in host memory as a numpy array (the host path takes it); anything else as it is"""
    return a.detach().numpy() if _is_torch(a) and not a.is_cuda else a


def _ptr(address):
    """an address (a data_ptr(), an int argument of an _into method) as a pointer argument; 0 and None are NULL"""
    return C.c_void_p(address or None)


def _on_device(tensor, device_index: int, owner: str, kind: str, name: str, widths, forms: str):
    """The device-side converters' checks: `tensor` (`kind`: "rays", "points", ...) is on the device of `owner` ("the scene",
    "the set") and is float32 [n, w] with w among `widths`.  Returns torch."""
    import torch
    if tensor.device.index != device_index:
        raise ValueError(f"{kind} are on {tensor.device}, {owner} on cuda:{device_index}")
    if tensor.dtype != torch.float32 or tensor.dim() != 2 or tensor.shape[1] not in widths:
        raise ValueError(f"a GPU {name} tensor must be float32 {forms}")
    return torch


def _replaced(tensor, given, column: int, value):
    """`tensor` with `value` (a scalar or [n]) in `column`, unless it is None: in a copy where `tensor` is the caller's own"""
    if value is not None:
        import torch
        tensor = tensor.clone() if tensor is given else tensor
        tensor[:, column] = torch.as_tensor(value, dtype=torch.float32, device=tensor.device)
    return tensor


def _device_rays(rays, device_index: int, owner: str, tmax=None):
    """a float32 [n, 8] GPU tensor on the device of `owner` as a contiguous shray_ray tensor (a copy when `tmax` replaces the
    rays' own)"""
    _on_device(rays, device_index, owner, "rays", "ray", (8,), "[n, 8] (the shray_ray layout)")
    return _replaced(rays.contiguous(), rays, 3, tmax)


def _device_points(points, device_index: int, owner: str, max_dist2=None):
    """a float32 [n, 3] / [n, 4] GPU tensor on the device of `owner` as a contiguous [n, 4] shray_point tensor (a copy when
    `max_dist2` replaces the points' own)"""
    torch = _on_device(points, device_index, owner, "points", "point", (3, 4), "[n, 3] (p) or [n, 4] (the shray_point layout)")
    if points.shape[1] == 3:
        pts = torch.empty((len(points), 4), dtype=torch.float32, device=points.device)
        pts[:, :3] = points
        pts[:, 3] = float("inf")
    else:
        pts = points.contiguous()
    return _replaced(pts, points, 3, max_dist2)


def _device_boxes(boxes, device_index: int, owner: str):
    """a float32 [n, 6] / [n, 8] GPU tensor on the device of `owner` as a contiguous [n, 8] shray_box tensor"""
    torch = _on_device(boxes, device_index, owner, "boxes", "box", (6, 8), "[n, 6] (lo, hi) or [n, 8] (the shray_box layout)")
    if boxes.shape[1] == 8:
        return boxes.contiguous()
    bx = torch.zeros((len(boxes), 8), dtype=torch.float32, device=boxes.device)
    bx[:, 0:3] = boxes[:, 0:3]
    bx[:, 4:7] = boxes[:, 3:6]
    return bx


def _device_triangles(triangles, device_index: int, owner: str):
    """a float32 [n, 9] / [n, 12] GPU tensor on the device of `owner` as a contiguous [n, 12] shray_triangle tensor"""
    torch = _on_device(triangles, device_index, owner, "triangles", "triangle", (9, 12),
                       "[n, 9] (a, b, c) or [n, 12] (the shray_triangle layout)")
    if triangles.shape[1] == 12:
        return triangles.contiguous()
    tr = torch.zeros((len(triangles), 12), dtype=torch.float32, device=triangles.device)
    for corner in range(3):
        tr[:, 4 * corner:4 * corner + 3] = triangles[:, 3 * corner:3 * corner + 3]
    return tr


def _out(want, dtype, *trailing, k=None):
    """An output of _per_item and _own_triangles: wanted or not, then per item `dtype` records (`k` of them, unless None) in
    an array, int32 / float32 [*trailing] ([k, *trailing]) in a tensor."""
    lead = () if k is None else (k,)
    return bool(want), dtype, lead, lead + trailing


def _new_outputs(outs, rows: int, device=None):
    """the wanted ones of `outs` (_out) with `rows` rows each, None for the others: arrays, or with `device` tensors there"""
    if device is None:
        return [np.empty((rows, *shape), dtype) if want else None for want, dtype, shape, _ in outs]
    import torch
    return [torch.empty((rows, *shape), dtype=torch.float32 if dtype is np.float32 else torch.int32, device=device) if want else None
            for want, dtype, _, shape in outs]


def _blocking(handle, host_form, counters_form, lead, d, after, outs, counters: bool = False):
    """_per_item's host half: `d` is the converted array of items."""
    got = _new_outputs(outs, len(d))
    args = (handle, *lead, d.ctypes.data_as(C.c_void_p), len(d), *after,
            *(o.ctypes.data_as(C.c_void_p) if o is not None else None for o in got))
    if counters:
        c = N.Counters()
        N.check(counters_form(*args, C.byref(c)))
        return (*got, c.as_dict())
    N.check(host_form(*args))
    return tuple(got)


def _per_item(handle, forms, lead, items, converters, after, outs, counters: bool = False):
    """Items in, per-item outputs out: the one marshalling path of the queries that take an items argument.  `forms`: the
    library's device form, blocking form and blocking form with counters (None where it has none), called with (`handle`,
    *`lead`, items, n, *`after`, an address or NULL per output[, the stream | the counters]).  `items`: a GPU tensor takes the
    device path on the current torch stream of its device, anything else (a CPU tensor as numpy) the blocking path;
    `converters` (_converters) names the kind and makes of either the library's layout, refusing another device or form.
    `outs`: an _out per output.  `counters` are refused on the device path.  Returns the outputs in order, None for those
    not wanted, as tensors or arrays[, then the counters as a dict]."""
    kind, on_device, on_host = converters
    items = _host_if_cpu(items)
    if not _is_torch(items):
        return _blocking(handle, forms[1], forms[2], lead, on_host(items), after, outs, counters)
    import torch
    if counters:
        raise ValueError(f"counters are counted on the host path: pass host {kind}")
    d = on_device(items)
    got = _new_outputs(outs, len(d), d.device)
    stream = torch.cuda.current_stream(d.device)
    d.record_stream(stream)   # (the query reads it after this call returns)
    N.check(forms[0](handle, *lead, _ptr(d.data_ptr()), len(d), *after, *(_ptr(None if o is None else o.data_ptr()) for o in got),
                     _ptr(stream.cuda_stream)))
    return tuple(got)


def _first_k(handle, functions, params, k: int, k_name: str, items, converters, record_dtype, trailing, second: bool, counts: bool,
             counters: bool):
    """The counted first-K queries (all-hits rays, within-radius, box-overlap, triangle-intersection, triangle-distance, and
    their instanced forms) through _per_item: per item a count and its first `k` records.  The records are an int32 [n, k,
    *trailing] tensor or a `record_dtype` [n, k] array, None when `k` is 0 (the library refuses a negative k); with `second`
    an int32 [n, k] output follows them (the instances); the counts are int32 [n], None unless `counts`.  Returns
    (records[, second], counts[, counters])."""
    if k == 0 and not counts:
        raise ValueError(f"nothing is asked for: {k_name} is 0 and counts is False")
    outs = [_out(k > 0, record_dtype, *trailing, k=k)] + ([_out(k > 0, np.int32, k=k)] if second else []) + [_out(counts, np.int32)]
    return _per_item(handle, functions, (C.byref(params),), items, converters, (), outs, counters)


def _own_triangles(handle, forms, params, instance, first: int, count, triangles, k: int, k_name: str, record_dtype, trailing,
                   counts: bool, device: bool, device_index):
    """The range forms: the queries are an owner's own triangles [first, first + count) (count None: up to the last of its
    `triangles()`), of instance `instance` of a set or (None) of a scene.  `forms`: the library's device and blocking form,
    called with (`handle`, `params`[, instance], first, count, records[, instances], counts[, the stream]).  Returns
    (records[, instances], counts) as _first_k does, arrays or with `device` tensors on cuda:`device_index()` enqueued on
    the current torch stream, of `rows` rows: `count`, or 0 for a range the library refuses."""
    if k == 0 and not counts:
        raise ValueError(f"nothing is asked for: {k_name} is 0 and counts is False")
    total = triangles()
    if count is None:
        count = max(total - first, 0)
    rows = count if first >= 0 and 0 <= count <= total - first else 0
    outs = [_out(k > 0, record_dtype, *trailing, k=k)] + ([_out(k > 0, np.int32, k=k)] if instance is not None else []) + [_out(counts, np.int32)]
    args = (handle, C.byref(params), *(() if instance is None else (instance,)), first, count)
    if not device:
        got = _new_outputs(outs, rows)
        N.check(forms[1](*args, *(o.ctypes.data_as(C.c_void_p) if o is not None else None for o in got)))
        return tuple(got)
    import torch
    where = torch.device("cuda", device_index())
    got = _new_outputs(outs, max(rows, 1), where)   # (an empty tensor has no pointer: one row is allocated for an empty range)
    N.check(forms[0](*args, *(_ptr(None if o is None else o.data_ptr()) for o in got), _ptr(torch.cuda.current_stream(where).cuda_stream)))
    return tuple(None if o is None else o[:rows] for o in got)


# a ray buffer / hit array of the query (include/shader_ray_query.h): 32 and 16 bytes per element
RAY_DTYPE = np.dtype([("origin", np.float32, 3), ("tmax", np.float32), ("direction", np.float32, 3), ("reserved", np.float32)])
HIT_DTYPE = np.dtype([("t", np.float32), ("u", np.float32), ("v", np.float32), ("triangle", np.int32)])


def _host_records(records, dtype, short, long, build, field, value, form) -> np.ndarray:
    """`dtype` records, or [n, short] (through `build`) / [n, long] (the C layout) float32, as one contiguous `dtype` array;
    `value`, unless None, replaces `field` in a copy.  `form` describes the accepted forms in the error."""
    records = np.asarray(records)
    if records.dtype != dtype:
        a = np.asarray(records, np.float32)
        if a.ndim != 2 or a.shape[1] not in (short, long):
            raise ValueError(form)
        records = build(a) if a.shape[1] == short else np.ascontiguousarray(a).view(dtype).reshape(-1)
    records = np.ascontiguousarray(records).copy() if value is not None else np.ascontiguousarray(records)
    if value is not None:
        records[field] = np.asarray(value, np.float32)
    return records


def _host_rays(rays, tmax=None) -> np.ndarray:
    """Scene.trace_rays's ray forms as one contiguous RAY_DTYPE array (a copy when `tmax` replaces the rays' own)."""
    return _host_records(rays, RAY_DTYPE, 6, 8, lambda a: make_rays(a[:, 0:3], a[:, 3:6]), "tmax", tmax,
                         "rays must be a RAY_DTYPE array or [n, 6] (origin, direction) / [n, 8] (shray_ray) float32")


def make_rays(origins, directions, tmax=None) -> np.ndarray:
    """A RAY_DTYPE array from [n, 3] origins and directions; tmax: a scalar or [n] (default 1e7, the shader's infinitely_far)."""
    origins = np.asarray(origins, np.float32).reshape(-1, 3)
    rays = np.zeros(len(origins), RAY_DTYPE)
    rays["origin"] = origins
    rays["direction"] = np.asarray(directions, np.float32).reshape(-1, 3)
    rays["tmax"] = np.float32(1e7) if tmax is None else np.asarray(tmax, np.float32)
    return rays


# a point buffer / result array of the closest-point query (include/shader_ray_point.h): 16 and 32 bytes per element
POINT_DTYPE = np.dtype([("p", np.float32, 3), ("max_dist2", np.float32)])
CLOSEST_DTYPE = np.dtype([("q", np.float32, 3), ("dist2", np.float32), ("u", np.float32), ("v", np.float32), ("triangle", np.int32),
                          ("region", np.int32)])


def _host_points(points, max_dist2=None) -> np.ndarray:
    """Scene.closest_points's host point forms as one contiguous POINT_DTYPE array (a copy when `max_dist2` replaces the
    points' own)."""
    return _host_records(points, POINT_DTYPE, 3, 4, make_points, "max_dist2", max_dist2,
                         "points must be a POINT_DTYPE array or [n, 3] (p) / [n, 4] (shray_point) float32")


def make_points(p, max_dist2=None) -> np.ndarray:
    """A POINT_DTYPE array from [n, 3] points; max_dist2: a scalar or [n] (default +inf: no limit)."""
    p = np.asarray(p, np.float32).reshape(-1, 3)
    out = np.zeros(len(p), POINT_DTYPE)
    out["p"] = p
    out["max_dist2"] = np.float32(np.inf) if max_dist2 is None else np.asarray(max_dist2, np.float32)
    return out


def query_params(any_hit: bool = False, max_bvh_iterations: int = 400, max_leaf_tests: int = 10) -> N.QueryParams:
    qp = N.QueryParams()
    N.load_query().shray_query_params_init(C.byref(qp))
    qp.max_bvh_iterations, qp.max_leaf_tests, qp.any_hit = max_bvh_iterations, max_leaf_tests, 1 if any_hit else 0
    return qp


def multihit_params(max_hits: int = 8, max_leaf_tests: int = 10) -> N.MultihitParams:
    mp = N.MultihitParams()
    N.load_multihit().shray_multihit_params_init(C.byref(mp))
    mp.max_hits, mp.max_leaf_tests = max_hits, max_leaf_tests
    return mp


def near_params(max_near: int = 8) -> N.NearParams:
    np_ = N.NearParams()
    N.load_near().shray_near_params_init(C.byref(np_))
    np_.max_near = max_near
    return np_


def overlap_params(max_triangles: int = 8, any_only: bool = False) -> N.OverlapParams:
    op = N.OverlapParams()
    N.load_overlap().shray_overlap_params_init(C.byref(op))
    op.max_triangles = max_triangles
    op.flags = N.OVERLAP_ANY if any_only else 0
    return op


def _set_overlap_params(max_triangles: int = 8, any_only: bool = False) -> N.OverlapParams:
    """shray_overlap_params for the instanced query, filled here: libshray_instance_overlap.so does not need libshray_overlap.so"""
    op = N.OverlapParams()
    op.struct_size = C.sizeof(N.OverlapParams)
    op.max_triangles = max_triangles
    op.flags = N.OVERLAP_ANY if any_only else 0
    op.reserved = 0
    return op


def intersect_params(max_triangles: int = 8, any_only: bool = False, skip_shared: bool = False) -> N.IntersectParams:
    op = N.IntersectParams()
    N.load_intersect().shray_intersect_params_init(C.byref(op))
    op.max_triangles = max_triangles
    op.flags = (N.INTERSECT_ANY if any_only else 0) | (N.INTERSECT_SKIP_SHARED if skip_shared else 0)
    return op


def _set_intersect_params(max_triangles: int = 8, any_only: bool = False, skip_shared: bool = False,
                          skip_own: bool = False) -> N.IntersectParams:
    """shray_intersect_params for the instanced query, filled here: libshray_instance_intersect.so does not need
    libshray_intersect.so.  skip_own sets SHRAY_INTERSECT_SKIP_OWN_INSTANCE, which only the instance form accepts."""
    op = N.IntersectParams()
    op.struct_size = C.sizeof(N.IntersectParams)
    op.max_triangles = max_triangles
    op.flags = ((N.INTERSECT_ANY if any_only else 0) | (N.INTERSECT_SKIP_SHARED if skip_shared else 0) |
                (N.INTERSECT_SKIP_OWN_INSTANCE if skip_own else 0))
    op.reserved = 0
    return op


def _pairs_params(first_row: int = 0, row_count: int = 0, any_only: bool = False, upper: bool = False,
                  skip_shared: bool = False) -> N.PairsParams:
    """shray_pairs_params (include/shader_ray_instance_pairs.h)"""
    op = N.PairsParams()
    op.struct_size = C.sizeof(N.PairsParams)
    op.flags = (N.PAIRS_ANY if any_only else 0) | (N.PAIRS_SKIP_SHARED if skip_shared else 0) | (N.PAIRS_UPPER if upper else 0)
    op.first_row, op.row_count = first_row, row_count
    return op


def clearance_params(max_pairs: int = 1, max_dist2: float = float("inf"), any_only: bool = False,
                     skip_shared: bool = False) -> N.ClearanceParams:
    op = N.ClearanceParams()
    N.load_clearance().shray_clearance_params_init(C.byref(op))
    op.max_pairs = max_pairs
    op.flags = (N.CLEARANCE_ANY if any_only else 0) | (N.CLEARANCE_SKIP_SHARED if skip_shared else 0)
    op.max_dist2 = float(max_dist2)   # (ctypes rounds a python float to float32)
    return op


def _set_clearance_params(max_pairs: int = 1, max_dist2: float = float("inf"), any_only: bool = False, skip_shared: bool = False,
                          skip_own: bool = False) -> N.ClearanceParams:
    """shray_clearance_params for the instanced query, filled here: libshray_instance_clearance.so does not need
    libshray_clearance.so.  skip_own sets SHRAY_CLEARANCE_SKIP_OWN_INSTANCE, which only the instance form accepts."""
    op = N.ClearanceParams()
    op.struct_size = C.sizeof(N.ClearanceParams)
    op.max_pairs = max_pairs
    op.flags = ((N.CLEARANCE_ANY if any_only else 0) | (N.CLEARANCE_SKIP_SHARED if skip_shared else 0) |
                (N.CLEARANCE_SKIP_OWN_INSTANCE if skip_own else 0))
    op.max_dist2 = float(max_dist2)   # (ctypes rounds a python float to float32)
    return op


# a record of the triangle-distance query (include/shader_ray_clearance.h): 48 bytes per element
PAIR_DISTANCE_DTYPE = np.dtype([("on_query", np.float32, 3), ("dist2", np.float32), ("on_scene", np.float32, 3), ("triangle", np.int32),
                                ("feature", np.int32), ("reserved", np.int32, 3)])


# a triangle buffer of the triangle-intersection query (include/shader_ray_intersect.h): 48 bytes per element
TRIANGLE_DTYPE = np.dtype([("a", np.float32, 3), ("pad0", np.float32), ("b", np.float32, 3), ("pad1", np.float32), ("c", np.float32, 3),
                           ("pad2", np.float32)])


def make_triangles(a, b=None, c=None) -> np.ndarray:
    """A TRIANGLE_DTYPE array from [n, 3, 3] or [n, 9] corners, or from three [n, 3] arrays a, b, c."""
    if b is None:
        corners = np.asarray(a, np.float32).reshape(-1, 3, 3)
        a, b, c = corners[:, 0], corners[:, 1], corners[:, 2]
    a = np.asarray(a, np.float32).reshape(-1, 3)
    out = np.zeros(len(a), TRIANGLE_DTYPE)
    out["a"] = a
    out["b"] = np.asarray(b, np.float32).reshape(-1, 3)
    out["c"] = np.asarray(c, np.float32).reshape(-1, 3)
    return out


def _host_triangles(triangles) -> np.ndarray:
    """Scene.intersecting_triangles's host triangle forms as one contiguous TRIANGLE_DTYPE array."""
    triangles = np.asarray(triangles)
    if triangles.dtype != TRIANGLE_DTYPE and triangles.ndim == 3 and triangles.shape[1:] == (3, 3):
        triangles = triangles.reshape(-1, 9)
    return _host_records(triangles, TRIANGLE_DTYPE, 9, 12, make_triangles, None, None,
                         "triangles must be a TRIANGLE_DTYPE array or [n, 3, 3] / [n, 9] (a, b, c) / [n, 12] (shray_triangle) float32")


# a box buffer of the box-overlap query (include/shader_ray_overlap.h): 32 bytes per element
BOX_DTYPE = np.dtype([("lo", np.float32, 3), ("pad0", np.float32), ("hi", np.float32, 3), ("pad1", np.float32)])


def make_boxes(lo, hi) -> np.ndarray:
    """A BOX_DTYPE array from [n, 3] lower and upper corners."""
    lo = np.asarray(lo, np.float32).reshape(-1, 3)
    out = np.zeros(len(lo), BOX_DTYPE)
    out["lo"] = lo
    out["hi"] = np.asarray(hi, np.float32).reshape(-1, 3)
    return out


def _host_boxes(boxes) -> np.ndarray:
    """Scene.triangles_in_boxes's host box forms as one contiguous BOX_DTYPE array."""
    return _host_records(boxes, BOX_DTYPE, 6, 8, lambda a: make_boxes(a[:, 0:3], a[:, 3:6]), None, None,
                         "boxes must be a BOX_DTYPE array or [n, 6] (lo, hi) / [n, 8] (shray_box) float32")


# the item kinds of the queries: kind -> (the device-side converter, the host-side converter)
_CONVERTERS = {"rays": (_device_rays, _host_rays), "points": (_device_points, _host_points), "boxes": (_device_boxes, _host_boxes),
               "triangles": (_device_triangles, _host_triangles)}


def _converters(kind: str, device_index, owner: str, value=None):
    """_per_item's converters of an items argument: (`kind`, the device-side one, the host-side one).  `device_index`: a
    callable, asked on the device path only; `value`, unless None, replaces the rays' tmax / the points' max_dist2."""
    on_device, on_host = _CONVERTERS[kind]
    if value is None:
        return kind, lambda tensor: on_device(tensor, device_index(), owner), on_host
    return kind, lambda tensor: on_device(tensor, device_index(), owner, value), lambda array: on_host(array, value)


def voxel_boxes(origin, cell, dims, device=None):
    """Scene.surface_voxels's boxes in grid order (k fastest): plane i of an axis is origin + i * cell in fp32, one multiply and
    one add; a voxel's lo and hi are two neighbouring planes.  A BOX_DTYPE array, or with `device` a float32 [n, 8] tensor."""
    nx, ny, nz = (int(d) for d in dims)
    if min(nx, ny, nz) < 1:
        raise ValueError("dims must be three positive integers")
    origin = np.asarray(origin, np.float32).reshape(3)
    cell = np.broadcast_to(np.asarray(cell, np.float32), (3,))
    if device is None:
        planes = [origin[a] + np.arange(n + 1, dtype=np.float32) * cell[a] for a, n in enumerate((nx, ny, nz))]
        out = np.zeros((nx, ny, nz), BOX_DTYPE)
        for a, shape in enumerate(((nx, 1, 1), (1, ny, 1), (1, 1, nz))):
            out["lo"][..., a] = planes[a][:-1].reshape(shape)
            out["hi"][..., a] = planes[a][1:].reshape(shape)
        return out.reshape(-1)
    import torch
    out = torch.zeros((nx, ny, nz, 8), dtype=torch.float32, device=device)
    for a, (n, shape) in enumerate(((nx, (nx, 1, 1)), (ny, (1, ny, 1)), (nz, (1, 1, nz)))):
        steps = torch.arange(n + 1, dtype=torch.float32, device=device) * float(cell[a])
        planes = steps + float(origin[a])
        out[..., a] = planes[:-1].reshape(shape)
        out[..., 4 + a] = planes[1:].reshape(shape)
    return out.reshape(-1, 8)


class DeviceFlat:
    """get_shader_data on the GPU (shray_flatten_device): the flattened arrays of a host-built BVH, resident
    on the device.  `download()` gives a SceneDesc with host pointers (owned by this object)."""

    def __init__(self, tree: N.TreeDesc, data_texture_width: int = 2048):
        self._lib = N.load_hip()
        self._tree = tree
        handle = C.c_void_p()
        N.check(self._lib.shray_flatten_device(C.byref(tree), data_texture_width, C.byref(handle)))
        self._handle = handle

    def download(self) -> N.SceneDesc:
        desc = N.SceneDesc()
        N.check(self._lib.shray_device_flat_download(self._handle, C.byref(desc)))
        desc._owner = self
        return desc

    def describe(self) -> N.SceneDesc:
        desc = N.SceneDesc()
        N.check(self._lib.shray_device_flat_describe(self._handle, C.byref(desc)))
        desc._owner = self
        return desc

    def arrays(self) -> dict:
        from .host import desc_arrays
        return desc_arrays(self.download())

    def close(self):
        if getattr(self, "_handle", None):
            self._lib.shray_device_flat_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceWorld:
    """File -> resident scene with the BVH, the flattening and everything scene creation derives done ON THE DEVICE (round 6):
    the host parses the file (libshray_host: load_triangles -- world.cpp:46-134 without make_bvh); shray_bvh_build_device,
    shray_flatten_device_tree and shray_scene_create_from_device do the rest where the data lies.  No tree is downloaded and no
    group tree is built on the host unless somebody asks for one (`host_world()`).  `seconds`: the stages' wall times."""

    def __init__(self, filename: str, environment: np.ndarray | None = None, options: "N.BvhOptions | None" = None, device: int | None = None,
                 data_texture_width: int = 2048, quiet: bool = True):
        import time
        from . import host
        hip, lib = N.load_hip(), N.load_host()
        lib.shray_host_set_quiet(1 if quiet else 0)
        if device is not None:
            N.check(hip.shray_set_device(device))
        self._hip, self._host, self.filename = hip, lib, filename
        self.seconds = {}
        t0 = time.perf_counter()
        handle = C.c_void_p()
        if lib.shray_host_load_triangles(filename.encode(), C.byref(handle)) != 0 or not handle:
            raise RuntimeError(f"load_triangles failed for {filename!r} (see stderr)")
        self._world_handle = handle
        tv, vd, nt, nv = C.POINTER(C.c_int32)(), C.POINTER(C.c_float)(), C.c_int32(), C.c_int32()
        if lib.shray_host_triangles(handle, C.byref(tv), C.byref(nt), C.byref(vd), C.byref(nv)) != 0:
            raise RuntimeError("shray_host_triangles failed")
        t1 = time.perf_counter()
        if options is None:
            options = host.bvh_options_from_environment()
        options.struct_size = C.sizeof(N.BvhOptions)
        self._options = options
        self._tree = C.c_void_p()
        N.check(hip.shray_bvh_build_device(tv, nt, vd, nv, 9, C.byref(options), C.byref(self._tree)))
        t2 = time.perf_counter()
        self._flat = C.c_void_p()
        N.check(hip.shray_flatten_device_tree(self._tree, data_texture_width, C.byref(self._flat)))
        t3 = time.perf_counter()
        self.scene = Scene.from_device(self._tree, self._flat, None)
        t4 = time.perf_counter()
        if environment is not None:
            self.scene.set_environment(environment)
        stats = N.BvhStats()
        N.check(hip.shray_device_tree_stats(self._tree, C.byref(stats)))
        self.stats = stats
        self.triangle_count = nt.value
        self.seconds = {"parse": t1 - t0, "bvh": t2 - t1, "bvh_on_the_device": stats.device_seconds, "flatten": t3 - t2, "scene": t4 - t3,
                        "triangles_to_resident": t4 - t1, "total": t4 - t0}
        self._adopted = False

    def frame_params(self, width: int, height: int, view=None, material: int | None = None, diffuse: int | None = None):
        """The frame block (ray.cpp:648-704) -- it needs the mesh's extent, not its tree."""
        from . import host
        return host.frame_params_of(self._world_handle, width, height, view, material, diffuse)

    def default_view(self):
        from . import host
        return host.default_view_of(self._world_handle)

    def flat_arrays(self) -> dict:
        """The flattened (reference-layout) arrays, downloaded (tests)."""
        from .host import desc_arrays
        desc = N.SceneDesc()
        N.check(self._hip.shray_device_flat_download(self._flat, C.byref(desc)))
        return desc_arrays(desc)

    def refit(self, vertex_data, stream_ptr: int | None = None) -> dict:
        """Refits the scene to moved vertices (Scene.refit): `vertex_data` is [V, 3] or [V, 9] float32 (numpy, or a torch tensor on
        the scene's device), in the numbering of the loaded triangle set (shray_host_triangles); with 9 columns (geometry.h:34-38)
        the normals are taken from column 6, with 3 the scene's normals are kept.  The tree's post-build triangle_vertices are
        uploaded once and reused.  Runs on `stream_ptr` (default: torch's current stream).  frame_params() stays framed on the
        mesh as loaded, and flat_arrays() and host_world() keep describing the loaded mesh."""
        import torch
        if getattr(self, "_d_triangle_vertices", None) is None:
            tree = N.TreeDesc()
            N.check(self._hip.shray_device_tree_download(self._tree, C.byref(tree), None))
            tv = np.ctypeslib.as_array(tree.triangle_vertices, shape=(3 * tree.triangle_count,)).copy() if tree.triangle_count else \
                np.zeros(0, np.int32)
            self._d_triangle_vertices = torch.from_numpy(tv).to(torch.device("cuda", self.scene.device_index()))
        d = self._d_triangle_vertices.device
        vd = vertex_data if _is_torch(vertex_data) else torch.from_numpy(np.ascontiguousarray(vertex_data, dtype=np.float32))
        vd = vd.to(device=d, dtype=torch.float32).contiguous()
        if vd.dim() != 2 or vd.shape[1] not in (3, 9):
            raise ValueError("vertex_data must be [V, 3] or [V, 9] float32")
        if stream_ptr is None:
            stream_ptr = torch.cuda.current_stream(d).cuda_stream
        return self.scene.refit(vd, self._d_triangle_vertices, 6 if vd.shape[1] == 9 else None, stream_ptr)

    def host_world(self):
        """The reference's `world` with its group tree (world.h:48-51), built NOW from the device's tree: shray_device_tree_download +
        shray_host_adopt_tree.  Returns the libshray_host world handle (owned by this object)."""
        if not self._adopted:
            tree, order = N.TreeDesc(), C.POINTER(C.c_int32)()
            N.check(self._hip.shray_device_tree_download(self._tree, C.byref(tree), C.byref(order)))
            if self._host.shray_host_adopt_tree(self._world_handle, C.byref(tree), order, float(self.seconds.get("bvh", 0.0))) != 0:
                raise RuntimeError("shray_host_adopt_tree refused the device-built tree")
            self._adopted = True
        return self._world_handle

    def close(self):
        if getattr(self, "scene", None) is not None:
            self.scene.close()
            self.scene = None
        for name, destroy in (("_flat", "shray_device_flat_destroy"), ("_tree", "shray_device_tree_destroy")):
            h = getattr(self, name, None)
            if h:
                getattr(self._hip, destroy)(h)
                setattr(self, name, None)
        if getattr(self, "_world_handle", None):
            self._host.shray_host_free_world(self._world_handle)
            self._world_handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# the Scene methods a DeviceWorld has as its own: each passes its arguments on to .scene unchanged
_SCENE_FORWARDS = ("trace_rays", "trace_rays_into", "trace_all_hits", "trace_all_hits_into", "crossing_counts", "closest_points",
                   "closest_points_into", "triangles_within", "triangles_within_into", "near_counts", "triangles_in_boxes",
                   "triangles_in_boxes_into", "box_counts", "boxes_touched", "surface_voxels", "signed_distance", "signed_distance_into",
                   "surface_info", "sign_data", "winding_number", "winding_number_into", "winding_signed_distance",
                   "winding_signed_distance_into", "winding_data", "primary_hits")


def _scene_forward(name: str):
    @functools.wraps(getattr(Scene, name))
    def forward(self, *args, **kwargs):
        return getattr(self.scene, name)(*args, **kwargs)
    forward.__qualname__ = f"DeviceWorld.{name}"
    return forward


for _name in _SCENE_FORWARDS:
    setattr(DeviceWorld, _name, _scene_forward(_name))
del _name


class InstanceSet:
    """Placed copies of resident scenes, traced together (include/shader_ray_instance.h): `scenes` is a list of Scene or
    DeviceWorld objects, all on one device (one entry per instance; an object may repeat), `transforms` [n, 3, 4] float32
    row-major object-to-world maps.  The set keeps references to the objects it was given (a DeviceWorld too: closing it
    destroys its scene), so they outlive it."""

    def __init__(self, scenes, transforms):
        self._lib = N.load_instance()
        self._owners = list(scenes)
        self._scenes = [s.scene if isinstance(s, DeviceWorld) else s for s in self._owners]
        n = len(self._scenes)
        m = self._transforms(transforms, n)
        array = (N.Instance * max(n, 1))()
        for i, scene in enumerate(self._scenes):
            if not isinstance(scene, Scene) or not getattr(scene, "_handle", None):
                raise TypeError(f"instance {i}: not an open Scene or DeviceWorld")
            array[i].scene = scene._handle
            C.memmove(array[i].object_to_world, m[i].ctypes.data, 48)
        handle = C.c_void_p()
        N.check(self._lib.shray_instance_set_create(array, n, C.byref(handle)))
        self._handle = handle
        self.count = n
        self.device = self._scenes[0].device_index()

    @staticmethod
    def _transforms(transforms, n: int) -> np.ndarray:
        m = np.ascontiguousarray(transforms, dtype=np.float32)
        if m.shape != (n, 3, 4):
            raise ValueError(f"transforms must be [{n}, 3, 4] float32, got {list(m.shape)}")
        return m

    def update(self, transforms=None):
        """New object-to-world maps ([n, 3, 4]) or None to keep them; re-reads every member scene (call it after refitting one).
        A float32 [n, 3, 4] torch tensor on the set's device takes the device path (shray_instance_set_update_device) on torch's
        current stream and returns without waiting: a refused map raises nothing here, update_status() reports it.  One on
        another device is refused; numpy arrays and CPU tensors take the blocking host path."""
        transforms = _host_if_cpu(transforms)
        if _is_torch(transforms):
            import torch
            if transforms.device.index != self.device:
                raise ValueError(f"transforms are on {transforms.device}, the set on cuda:{self.device}")
            if transforms.dtype != torch.float32 or tuple(transforms.shape) != (self.count, 3, 4):
                raise ValueError(f"a GPU transform tensor must be float32 [{self.count}, 3, 4], got {transforms.dtype} "
                                 f"{list(transforms.shape)}")
            m = transforms.contiguous()
            stream = torch.cuda.current_stream(m.device)
            m.record_stream(stream)   # (the update reads it after this call returns)
            self.update_into(m.data_ptr(), stream.cuda_stream)
            return
        if transforms is None:
            N.check(self._lib.shray_instance_set_update(self._handle, None))
            return
        m = self._transforms(transforms, self.count)
        N.check(self._lib.shray_instance_set_update(self._handle, m.ctypes.data_as(N.c_float_p)))

    def update_into(self, transforms_ptr: int, stream_ptr: int = 0):
        """The asynchronous update on device memory of the set's device (shray_instance_set_update_device): count * 12 float32
        object-to-world maps at `transforms_ptr`, or 0 to keep the current ones, on a HIP stream (`stream_ptr`, e.g.
        torch.cuda.current_stream().cuda_stream).  The array must stay alive until the update has run."""
        N.check(self._lib.shray_instance_set_update_device(self._handle, _ptr(transforms_ptr), _ptr(stream_ptr)))

    def update_status(self) -> int:
        """Waits for the most recent device update: -1 if it was applied (or none was made), else the lowest instance index whose
        transform was refused (that update changed nothing)."""
        refused = C.c_int32()
        N.check(self._lib.shray_instance_set_update_status(self._handle, C.byref(refused)))
        return refused.value

    def world_to_object(self) -> np.ndarray:
        """W of every instance, [n, 3, 4] float32: the float rounding of the inverse map, as the query applies it."""
        out = np.zeros((self.count, 3, 4), np.float32)
        N.check(self._lib.shray_instance_set_world_to_object(self._handle, out.ctypes.data_as(N.c_float_p)))
        return out

    def trace_rays(self, rays, tmax=None, any_hit: bool = False, max_bvh_iterations: int = 400, max_leaf_tests: int = 10,
                   counters: bool = False):
        """World-space ray queries (Scene.trace_rays's forms, blocking).  A float32 [n, 8] torch tensor on the set's device takes
        the device path; one on another device is refused.  Returns (hits: HIT_DTYPE, instances: int32), and with counters=True
        also the walks' counters."""
        qp = query_params(any_hit, max_bvh_iterations, max_leaf_tests)
        lib = self._lib
        out = _per_item(self._handle, (lib.shray_trace_instances_device, lib.shray_trace_instances, lib.shray_trace_instances_counters),
                        (C.byref(qp),), rays, self._items("rays", tmax), (), [_out(True, HIT_DTYPE, 4), _out(True, np.int32)], counters)
        if _is_torch(out[0]):   # (the copies to the host wait for the query, on the stream it was enqueued on)
            return np.ascontiguousarray(out[0].cpu().numpy()).view(HIT_DTYPE).reshape(-1), out[1].cpu().numpy()
        return out

    def _items(self, kind: str, value=None):
        """_per_item's converters of an items argument of `kind`, for the set's device"""
        return _converters(kind, lambda: self.device, "the set", value)

    def trace_rays_into(self, rays_ptr: int, count: int, hits_ptr: int, instances_ptr: int = 0, stream_ptr: int = 0,
                        any_hit: bool = False, max_bvh_iterations: int = 400, max_leaf_tests: int = 10):
        """Asynchronous world-space ray queries on device memory of the set's device (shray_trace_instances_device): `count`
        shray_ray records at `rays_ptr` -> shray_hit records at `hits_ptr` and, unless `instances_ptr` is 0, int32 instance
        indices there, on a HIP stream (`stream_ptr`, e.g. torch.cuda.current_stream().cuda_stream)."""
        qp = query_params(any_hit, max_bvh_iterations, max_leaf_tests)
        N.check(self._lib.shray_trace_instances_device(self._handle, C.byref(qp), _ptr(rays_ptr), count, _ptr(hits_ptr),
                                                       _ptr(instances_ptr), _ptr(stream_ptr)))

    def trace_all_hits(self, rays, max_hits: int = 8, counts: bool = True, max_leaf_tests: int = 10, counters: bool = False):
        """Instanced all-hits ray queries (include/shader_ray_instance_multihit.h): per world ray the number of surfaces it
        crosses over all instances and its first `max_hits` crossings, sorted by (t, instance, triangle), the other slots
        {tmax, 0, 0, HIT_MISS} with instance -1.  `rays` as for Scene.trace_all_hits: host rays take the blocking path and
        return (hits: HIT_DTYPE [n, max_hits], instances: int32 [n, max_hits], counts: int32 [n]); a float32 [n, 8] GPU tensor
        on the set's device takes the device path on the current torch stream and returns (int32 [n, max_hits, 4] tensor of
        shray_hit records, int32 [n, max_hits] tensor, int32 [n] tensor).  counts=False returns None for the counts and lets
        the walks skip what cannot reach the first `max_hits` (the same records); max_hits = 0 returns None for the hits and
        instances.  counters=True (host rays only) also returns the counters of the form that skips nothing, summed over
        a ray's walks."""
        lib = N.load_instance_multihit()
        return _first_k(self._handle, (lib.shray_trace_instances_all_hits_device, lib.shray_trace_instances_all_hits,
                                       lib.shray_trace_instances_all_hits_counters),
                        multihit_params(max_hits, max_leaf_tests), max_hits, "max_hits", rays, self._items("rays"), HIT_DTYPE, (4,), True,
                        counts, counters)

    def trace_all_hits_into(self, rays_ptr: int, count: int, hits_ptr: int, instances_ptr: int = 0, counts_ptr: int = 0,
                            max_hits: int = 8, stream_ptr: int = 0, max_leaf_tests: int = 10):
        """Asynchronous instanced all-hits queries on device memory of the set's device
        (shray_trace_instances_all_hits_device): `count` shray_ray records at `rays_ptr` -> count * max_hits shray_hit records
        at `hits_ptr` (0 iff max_hits is 0), unless `instances_ptr` is 0 count * max_hits int32 instance indices there, and
        unless `counts_ptr` is 0 `count` int32 crossing counts there, on a HIP stream (`stream_ptr`)."""
        mp = multihit_params(max_hits, max_leaf_tests)
        N.check(N.load_instance_multihit().shray_trace_instances_all_hits_device(
            self._handle, C.byref(mp), _ptr(rays_ptr), count, _ptr(hits_ptr), _ptr(instances_ptr), _ptr(counts_ptr), _ptr(stream_ptr)))

    def crossing_counts(self, rays, max_leaf_tests: int = 10):
        """How many surfaces each world ray crosses before its tmax over all instances (trace_all_hits with max_hits = 0):
        int32 [n], numpy for host rays, a tensor for GPU rays."""
        return self.trace_all_hits(rays, max_hits=0, counts=True, max_leaf_tests=max_leaf_tests)[2]

    def closest_points(self, points, max_dist2=None, counters: bool = False):
        """Instanced closest-point queries (include/shader_ray_instance_point.h): the nearest point of any instance's surface to
        each world-space point, measured on the instances' triangles mapped to the world by the set's object-to-world floats.
        `points` and `max_dist2` as for Scene.closest_points.  Host points take the blocking path and return (records:
        CLOSEST_DTYPE [n], instances: int32 [n]); a float32 [n, 3] / [n, 4] GPU tensor on the set's device takes the device
        path on the current torch stream and returns (int32 [n, 8] tensor of shray_closest records, int32 [n] tensor).  A miss
        has instance -1.  counters=True (host points only) also returns the walks' counters."""
        lib = N.load_instance_point()
        return _per_item(self._handle, (lib.shray_closest_points_instances_device, lib.shray_closest_points_instances,
                                        lib.shray_closest_points_instances_counters),
                         (), points, self._items("points", max_dist2), (), [_out(True, CLOSEST_DTYPE, 8), _out(True, np.int32)], counters)

    def closest_points_into(self, points_ptr: int, count: int, out_ptr: int, instances_ptr: int = 0, stream_ptr: int = 0):
        """Asynchronous instanced closest-point queries on device memory of the set's device
        (shray_closest_points_instances_device): `count` shray_point records at `points_ptr` -> `count` shray_closest records at
        `out_ptr` and, unless `instances_ptr` is 0, int32 instance indices there, on a HIP stream (`stream_ptr`)."""
        N.check(N.load_instance_point().shray_closest_points_instances_device(
            self._handle, _ptr(points_ptr), count, _ptr(out_ptr), _ptr(instances_ptr), _ptr(stream_ptr)))

    def signed_distance(self, points, max_dist2=None, closest: bool = False, counters: bool = False):
        """Instanced signed distances (include/shader_ray_instance_sdf.h): per world-space point the distance to the nearest
        instance's surface (closest_points' record), negative where the point lies inside that instance, the sign decided in
        the instance's object space with its member scene's pseudonormals; NaN for a point with nothing within its radius.
        `points` and `max_dist2` as for closest_points.  Host points take the blocking path and return float32 [n]; a float32
        [n, 3] / [n, 4] GPU tensor on the set's device takes the device path on the current torch stream and returns a float32
        [n] tensor.  With closest=True returns (values, records, instances), the last two as closest_points returns them.
        counters=True (host points only) also returns the counters of the sign walks, last."""
        lib = N.load_instance_sdf()
        out = _per_item(self._handle, (lib.shray_signed_distance_instances_device, lib.shray_signed_distance_instances,
                                       lib.shray_signed_distance_instances_counters),
                        (), points, self._items("points", max_dist2), (),
                        [_out(True, np.float32), _out(closest, CLOSEST_DTYPE, 8), _out(closest, np.int32)], counters)
        out = out if closest else out[:1] + out[3:]   # (values[, records, instances][, counters])
        return out if len(out) > 1 else out[0]

    def signed_distance_into(self, points_ptr: int, count: int, out_ptr: int, closest_ptr: int = 0, instances_ptr: int = 0,
                             stream_ptr: int = 0):
        """Asynchronous instanced signed distance queries on device memory of the set's device
        (shray_signed_distance_instances_device): `count` shray_point records at `points_ptr` -> `count` float32 at `out_ptr`,
        unless `closest_ptr` is 0 `count` shray_closest records there, and unless `instances_ptr` is 0 int32 instance indices
        there, on a HIP stream (`stream_ptr`)."""
        N.check(N.load_instance_sdf().shray_signed_distance_instances_device(
            self._handle, _ptr(points_ptr), count, _ptr(out_ptr), _ptr(closest_ptr), _ptr(instances_ptr), _ptr(stream_ptr)))

    def closed(self) -> bool:
        """Whether every member scene is closed (Scene.surface_info()["closed"]): what the sign's guarantee asks of them."""
        return all(bool(s.surface_info()["closed"]) for s in {id(s): s for s in self._scenes}.values())

    def winding_number(self, points, beta: float = 2.0, containing: bool = False):
        """Instanced winding numbers (include/shader_ray_instance_winding.h): per world-space point the sum over every instance
        of the member scene's winding number at the point mapped to object space, negated for a mirroring map: about 1 inside
        one closed outward-wound instance, 2 where two overlap, 0 outside all; NaN for a point with a non-finite coordinate.
        `points` and `beta` as for Scene.winding_number.  Host points take the blocking path and return float32 [n]; a GPU
        tensor on the set's device takes the device path on the current torch stream and returns a float32 [n] tensor.  With
        containing=True returns (values, int32 [n]): the lowest instance whose own term is above 0.5, or -1."""
        lib = N.load_instance_winding()
        out = _per_item(self._handle, (lib.shray_winding_number_instances_device, lib.shray_winding_number_instances, None), (), points,
                        self._items("points"), (beta,), [_out(True, np.float32), _out(containing, np.int32)])
        return out if containing else out[0]

    def winding_number_into(self, points_ptr: int, count: int, out_ptr: int, containing_ptr: int = 0, beta: float = 2.0,
                            stream_ptr: int = 0):
        """Asynchronous instanced winding numbers on device memory of the set's device (shray_winding_number_instances_device):
        `count` shray_point records at `points_ptr` -> `count` float32 at `out_ptr` and, unless `containing_ptr` is 0, int32
        containing instances there, on a HIP stream (`stream_ptr`)."""
        N.check(N.load_instance_winding().shray_winding_number_instances_device(
            self._handle, _ptr(points_ptr), count, beta, _ptr(out_ptr), _ptr(containing_ptr), _ptr(stream_ptr)))

    def winding_signed_distance(self, points, max_dist2=None, beta: float = 2.0, closest: bool = False):
        """Instanced signed distances whose sign comes from the summed winding number
        (shray_winding_signed_distance_instances): closest_points' record, negative where winding_number is above 0.5, the
        union's sign; NaN for a point with nothing within its radius.  Arguments and results as for signed_distance."""
        lib = N.load_instance_winding()
        out = _per_item(self._handle, (lib.shray_winding_signed_distance_instances_device, lib.shray_winding_signed_distance_instances, None),
                        (), points, self._items("points", max_dist2), (beta,),
                        [_out(True, np.float32), _out(closest, CLOSEST_DTYPE, 8), _out(closest, np.int32)])
        return out if closest else out[0]

    def winding_signed_distance_into(self, points_ptr: int, count: int, out_ptr: int, closest_ptr: int = 0, instances_ptr: int = 0,
                                     beta: float = 2.0, stream_ptr: int = 0):
        """Asynchronous instanced winding-signed distances on device memory of the set's device
        (shray_winding_signed_distance_instances_device), as signed_distance_into."""
        N.check(N.load_instance_winding().shray_winding_signed_distance_instances_device(
            self._handle, _ptr(points_ptr), count, beta, _ptr(out_ptr), _ptr(closest_ptr), _ptr(instances_ptr), _ptr(stream_ptr)))

    def orientations(self) -> np.ndarray:
        """The orientation of every instance's world-to-object map, float32 [n] of +1 or -1 (-1: a mirror), computed on the
        device as the winding queries compute it (shray_instance_set_orientations)."""
        out = np.zeros(self.count, np.float32)
        N.check(N.load_instance_winding().shray_instance_set_orientations(self._handle, out.ctypes.data_as(C.c_void_p)))
        return out

    def triangles_within(self, points, max_near: int = 8, counts: bool = True, counters: bool = False):
        """Instanced within-radius queries (include/shader_ray_instance_near.h): per world-space point the number of
        (instance, triangle) pairs whose closest point lies within its max_dist2, measured on the instances' triangles mapped
        to the world by the set's object-to-world floats, and the nearest `max_near` of them as shray_closest records, sorted
        by (dist2, instance, triangle), the other slots miss records with instance -1.  `points` as for
        Scene.triangles_within: host points take the blocking path and return (records: CLOSEST_DTYPE [n, max_near],
        instances: int32 [n, max_near], counts: int32 [n]); a float32 [n, 3] / [n, 4] GPU tensor on the set's device takes the
        device path on the current torch stream and returns (int32 [n, max_near, 8] tensor of shray_closest records, int32
        [n, max_near] tensor, int32 [n] tensor).  counts=False returns None for the counts and lets the walks skip what cannot
        reach the nearest `max_near` (the same records); max_near = 0 returns None for the records and instances.
        counters=True (host points only) also returns the counters of the walk that prunes only by max_dist2, summed over a
        point's walks."""
        lib = N.load_instance_near()
        return _first_k(self._handle, (lib.shray_near_triangles_instances_device, lib.shray_near_triangles_instances,
                                       lib.shray_near_triangles_instances_counters),
                        near_params(max_near), max_near, "max_near", points, self._items("points"), CLOSEST_DTYPE, (8,), True, counts, counters)

    def triangles_within_into(self, points_ptr: int, count: int, out_ptr: int, instances_ptr: int = 0, counts_ptr: int = 0,
                              max_near: int = 8, stream_ptr: int = 0):
        """Asynchronous instanced within-radius queries on device memory of the set's device
        (shray_near_triangles_instances_device): `count` shray_point records at `points_ptr` -> count * max_near shray_closest
        records at `out_ptr` (0 iff max_near is 0), unless `instances_ptr` is 0 count * max_near int32 instance indices there,
        and unless `counts_ptr` is 0 `count` int32 near counts there, on a HIP stream (`stream_ptr`)."""
        np_ = near_params(max_near)
        N.check(N.load_instance_near().shray_near_triangles_instances_device(
            self._handle, C.byref(np_), _ptr(points_ptr), count, _ptr(out_ptr), _ptr(instances_ptr), _ptr(counts_ptr), _ptr(stream_ptr)))

    def near_counts(self, points):
        """How many (instance, triangle) pairs lie within each world point's max_dist2 (triangles_within with max_near = 0):
        int32 [n], numpy for host points, a tensor for GPU points."""
        return self.triangles_within(points, max_near=0, counts=True)[2]

    def triangles_in_boxes(self, boxes, max_triangles: int = 8, counts: bool = True, counters: bool = False, any_only: bool = False):
        """Instanced box-overlap queries (include/shader_ray_instance_overlap.h): per axis-aligned world box the number of
        (instance, triangle) pairs that touch it, tested on the instances' triangles mapped to the world by the set's
        object-to-world floats, and the `max_triangles` smallest of them in (instance, triangle) order, the other slots
        SHRAY_HIT_MISS (-1) with instance -1.  `boxes` as for Scene.triangles_in_boxes: host boxes take the blocking path and
        return (indices: int32 [n, max_triangles], instances: int32 [n, max_triangles], counts: int32 [n]); a float32 [n, 6] /
        [n, 8] GPU tensor on the set's device takes the device path on the current torch stream and returns tensors of the
        same shapes.  counts=False returns None for the counts and lets a box that holds `max_triangles` pairs skip the
        instances above them (the same indices); max_triangles = 0 returns None for the indices and instances.  any_only=True
        (with max_triangles = 0) sets SHRAY_OVERLAP_ANY: the count is 1 or 0 and a box stops at its first touching pair.
        counters=True (host boxes only) also returns the counters of the walk that does not prune, summed over a box's walks."""
        lib = N.load_instance_overlap()
        return _first_k(self._handle, (lib.shray_overlap_triangles_instances_device, lib.shray_overlap_triangles_instances,
                                       lib.shray_overlap_triangles_instances_counters),
                        _set_overlap_params(max_triangles, any_only), max_triangles, "max_triangles", boxes, self._items("boxes"), np.int32, (),
                        True, counts, counters)

    def triangles_in_boxes_into(self, boxes_ptr: int, count: int, out_ptr: int, instances_ptr: int = 0, counts_ptr: int = 0,
                                max_triangles: int = 8, any_only: bool = False, stream_ptr: int = 0):
        """Asynchronous instanced box-overlap queries on device memory of the set's device
        (shray_overlap_triangles_instances_device): `count` shray_box records at `boxes_ptr` -> count * max_triangles int32
        triangle indices at `out_ptr` (0 iff max_triangles is 0), unless `instances_ptr` is 0 count * max_triangles int32
        instance indices there, and unless `counts_ptr` is 0 `count` int32 counts there, on a HIP stream (`stream_ptr`)."""
        op = _set_overlap_params(max_triangles, any_only)
        N.check(N.load_instance_overlap().shray_overlap_triangles_instances_device(
            self._handle, C.byref(op), _ptr(boxes_ptr), count, _ptr(out_ptr), _ptr(instances_ptr), _ptr(counts_ptr), _ptr(stream_ptr)))

    def box_counts(self, boxes):
        """How many (instance, triangle) pairs touch each world box (triangles_in_boxes with max_triangles = 0): int32 [n],
        numpy for host boxes, a tensor for GPU boxes."""
        return self.triangles_in_boxes(boxes, max_triangles=0, counts=True)[2]

    def boxes_touched(self, boxes):
        """Whether any triangle of any instance touches each world box (SHRAY_OVERLAP_ANY: a box stops at its first pair):
        bool [n], numpy for host boxes, a tensor for GPU boxes."""
        return self.triangles_in_boxes(boxes, max_triangles=0, counts=True, any_only=True)[2] != 0

    def surface_voxels(self, origin, cell, dims, device=None):
        """The occupancy grid of the placed surfaces: bool [nx, ny, nz], voxel (i, j, k) set iff a triangle of an instance
        touches the box of Scene.surface_voxels (voxel_boxes: the same planes, shared bit for bit by neighbours).  device=None
        builds the boxes with numpy and takes the host path; a torch device (the set's) builds them there and returns a
        tensor.  The query is boxes_touched."""
        boxes = voxel_boxes(origin, cell, dims, device)
        nx, ny, nz = (int(d) for d in dims)
        return self.boxes_touched(boxes).reshape(nx, ny, nz)

    def intersecting_triangles(self, triangles, max_triangles: int = 8, counts: bool = True, counters: bool = False, any_only: bool = False,
                               skip_shared: bool = False):
        """Instanced triangle-intersection queries (include/shader_ray_instance_intersect.h): per world query triangle the
        number of (instance, triangle) pairs it intersects, tested on the instances' triangles mapped to the world by the
        set's object-to-world floats, and the `max_triangles` smallest of them in (instance, triangle) order, the other slots
        SHRAY_HIT_MISS (-1) with instance -1.  `triangles` as for Scene.intersecting_triangles: host triangles take the
        blocking path and return (indices: int32 [n, max_triangles], instances: int32 [n, max_triangles], counts: int32 [n]);
        a float32 [n, 9] / [n, 12] GPU tensor on the set's device takes the device path on the current torch stream and
        returns tensors of the same shapes.  counts=False returns None for the counts and lets a query that holds
        `max_triangles` pairs skip the instances above them (the same indices); max_triangles = 0 returns None for the indices
        and instances.  any_only=True (with max_triangles = 0) sets SHRAY_INTERSECT_ANY: the count is 1 or 0 and a query stops
        at its first member.  skip_shared=True sets SHRAY_INTERSECT_SKIP_SHARED, judged on world corners.  counters=True (host
        triangles only) also returns the counters of the walk that does not prune, summed over a query's walks."""
        lib = N.load_instance_intersect()
        return _first_k(self._handle, (lib.shray_intersect_triangles_instances_device, lib.shray_intersect_triangles_instances,
                                       lib.shray_intersect_triangles_instances_counters),
                        _set_intersect_params(max_triangles, any_only, skip_shared), max_triangles, "max_triangles", triangles,
                        self._items("triangles"), np.int32, (), True, counts, counters)

    def intersecting_triangles_into(self, triangles_ptr: int, count: int, out_ptr: int, instances_ptr: int = 0, counts_ptr: int = 0,
                                    max_triangles: int = 8, any_only: bool = False, skip_shared: bool = False, stream_ptr: int = 0):
        """Asynchronous instanced triangle-intersection queries on device memory of the set's device
        (shray_intersect_triangles_instances_device): `count` shray_triangle records at `triangles_ptr` -> count *
        max_triangles int32 triangle indices at `out_ptr` (0 iff max_triangles is 0), unless `instances_ptr` is 0 count *
        max_triangles int32 instance indices there, and unless `counts_ptr` is 0 `count` int32 counts there, on a HIP stream
        (`stream_ptr`)."""
        op = _set_intersect_params(max_triangles, any_only, skip_shared)
        N.check(N.load_instance_intersect().shray_intersect_triangles_instances_device(
            self._handle, C.byref(op), _ptr(triangles_ptr), count, _ptr(out_ptr), _ptr(instances_ptr), _ptr(counts_ptr), _ptr(stream_ptr)))

    def intersection_counts(self, triangles, skip_shared: bool = False):
        """How many (instance, triangle) pairs each world query triangle intersects (intersecting_triangles with max_triangles
        = 0): int32 [n], numpy for host triangles, a tensor for GPU triangles."""
        return self.intersecting_triangles(triangles, max_triangles=0, counts=True, skip_shared=skip_shared)[2]

    def triangles_intersected(self, triangles, skip_shared: bool = False):
        """Whether each world query triangle intersects any triangle of any instance (SHRAY_INTERSECT_ANY: a query stops at its
        first member): bool [n], numpy for host triangles, a tensor for GPU triangles."""
        return self.intersecting_triangles(triangles, max_triangles=0, counts=True, any_only=True, skip_shared=skip_shared)[2] != 0

    def triangle_count(self, instance: int) -> int:
        """The number of triangles of instance `instance`'s scene."""
        if not 0 <= instance < self.count:
            raise ValueError(f"instance {instance} is not among the set's {self.count}")
        return self._scenes[instance].triangle_count()

    def _triangles_of(self, instance: int) -> int:
        """triangle_count, 0 for an instance that is not among the set's (the library refuses it)"""
        return self.triangle_count(instance) if 0 <= instance < self.count else 0

    def instance_intersections(self, instance: int, max_triangles: int = 8, counts: bool = True, any_only: bool = False,
                               skip_shared: bool = False, skip_own: bool = True, first: int = 0, count: int | None = None,
                               device: bool = False):
        """The instance form (shray_intersect_instance): the queries are the triangles [first, first + count) of instance
        `instance`'s scene (count=None: up to the last one) under that instance's current map, read on the device when the
        query runs.  Returns (indices: int32 [count, max_triangles], instances: int32 [count, max_triangles], counts: int32
        [count]) as numpy arrays from the blocking form, or with device=True as tensors on the set's device enqueued on the
        current torch stream (shray_intersect_instance_device).  skip_own defaults to True here
        (SHRAY_INTERSECT_SKIP_OWN_INSTANCE): no pair of instance `instance` itself is a member -- by its index, so a duplicate
        instance at the same place is found.  max_triangles = 0 returns None for the indices and instances, counts=False None
        for the counts; any_only and skip_shared as for intersecting_triangles."""
        lib = N.load_instance_intersect()
        return _own_triangles(self._handle, (lib.shray_intersect_instance_device, lib.shray_intersect_instance),
                              _set_intersect_params(max_triangles, any_only, skip_shared, skip_own), instance, first, count,
                              lambda: self._triangles_of(instance), max_triangles, "max_triangles", np.int32, (), counts, device,
                              lambda: self.device)

    def instance_intersections_into(self, instance: int, first: int, count: int, out_ptr: int, instances_ptr: int = 0,
                                    counts_ptr: int = 0, max_triangles: int = 8, any_only: bool = False, skip_shared: bool = False,
                                    skip_own: bool = True, stream_ptr: int = 0):
        """Asynchronous instance form (shray_intersect_instance_device): the triangles [first, first + count) of instance
        `instance` -> count * max_triangles int32 triangle indices at `out_ptr` (0 iff max_triangles is 0), unless
        `instances_ptr` is 0 as many instance indices there, and unless `counts_ptr` is 0 `count` int32 counts there, device
        memory of the set's device, on a HIP stream (`stream_ptr`)."""
        op = _set_intersect_params(max_triangles, any_only, skip_shared, skip_own)
        N.check(N.load_instance_intersect().shray_intersect_instance_device(
            self._handle, C.byref(op), instance, first, count, _ptr(out_ptr), _ptr(instances_ptr), _ptr(counts_ptr), _ptr(stream_ptr)))

    def instances_colliding(self) -> np.ndarray:
        """bool [n]: instance i has a triangle that intersects a triangle of another instance (one SHRAY_INTERSECT_ANY |
        SHRAY_INTERSECT_SKIP_OWN_INSTANCE launch of the instance form per instance)."""
        return np.array([bool(self.instance_intersections(i, max_triangles=0, counts=True, any_only=True)[2].any())
                         for i in range(self.count)], bool)

    def _pair_rows(self, rows):
        """(first_row, row_count) of `rows`: None (every instance), a (first_row, row_count) pair, or a range of step 1"""
        if rows is None:
            return 0, self.count
        if isinstance(rows, range):
            if rows.step != 1:
                raise ValueError("rows must be a range of step 1")
            return rows.start, len(rows)
        first_row, row_count = rows
        return int(first_row), int(row_count)

    def collision_matrix(self, rows=None, upper: bool = False, skip_shared: bool = False) -> np.ndarray:
        """Which placed parts collide, and with which other part (include/shader_ray_instance_pairs.h, SHRAY_PAIRS_ANY): bool
        [r, n], entry (a - first_row, b) set iff a triangle of instance a, as the query, intersects a triangle of instance b;
        one launch for all the rows.  `rows`: None for every instance, else (first_row, row_count) or a range.  The matrix is
        ordered (the per-pair test is not symmetric in fp32) and its diagonal is False; upper=True asks for the cells with b >
        a only, skip_shared=True sets SHRAY_PAIRS_SKIP_SHARED."""
        first_row, row_count = self._pair_rows(rows)
        ok = first_row >= 0 and row_count >= 0 and first_row + row_count <= self.count   # (the library refuses any other range)
        cells = np.empty((row_count if ok else 0, self.count), np.int64)
        op = _pairs_params(first_row, row_count, True, upper, skip_shared)
        N.check(N.load_instance_pairs().shray_instance_pairs_intersect(self._handle, C.byref(op), None, cells.ctypes.data_as(C.c_void_p)))
        return cells != 0

    def collision_pairs(self, rows=None, counts: bool = True, upper: bool = False, skip_shared: bool = False, counters: bool = False,
                        device: bool = False):
        """The collision matrix with its witnesses (include/shader_ray_instance_pairs.h): (triangle_a: int32 [r, n],
        triangle_b: int32 [r, n], counts: int64 [r, n]).  Cell (a - first_row, b) holds the number of pairs (triangle ta of
        instance a as the query, triangle tb of instance b) that intersect, and the lexicographically smallest such (ta, tb),
        -1 and -1 where there is none.  counts=False returns None for the counts and lets the walk skip what cannot lower a
        cell's pair.  Numpy arrays from the blocking form, or with device=True tensors on the set's device enqueued on the
        current torch stream.  counters=True (the blocking form only) also returns the counters of the walk that skips
        nothing by what a cell already holds.  `rows`, upper and skip_shared as for collision_matrix."""
        first_row, row_count = self._pair_rows(rows)
        ok = first_row >= 0 and row_count >= 0 and first_row + row_count <= self.count   # (the library refuses any other range)
        r, n = (row_count if ok else 0), self.count
        op = _pairs_params(first_row, row_count, False, upper, skip_shared)
        lib = N.load_instance_pairs()
        if device:
            import torch
            if counters:
                raise ValueError("counters are counted on the host path: pass device=False")
            where = torch.device("cuda", self.device)
            # (an empty tensor has no pointer: one cell is allocated for an empty range)
            new = lambda want: torch.empty(max(r * n, 1), dtype=torch.int64, device=where) if want else None
            keys, cnt = new(True), new(counts)
            N.check(lib.shray_instance_pairs_intersect_device(self._handle, C.byref(op), C.c_void_p(keys.data_ptr()),
                                                              C.c_void_p(cnt.data_ptr() if counts else None),
                                                              C.c_void_p(torch.cuda.current_stream(where).cuda_stream)))
            keys = keys[:r * n].reshape(r, n)       # (SHRAY_PAIRS_NONE is -1 as an int64: both halves come out -1)
            return (keys >> 32).to(torch.int32), (keys & 0xFFFFFFFF).to(torch.int32), (cnt[:r * n].reshape(r, n) if counts else None)
        keys = np.empty((r, n), np.uint64)
        cnt = np.empty((r, n), np.int64) if counts else None
        args = (self._handle, C.byref(op), keys.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p) if counts else None)
        tally = N.Counters()
        N.check(lib.shray_instance_pairs_intersect_counters(*args, C.byref(tally)) if counters else lib.shray_instance_pairs_intersect(*args))
        out = ((keys >> np.uint64(32)).astype(np.uint32).view(np.int32), (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32), cnt)
        return (*out, tally.as_dict()) if counters else out

    def collision_pairs_into(self, first_ptr: int, counts_ptr: int, first_row: int = 0, row_count: int | None = None,
                             any_only: bool = False, upper: bool = False, skip_shared: bool = False, stream_ptr: int = 0):
        """Asynchronous collision matrix on device memory of the set's device (shray_instance_pairs_intersect_device): the
        rows [first_row, first_row + row_count) (row_count=None: up to the last instance) -> row_count * n uint64 keys (ta <<
        32 | tb, all ones where none) at `first_ptr` unless it is 0, and row_count * n int64 counts at `counts_ptr` unless it is
        0, on a HIP stream (`stream_ptr`).  The call initialises the cells itself.  any_only=True (with first_ptr 0) writes 1
        or 0 into the counts."""
        if row_count is None:
            row_count = max(self.count - first_row, 0)
        op = _pairs_params(first_row, row_count, any_only, upper, skip_shared)
        N.check(N.load_instance_pairs().shray_instance_pairs_intersect_device(
            self._handle, C.byref(op), _ptr(first_ptr), _ptr(counts_ptr), _ptr(stream_ptr)))

    def colliding_pairs(self, upper: bool = True) -> np.ndarray:
        """int32 [m, 2]: the set cells (a, b) of collision_matrix in row-major order; with upper=True (the default) every
        unordered pair is asked once, as (a, b) with a < b and instance a's triangles as the queries."""
        return np.argwhere(self.collision_matrix(upper=upper)).astype(np.int32).reshape(-1, 2)

    def triangle_distances(self, triangles, max_dist2: float = float("inf"), max_pairs: int = 1, counts: bool = True, counters: bool = False,
                           skip_shared: bool = False, any_only: bool = False):
        """Instanced triangle-distance queries (include/shader_ray_instance_clearance.h): per world query triangle the number
        of (instance, triangle) pairs whose squared distance to it is at most `max_dist2`, computed on the instances'
        triangles mapped to the world by the set's object-to-world floats, and the `max_pairs` nearest of them in (dist2,
        instance, triangle) order as PAIR_DISTANCE_DTYPE records (world witnesses and dist2, the member scene's own triangle
        index), the other slots miss records (triangle -1) with instance -1.  `triangles` as for Scene.triangle_distances:
        host triangles take the blocking path and return (records: PAIR_DISTANCE_DTYPE [n, max_pairs], instances: int32 [n,
        max_pairs], counts: int32 [n]); a float32 [n, 9] / [n, 12] GPU tensor on the set's device takes the device path on the
        current torch stream and returns the records as an int32 [n, max_pairs, 12] tensor and the others as tensors.
        counts=False returns None for the counts and lets the walk skip what cannot reach the nearest `max_pairs`; max_pairs
        = 0 returns None for the records and instances.  skip_shared=True sets SHRAY_CLEARANCE_SKIP_SHARED, judged on world
        corners; any_only=True (with max_pairs = 0) SHRAY_CLEARANCE_ANY.  counters=True (host triangles only) also returns the
        counters of the walk that prunes by max_dist2 only, summed over a query's walks."""
        lib = N.load_instance_clearance()
        return _first_k(self._handle, (lib.shray_clearance_triangles_instances_device, lib.shray_clearance_triangles_instances,
                                       lib.shray_clearance_triangles_instances_counters),
                        _set_clearance_params(max_pairs, max_dist2, any_only, skip_shared), max_pairs, "max_pairs", triangles,
                        self._items("triangles"), PAIR_DISTANCE_DTYPE, (12,), True, counts, counters)

    def triangle_distances_into(self, triangles_ptr: int, count: int, out_ptr: int, instances_ptr: int = 0, counts_ptr: int = 0,
                                max_dist2: float = float("inf"), max_pairs: int = 1, any_only: bool = False, skip_shared: bool = False,
                                stream_ptr: int = 0):
        """Asynchronous instanced triangle-distance queries on device memory of the set's device
        (shray_clearance_triangles_instances_device): `count` shray_triangle records at `triangles_ptr` -> count * max_pairs
        shray_pair_distance records at `out_ptr` (0 iff max_pairs is 0), unless `instances_ptr` is 0 count * max_pairs int32
        instance indices there, and unless `counts_ptr` is 0 `count` int32 counts there, on a HIP stream (`stream_ptr`)."""
        op = _set_clearance_params(max_pairs, max_dist2, any_only, skip_shared)
        N.check(N.load_instance_clearance().shray_clearance_triangles_instances_device(
            self._handle, C.byref(op), _ptr(triangles_ptr), count, _ptr(out_ptr), _ptr(instances_ptr), _ptr(counts_ptr), _ptr(stream_ptr)))

    def clearance_counts(self, triangles, max_dist2: float, skip_shared: bool = False):
        """How many (instance, triangle) pairs lie within `max_dist2` of each world query triangle (triangle_distances with
        max_pairs = 0): int32 [n], numpy for host triangles, a tensor for GPU triangles."""
        return self.triangle_distances(triangles, max_dist2, max_pairs=0, counts=True, skip_shared=skip_shared)[2]

    def within_tolerance(self, triangles, max_dist2: float, skip_shared: bool = False):
        """Whether any triangle of any instance lies within `max_dist2` of each world query triangle (SHRAY_CLEARANCE_ANY: a
        query stops at its first member): bool [n], numpy for host triangles, a tensor for GPU triangles."""
        return self.triangle_distances(triangles, max_dist2, max_pairs=0, counts=True, skip_shared=skip_shared, any_only=True)[2] != 0

    def instance_clearance(self, instance: int, max_dist2: float = float("inf"), max_pairs: int = 1, skip_shared: bool = False,
                           skip_own: bool = True, first: int = 0, count: int | None = None, counts: bool = True, any_only: bool = False,
                           device: bool = False):
        """The instance form (shray_clearance_instance): the queries are the triangles [first, first + count) of instance
        `instance`'s scene (count=None: up to the last one) under that instance's current map, read on the device when the
        query runs.  Returns (records: PAIR_DISTANCE_DTYPE [count, max_pairs], instances: int32 [count, max_pairs], counts:
        int32 [count]) as numpy arrays from the blocking form, or with device=True as tensors on the set's device (the records
        int32 [count, max_pairs, 12]) enqueued on the current torch stream (shray_clearance_instance_device).  skip_own
        defaults to True here (SHRAY_CLEARANCE_SKIP_OWN_INSTANCE): no pair of instance `instance` itself is a member -- by its
        index, so a duplicate instance at the same place is found at distance 0.  max_pairs = 0 returns None for the records
        and instances, counts=False None for the counts; any_only and skip_shared as for triangle_distances."""
        lib = N.load_instance_clearance()
        return _own_triangles(self._handle, (lib.shray_clearance_instance_device, lib.shray_clearance_instance),
                              _set_clearance_params(max_pairs, max_dist2, any_only, skip_shared, skip_own), instance, first, count,
                              lambda: self._triangles_of(instance), max_pairs, "max_pairs", PAIR_DISTANCE_DTYPE, (12,), counts, device,
                              lambda: self.device)

    def instance_clearance_into(self, instance: int, first: int, count: int, out_ptr: int, instances_ptr: int = 0, counts_ptr: int = 0,
                                max_dist2: float = float("inf"), max_pairs: int = 1, any_only: bool = False, skip_shared: bool = False,
                                skip_own: bool = True, stream_ptr: int = 0):
        """Asynchronous instance form (shray_clearance_instance_device): the triangles [first, first + count) of instance
        `instance` -> count * max_pairs shray_pair_distance records at `out_ptr` (0 iff max_pairs is 0), unless
        `instances_ptr` is 0 as many int32 instance indices there, and unless `counts_ptr` is 0 `count` int32 counts there,
        device memory of the set's device, on a HIP stream (`stream_ptr`)."""
        op = _set_clearance_params(max_pairs, max_dist2, any_only, skip_shared, skip_own)
        N.check(N.load_instance_clearance().shray_clearance_instance_device(
            self._handle, C.byref(op), instance, first, count, _ptr(out_ptr), _ptr(instances_ptr), _ptr(counts_ptr), _ptr(stream_ptr)))

    def instances_within(self, max_dist2: float) -> np.ndarray:
        """bool [n]: instance i has a triangle within `max_dist2` of a triangle of another instance (one SHRAY_CLEARANCE_ANY |
        SHRAY_CLEARANCE_SKIP_OWN_INSTANCE launch of the instance form per instance)."""
        return np.array([bool(self.instance_clearance(i, max_dist2, max_pairs=0, counts=True, any_only=True)[2].any())
                         for i in range(self.count)], bool)

    def instance_distance(self, instance: int, max_dist2: float = float("inf"), max_pairs: int = 1, counts: bool = True,
                          skip_shared: bool = False):
        """Instance `instance` against the rest of the set: the blocking instance form with SHRAY_CLEARANCE_SKIP_OWN_INSTANCE over
        all of its triangles.  Returns (records, instances, counts, minimum): instance_clearance's arrays, and the smallest
        dist2 of any pair within `max_dist2` (0 where the instance interpenetrates another, +inf where no pair is that near)
        -- the clearance of the instance from the others, squared; reduced on the host as Scene.distance_to does."""
        if max_pairs < 1:
            raise ValueError("instance_distance needs max_pairs >= 1: the minimum is read from each query's first record")
        records, inst, n = self.instance_clearance(instance, max_dist2, max_pairs=max_pairs, skip_shared=skip_shared, counts=counts)
        found = records[:, 0][records[:, 0]["triangle"] >= 0]
        return records, inst, n, float(found["dist2"].min()) if len(found) else float("inf")

    def close(self):
        if getattr(self, "_handle", None):
            self._lib.shray_instance_set_destroy(self._handle)
            self._handle = None
        self._scenes = []
        self._owners = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PinnedFrame:
    """RGBA float32 [height, width, 4] in pinned host memory (shray_pinned_alloc): the destination of the
    PCIe-speed readback forms."""

    def __init__(self, width: int, height: int):
        self._lib = N.load_hip()
        p = C.c_void_p()
        N.check(self._lib.shray_pinned_alloc(width * height * 16, C.byref(p)))
        self.ptr = p.value
        self.array = np.ctypeslib.as_array((C.c_float * (width * height * 4)).from_address(self.ptr)).reshape(height, width, 4)

    def close(self):
        if getattr(self, "ptr", None):
            self.array = None
            self._lib.shray_pinned_free(C.c_void_p(self.ptr))
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def tile_buffer_bytes(width: int, height: int, tiles: N.TileSet | None) -> int:
    return int(N.load_hip().shray_tile_buffer_bytes(width, height, C.byref(tiles) if tiles is not None else None))


def algorithmic_bytes(counters: dict, pixels: int, normals_fp16: bool = True, out_bytes: int = 16) -> int:
    """Cache-less byte count of the reference's own fetches:
    32 B per node visit (24 B box + 8 B links), +8 B per leaf visit (start, count),
    36 B per triangle test (3 x 12 B), 18 B per shaded hit (3 fp16 normals; 36 B if
    fp32), 48 B per environment lookup (4 texels x 12 B), 16 B per output pixel."""
    c = counters
    return (32 * c["node_visits"] + 8 * c["leaf_visits"] + 36 * c["triangle_tests"]
            + (18 if normals_fp16 else 36) * c["shaded_hits"] + 48 * c["env_lookups"] + out_bytes * pixels)
