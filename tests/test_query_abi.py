"""The ray-query and instanced-query entry points (include/shader_ray_query.h, include/shader_ray_instance.h) refuse bad
arguments before they touch the scene or set handle, treat count 0 as a no-op, and zero the caller's counters first."""
import ctypes as C

import numpy as np


def test_trace_argument_errors(pkg):
    """NULL pointers, bad query params, a negative count and misaligned device buffers fail with SHRAY_ERR_INVALID_ARGUMENT;
    count 0 with valid pointers is a no-op that needs no scene, set or device, and leaves the counters zeroed."""
    N = pkg._native
    query, instance = N.load_query(), N.load_instance()
    qp, bad_size, bad_range = N.QueryParams(), N.QueryParams(), N.QueryParams()
    for p in (qp, bad_size, bad_range):
        query.shray_query_params_init(C.byref(p))
    bad_size.struct_size += 4
    bad_range.any_hit = 2
    q = C.byref(qp)
    rays, hits, inst, c = (N.Ray * 2)(), (N.Hit * 2)(), (C.c_int32 * 2)(), N.Counters()
    buf = np.zeros(64, np.uint8)
    base = (buf.ctypes.data + 15) & ~15
    dev = C.c_void_p(base)
    fake = C.c_void_p(1)   # never read: every call below is refused (or a no-op) before the handle is touched
    cases = []
    for lib, trace, out, d_out in ((query, "shray_trace_rays", (), ()), (instance, "shray_trace_instances", (inst,), (dev,))):
        host, counted, device = (getattr(lib, trace + suffix) for suffix in ("", "_counters", "_device"))
        cases += [
            (host, fake, None, rays, 2, hits, *out),
            (host, fake, C.byref(bad_size), rays, 2, hits, *out),
            (host, fake, C.byref(bad_range), rays, 2, hits, *out),
            (host, None, q, rays, 2, hits, *out),
            (host, fake, q, None, 2, hits, *out),
            (host, fake, q, rays, 2, None, *out),
            (host, fake, q, rays, -1, hits, *out),
            (counted, fake, q, rays, 2, hits, *out, None),
            (counted, fake, None, rays, 2, hits, *out, C.byref(c)),
            (counted, None, q, rays, 2, hits, *out, C.byref(c)),
            (counted, fake, q, None, 2, hits, *out, C.byref(c)),
            (counted, fake, q, rays, -3, hits, *out, C.byref(c)),
            (device, fake, None, dev, 1, dev, *d_out, None),
            (device, None, q, dev, 1, dev, *d_out, None),
            (device, fake, q, None, 1, dev, *d_out, None),
            (device, fake, q, dev, 1, None, *d_out, None),
            (device, fake, q, dev, -1, dev, *d_out, None),
            (device, fake, q, C.c_void_p(base + 4), 1, dev, *d_out, None),
            (device, fake, q, dev, 1, C.c_void_p(base + 8), *d_out, None),
        ]
    cases.append((instance.shray_trace_instances_device, fake, q, dev, 1, dev, C.c_void_p(base + 2), None))
    for k, (fn, *args) in enumerate(cases):
        assert fn(*args) == -1, (k, fn.__name__)
        assert N.load_hip().shray_last_error(), (k, fn.__name__)

    assert query.shray_trace_rays(fake, q, rays, 0, hits) == 0
    assert query.shray_trace_rays_device(fake, q, dev, 0, dev, None) == 0
    assert instance.shray_trace_instances(fake, q, rays, 0, hits, None) == 0
    assert instance.shray_trace_instances(fake, q, rays, 0, hits, inst) == 0
    assert instance.shray_trace_instances_device(fake, q, dev, 0, dev, None, None) == 0
    for counted, args in ((query.shray_trace_rays_counters, (None,)), (instance.shray_trace_instances_counters, (None, None))):
        c.samples, c.node_visits, c.bad_hits = 99, 5, 7
        assert counted(fake, q, rays, 0, *args, C.byref(c)) == 0
        assert c.as_dict() == dict.fromkeys(c.as_dict(), 0)
