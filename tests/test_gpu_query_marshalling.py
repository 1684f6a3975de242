"""The one marshalling path of the Python query bindings (tracer._per_item, tracer._own_triangles) on the GPU: for the eight
point-family methods, four first-K methods and the four range forms, on the 528-triangle lobed mesh as one scene and as a set of
two instances of it, the result from a GPU tensor equals the result from numpy byte for byte -- from the C layouts and from the
short forms [n, 3] / [n, 6] / [n, 9] -- once on torch's default stream and once inside torch.cuda.stream(side_stream).  Five
points, boxes, triangles and rays drawn with a fixed seed inside the scene's bounds.  The Scene range forms on the device answer
an empty range with empty tensors and a refused range with the host form's range error."""
import numpy as np
import pytest

from test_gpu_point_query import loaded

pytestmark = pytest.mark.gpu

F = np.float32
N_ITEMS = 5
_made = {}


@pytest.fixture(scope="module")
def world(pkg, gpu):
    """(tracer, the scene, a set of two instances of it, the items by kind: {kind: (short form, C layout)} float32 arrays, the
    squared radius the distance queries use)"""
    T = pkg.tracer
    arrays, scene = loaded(pkg, "lobed_528")
    verts = np.asarray(arrays["vertex_positions"], F).reshape(-1, 3)
    lo, hi = verts.min(0), verts.max(0)
    maps = np.tile(np.eye(3, 4, dtype=F), (2, 1, 1))
    maps[1, :, 3] = (hi - lo) * F(0.25)
    group = _made["set"] = T.InstanceSet([scene, scene], maps)
    rng = np.random.default_rng(528)
    inside = lambda *shape: (lo + rng.random((*shape, 3)) * (hi - lo)).astype(F)
    points = inside(N_ITEMS)
    corners = np.sort(inside(N_ITEMS, 2), axis=1)
    direction = rng.normal(size=(N_ITEMS, 3)).astype(F)
    rays = np.concatenate([inside(N_ITEMS), direction], axis=1)
    triangles = inside(N_ITEMS, 3).reshape(N_ITEMS, 9)
    layout = lambda records: np.ascontiguousarray(records).view(F).reshape(N_ITEMS, -1)
    items = {"points": (points, layout(T.make_points(points))),
             "boxes": (corners.reshape(N_ITEMS, 6), layout(T.make_boxes(corners[:, 0], corners[:, 1]))),
             "triangles": (triangles, layout(T.make_triangles(triangles))),
             "rays": (rays, layout(T.make_rays(rays[:, 0:3], rays[:, 3:6])))}
    yield T, scene, group, items, float(((hi - lo) ** 2).sum()) * 0.04
    _made.pop("set").close()


def raw(value):
    """a result as bytes (a tensor by way of the host), None as None, a tuple member by member"""
    if isinstance(value, tuple):
        return tuple(raw(v) for v in value)
    if value is None:
        return None
    return np.ascontiguousarray(value if isinstance(value, np.ndarray) else value.cpu().numpy()).tobytes()


def queries(scene, group, radius2):
    """(name, kind of items, the call) of every method under test"""
    return [
        ("Scene.closest_points", "points", lambda p: scene.closest_points(p)),
        ("Scene.closest_points, max_dist2", "points", lambda p: scene.closest_points(p, max_dist2=radius2)),
        ("Scene.signed_distance", "points", lambda p: scene.signed_distance(p, closest=True)),
        ("Scene.signed_distance, values only", "points", lambda p: scene.signed_distance(p, max_dist2=radius2)),
        ("Scene.winding_number", "points", lambda p: scene.winding_number(p)),
        ("Scene.winding_signed_distance", "points", lambda p: scene.winding_signed_distance(p, beta=1.5, closest=True)),
        ("InstanceSet.closest_points", "points", lambda p: group.closest_points(p, max_dist2=radius2)),
        ("InstanceSet.signed_distance", "points", lambda p: group.signed_distance(p, closest=True)),
        ("InstanceSet.signed_distance, values only", "points", lambda p: group.signed_distance(p)),
        ("InstanceSet.winding_number", "points", lambda p: group.winding_number(p, containing=True)),
        ("InstanceSet.winding_signed_distance", "points", lambda p: group.winding_signed_distance(p, max_dist2=radius2, closest=True)),
        ("Scene.triangles_within", "points", lambda p: scene.triangles_within(p, max_near=3)),
        ("Scene.intersecting_triangles", "triangles", lambda t: scene.intersecting_triangles(t, max_triangles=3)),
        ("Scene.triangle_distances", "triangles", lambda t: scene.triangle_distances(t, radius2, max_pairs=2, counts=False)),
        ("InstanceSet.triangles_in_boxes", "boxes", lambda b: group.triangles_in_boxes(b, max_triangles=3)),
        ("InstanceSet.trace_all_hits", "rays", lambda r: group.trace_all_hits(r, max_hits=3)),
    ]


def range_forms(scene, group, radius2, **where):
    """(name, the call with device=False / True) of the four range forms over `where` (first, count)"""
    return [
        ("Scene.self_intersections", lambda device: scene.self_intersections(max_triangles=2, device=device, **where)),
        ("Scene.self_clearance", lambda device: scene.self_clearance(radius2, max_pairs=2, device=device, **where)),
        ("InstanceSet.instance_intersections", lambda device: group.instance_intersections(1, max_triangles=2, device=device, **where)),
        ("InstanceSet.instance_clearance", lambda device: group.instance_clearance(1, radius2, max_pairs=2, device=device, **where)),
    ]


@pytest.mark.parametrize("stream", ("default", "side"))
def test_a_gpu_tensor_and_numpy_give_the_same_bytes(world, stream):
    import torch
    T, scene, group, items, radius2 = world
    with torch.cuda.stream(torch.cuda.Stream() if stream == "side" else torch.cuda.current_stream()):
        for name, kind, call in queries(scene, group, radius2):
            short, c_layout = items[kind]
            want = call(c_layout)
            assert not any(isinstance(v, torch.Tensor) for v in (want if isinstance(want, tuple) else (want,))), name
            assert raw(call(short)) == raw(want), f"{name}: numpy, the short form"
            got = call(torch.from_numpy(c_layout).cuda())
            assert all(v is None or v.is_cuda for v in (got if isinstance(got, tuple) else (got,))), name
            assert raw(got) == raw(want), f"{name}: a GPU tensor, the C layout"
            if kind != "rays":   # (a GPU ray tensor has the C layout only)
                assert raw(call(torch.from_numpy(short).cuda())) == raw(want), f"{name}: a GPU tensor, the short form"
        for name, call in range_forms(scene, group, radius2, first=7, count=20):
            want, got = call(False), call(True)
            assert all(v.is_cuda and len(v) == 20 for v in got), name
            assert raw(got) == raw(want), name
        torch.cuda.current_stream().synchronize()


def test_the_scene_range_forms_answer_an_empty_range_on_the_device(world):
    import torch
    T, scene, group, items, radius2 = world
    out, n = scene.self_intersections(first=7, count=0, device=True)
    assert out.is_cuda and out.dtype == torch.int32 and tuple(out.shape) == (0, 8) and tuple(n.shape) == (0,)
    out, n = scene.self_clearance(first=7, count=0, device=True)
    assert out.is_cuda and out.dtype == torch.int32 and tuple(out.shape) == (0, 1, 12) and tuple(n.shape) == (0,)
    for name, call in range_forms(scene, group, radius2, first=scene.triangle_count(), count=None):   # the empty range at the end
        want, got = call(False), call(True)
        as_tensors = [v.shape + ((12,) if v.dtype == T.PAIR_DISTANCE_DTYPE else ()) for v in want]   # (a record is 12 int32)
        assert [tuple(v.shape) for v in got] == as_tensors and all(v.is_cuda and len(v) == 0 for v in got), name


def test_the_scene_range_forms_report_a_refused_range_as_the_range_on_the_device(pkg, world):
    T, scene, group, items, radius2 = world
    triangles = scene.triangle_count()
    for name, call in range_forms(scene, group, radius2, first=triangles, count=1):
        with pytest.raises(pkg._native.ShrayError) as on_host:
            call(False)
        with pytest.raises(pkg._native.ShrayError) as on_device:
            call(True)
        assert on_device.value.code == on_host.value.code == -1, name   # SHRAY_ERR_INVALID_ARGUMENT
        assert str(on_device.value) == str(on_host.value), name
        assert f"{triangles} .. {triangles + 1}" in str(on_device.value) and str(triangles) in str(on_device.value), name
