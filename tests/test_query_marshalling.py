"""What the host path of every query method of Scene and InstanceSet hands the C library, and what it returns, checked without a
device and without a built library: the objects are made with object.__new__ and a fake handle, and every N.load_* function
returns a stand-in whose attributes record (function name, arguments) and return 0.  Per case: which C function is called, the
scalar arguments, the items as the library would read them, each output pointer (the address of the returned array of the
stated dtype and shape, or NULL exactly where the contract says None), and the arity and order of the returned tuple."""
import ctypes as C

import numpy as np
import pytest

SCENE_HANDLE, SET_HANDLE = 0x5CE0E, 0x5E7
TRIANGLES = 5      # what the stand-in's shray_scene_geometry_counts reports: 3 x 5 corners
ITEMS, COUNTERS = "items", "counters"
TALLY = {"node_visits": 7, "traversals": 3}   # what the stand-in's counters forms count

RNG = np.random.default_rng(20261021)
POINTS = RNG.uniform(-1, 1, (3, 3)).astype(np.float32)
RAYS = RNG.uniform(-1, 1, (3, 6)).astype(np.float32)
BOXES = np.sort(RNG.uniform(-1, 1, (3, 2, 3)).astype(np.float32), axis=1).reshape(3, 6)
CORNERS = RNG.uniform(-1, 1, (3, 9)).astype(np.float32)


class StandIn:
    """A library: every attribute is a C function that records (name, arguments) and returns 0.  The params initialisers are
    not recorded, shray_scene_geometry_counts reports TRIANGLES triangles, a trailing shray_counters is filled with TALLY, and
    the bytes at the pointer argument `peek` = (index, bytes) are kept while the caller's array is still alive."""

    def __init__(self, counters_type):
        self.calls, self.peek, self.seen, self.counters_type = [], None, None, counters_type

    def __getattr__(self, name):
        def function(*args):
            if name.endswith("_params_init"):
                return 0
            if name == "shray_scene_geometry_counts":
                if args[1] is not None:
                    args[1]._obj.value = 3 * TRIANGLES
                return 0
            tally = getattr(args[-1], "_obj", None) if args else None
            if isinstance(tally, self.counters_type):
                for key, value in TALLY.items():
                    setattr(tally, key, value)
            self.calls.append((name, args))
            if self.peek is not None:
                self.seen = C.string_at(address(args[self.peek[0]]), self.peek[1])
            return 0
        return function


def address(pointer):
    """a pointer argument as an int, None for NULL"""
    return pointer.value if isinstance(pointer, C.c_void_p) else pointer


@pytest.fixture
def world(monkeypatch):
    """(tracer module, stand-in library, a Scene, an InstanceSet of two of it)"""
    from __graft_entry__ import load_package
    pkg = load_package()
    T, N = pkg.tracer, pkg._native
    lib = StandIn(N.Counters)
    for name in dir(N):
        if name.startswith("load_"):
            monkeypatch.setattr(N, name, lambda: lib)
    scene = object.__new__(T.Scene)
    scene._lib, scene._handle = lib, C.c_void_p(SCENE_HANDLE)
    group = object.__new__(T.InstanceSet)
    group._lib, group._handle, group.count, group.device = lib, C.c_void_p(SET_HANDLE), 2, 0
    group._scenes = group._owners = [scene, scene]
    yield T, lib, scene, group
    scene._handle = group._handle = None   # (nothing for __del__ to destroy)


def dtype_of(T, name):
    return {"hit": T.HIT_DTYPE, "closest": T.CLOSEST_DTYPE, "pair": T.PAIR_DISTANCE_DTYPE, "f32": np.dtype(np.float32),
            "i32": np.dtype(np.int32)}[name]


def items_of(T, kind, replace=None):
    """the three items of `kind` as the method is given them, and as the library is to read them"""
    if kind == "points":
        return POINTS, T.make_points(POINTS, replace)
    if kind == "rays":
        return RAYS, T.make_rays(RAYS[:, 0:3], RAYS[:, 3:6], replace)
    if kind == "boxes":
        return BOXES, T.make_boxes(BOXES[:, 0:3], BOXES[:, 3:6])
    return CORNERS, T.make_triangles(CORNERS)


def check(T, lib, handle, got, function, middle, outs, layout, rows=3, items_bytes=None):
    """One recorded call of `function`: (handle, *middle, *output pointers[, counters]).  `middle`: ITEMS (the pointer whose
    bytes were peeked), a number, or (params type name, {field: value}).  `outs`: per output pointer (dtype name, shape per
    row) or None for NULL.  `layout`: the returned value, an index into `outs` for a bare array, or a list of such indices and
    COUNTERS for a tuple in that order."""
    (name, args), = lib.calls
    assert name == function
    assert address(args[0]) == handle
    with_counters = COUNTERS in layout if isinstance(layout, list) else False
    assert len(args) == 1 + len(middle) + len(outs) + (1 if with_counters else 0)
    for want, arg in zip(middle, args[1:]):
        if want is ITEMS:
            assert lib.seen == items_bytes
        elif isinstance(want, tuple):
            params = arg._obj
            assert type(params).__name__ == want[0]
            for field, value in want[1].items():
                assert getattr(params, field) == value, field
        else:
            assert arg == want and type(arg) is type(want)
    if isinstance(layout, list):
        assert type(got) is tuple and len(got) == len(layout)
    else:
        got, layout = (got,), [layout]
    pointers = args[1 + len(middle):1 + len(middle) + len(outs)]
    returned = {slot: value for slot, value in zip(layout, got)}
    for i, (spec, pointer) in enumerate(zip(outs, pointers)):
        if spec is None:
            assert address(pointer) is None
            assert returned.get(i, None) is None
            continue
        array = returned[i]   # (every array the library fills is returned)
        assert isinstance(array, np.ndarray) and array.dtype == dtype_of(T, spec[0]) and array.shape == (rows, *spec[1])
        assert array.flags.c_contiguous and address(pointer) == array.ctypes.data
    if with_counters:
        assert isinstance(args[-1]._obj, lib.counters_type)
        tally = returned[COUNTERS]
        assert tally == {**{key: 0 for key in tally}, **TALLY} and len(tally) == 8


def call(T, lib, obj, method, kind, replace, items_at, **kwargs):
    given, read = items_of(T, kind, replace)
    lib.peek = (items_at, read.nbytes)
    extra = {} if replace is None else {"tmax" if kind == "rays" else "max_dist2": replace}
    return getattr(obj, method)(given, **extra, **kwargs), read.tobytes()


BOOLS = (False, True)

# the queries with one record per item: (owner, method, kind, replaced field value, keyword arguments, C function, arguments
# between the handle and the outputs, outputs, returned layout)
PER_ITEM = []
for counters in BOOLS:
    tail, c = ("_counters", [COUNTERS]) if counters else ("", [])
    qp = ("QueryParams", {"max_bvh_iterations": 300, "max_leaf_tests": 9, "any_hit": 1})
    PER_ITEM += [
        ("scene", "trace_rays", "rays", 2.5, dict(any_hit=True, max_bvh_iterations=300, max_leaf_tests=9, counters=counters),
         "shray_trace_rays" + tail, [qp, ITEMS, 3], [("hit", ())], [0] + c if counters else 0),
        ("set", "trace_rays", "rays", None, dict(any_hit=True, max_bvh_iterations=300, max_leaf_tests=9, counters=counters),
         "shray_trace_instances" + tail, [qp, ITEMS, 3], [("hit", ()), ("i32", ())], [0, 1] + c),
        ("scene", "closest_points", "points", 4.0, dict(counters=counters), "shray_closest_points" + tail, [ITEMS, 3],
         [("closest", ())], [0] + c if counters else 0),
        ("set", "closest_points", "points", None, dict(counters=counters), "shray_closest_points_instances" + tail, [ITEMS, 3],
         [("closest", ()), ("i32", ())], [0, 1] + c),
    ]
    for closest in BOOLS:
        PER_ITEM.append(("set", "signed_distance", "points", 4.0, dict(closest=closest, counters=counters),
                         "shray_signed_distance_instances" + tail, [ITEMS, 3],
                         [("f32", ()), ("closest", ()) if closest else None, ("i32", ()) if closest else None],
                         ([0, 1, 2] if closest else [0]) + c if closest or counters else 0))
for closest in BOOLS:
    record = ("closest", ()) if closest else None
    PER_ITEM += [
        ("scene", "signed_distance", "points", 4.0, dict(closest=closest), "shray_signed_distance", [ITEMS, 3],
         [("f32", ()), record], [0, 1] if closest else 0),
        ("scene", "winding_signed_distance", "points", None, dict(beta=1.5, closest=closest), "shray_winding_signed_distance",
         [ITEMS, 3, 1.5], [("f32", ()), record], [0, 1] if closest else 0),
        ("set", "winding_signed_distance", "points", 4.0, dict(beta=1.5, closest=closest), "shray_winding_signed_distance_instances",
         [ITEMS, 3, 1.5], [("f32", ()), record, ("i32", ()) if closest else None], [0, 1, 2] if closest else 0),
        ("set", "winding_number", "points", None, dict(beta=1.5, containing=closest), "shray_winding_number_instances",
         [ITEMS, 3, 1.5], [("f32", ()), ("i32", ()) if closest else None], [0, 1] if closest else 0),
    ]
PER_ITEM.append(("scene", "winding_number", "points", None, dict(beta=1.5), "shray_winding_number", [ITEMS, 3, 1.5], [("f32", ())], 0))


@pytest.mark.parametrize("case", PER_ITEM, ids=lambda c: f"{c[0]}.{c[1]}-{'-'.join(f'{k}={v}' for k, v in c[4].items())}")
def test_a_query_with_one_record_per_item(world, case):
    T, lib, scene, group = world
    owner, method, kind, replace, kwargs, function, middle, outs, layout = case
    obj, handle = (scene, SCENE_HANDLE) if owner == "scene" else (group, SET_HANDLE)
    got, read = call(T, lib, obj, method, kind, replace, 1 + middle.index(ITEMS), **kwargs)
    check(T, lib, handle, got, function, middle, outs, layout, items_bytes=read)


# the counted first-K queries: (method, kind, name of K, further keyword arguments, C function of the scene, of the set, params
# type, its fields besides K, record dtype, trailing shape of a record in the arrays)
FIRST_K = [
    ("trace_all_hits", "rays", "max_hits", dict(max_leaf_tests=9), "shray_trace_all_hits", "shray_trace_instances_all_hits",
     "MultihitParams", {"max_leaf_tests": 9}, "hit"),
    ("triangles_within", "points", "max_near", {}, "shray_near_triangles", "shray_near_triangles_instances", "NearParams", {}, "closest"),
    ("triangles_in_boxes", "boxes", "max_triangles", {}, "shray_overlap_triangles", "shray_overlap_triangles_instances",
     "OverlapParams", {"flags": 0}, "i32"),
    ("intersecting_triangles", "triangles", "max_triangles", dict(skip_shared=True), "shray_intersect_triangles",
     "shray_intersect_triangles_instances", "IntersectParams", {"flags": 2}, "i32"),
    ("triangle_distances", "triangles", "max_pairs", dict(max_dist2=0.25, skip_shared=True), "shray_clearance_triangles",
     "shray_clearance_triangles_instances", "ClearanceParams", {"flags": 2, "max_dist2": 0.25}, "pair"),
]


@pytest.mark.parametrize("counters", BOOLS, ids=lambda b: f"counters={b}")
@pytest.mark.parametrize("counts", BOOLS, ids=lambda b: f"counts={b}")
@pytest.mark.parametrize("k", (0, 2))
@pytest.mark.parametrize("owner", ("scene", "set"))
@pytest.mark.parametrize("case", FIRST_K, ids=lambda c: c[0])
def test_a_counted_first_k_query(world, case, owner, k, counts, counters):
    T, lib, scene, group = world
    method, kind, k_name, kwargs, of_scene, of_set, params_type, fields, record = case
    obj, handle, function = (scene, SCENE_HANDLE, of_scene) if owner == "scene" else (group, SET_HANDLE, of_set)
    kwargs = {**kwargs, k_name: k, "counts": counts, "counters": counters}
    if k == 0 and not counts:
        with pytest.raises(ValueError, match=f"nothing is asked for: {k_name} is 0 and counts is False"):
            call(T, lib, obj, method, kind, None, 2, **kwargs)
        assert lib.calls == []
        return
    got, read = call(T, lib, obj, method, kind, None, 2, **kwargs)
    outs = [(record, (k,)) if k else None] + ([("i32", (k,)) if k else None] if owner == "set" else []) + [("i32", ()) if counts else None]
    layout = list(range(len(outs))) + ([COUNTERS] if counters else [])
    check(T, lib, handle, got, function + ("_counters" if counters else ""), [(params_type, {**fields, k_name: k}), ITEMS, 3], outs,
          layout, items_bytes=read)


# an owner's own triangles as the queries: (owner, method, name of K, further keyword arguments, C function, params type, its
# fields besides K, record dtype)
RANGES = [
    ("scene", "self_intersections", "max_triangles", {}, "shray_intersect_self", "IntersectParams", {"flags": 2}, "i32"),
    ("scene", "self_clearance", "max_pairs", dict(max_dist2=0.25), "shray_clearance_self", "ClearanceParams",
     {"flags": 2, "max_dist2": 0.25}, "pair"),
    ("set", "instance_intersections", "max_triangles", {}, "shray_intersect_instance", "IntersectParams", {"flags": 4}, "i32"),
    ("set", "instance_clearance", "max_pairs", dict(max_dist2=0.25), "shray_clearance_instance", "ClearanceParams",
     {"flags": 4, "max_dist2": 0.25}, "pair"),
]


@pytest.mark.parametrize("counts", BOOLS, ids=lambda b: f"counts={b}")
@pytest.mark.parametrize("k", (0, 2))
@pytest.mark.parametrize("first,count,rows", [(0, None, TRIANGLES), (1, 2, 2), (TRIANGLES, 0, 0)], ids=("full", "inner", "empty-at-the-end"))
@pytest.mark.parametrize("case", RANGES, ids=lambda c: c[1])
def test_a_range_form(world, case, first, count, rows, k, counts):
    T, lib, scene, group = world
    owner, method, k_name, kwargs, function, params_type, fields, record = case
    kwargs = {**kwargs, k_name: k, "counts": counts, "first": first, "count": count}
    if k == 0 and not counts:
        with pytest.raises(ValueError, match=f"nothing is asked for: {k_name} is 0 and counts is False"):
            getattr(scene, method)(**kwargs) if owner == "scene" else getattr(group, method)(1, **kwargs)
        assert lib.calls == []
        return
    params = (params_type, {**fields, k_name: k})
    if owner == "scene":
        got = getattr(scene, method)(**kwargs)
        handle, middle = SCENE_HANDLE, [params, first, rows]
        outs = [(record, (k,)) if k else None, ("i32", ()) if counts else None]
    else:
        got = getattr(group, method)(1, **kwargs)
        handle, middle = SET_HANDLE, [params, 1, first, rows]
        outs = [(record, (k,)) if k else None, ("i32", (k,)) if k else None, ("i32", ()) if counts else None]
    check(T, lib, handle, got, function, middle, outs, list(range(len(outs))), rows=rows)
