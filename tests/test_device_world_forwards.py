"""DeviceWorld's forwards to its Scene: exactly the listed methods are forwarded, as real attributes of the class with
Scene's documentation, and each passes its arguments on unchanged and returns what the scene's method returns.  No device:
the world is made without __init__ and its scene is a stub that records its calls."""
import inspect

import pytest

FORWARDS = ["trace_rays", "trace_rays_into", "trace_all_hits", "trace_all_hits_into", "crossing_counts", "closest_points",
            "closest_points_into", "triangles_within", "triangles_within_into", "near_counts", "triangles_in_boxes",
            "triangles_in_boxes_into", "box_counts", "boxes_touched", "surface_voxels", "signed_distance", "signed_distance_into",
            "surface_info", "sign_data", "winding_number", "winding_number_into", "winding_signed_distance",
            "winding_signed_distance_into", "winding_data", "primary_hits"]
NOT_FORWARDED = ["refit", "close", "host_world", "frame_params", "flat_arrays"]


class RecordingScene:
    """Answers any method: records (name, args, kwargs) and returns a token of its own per call."""

    def __init__(self):
        self.calls = []

    def close(self, *args, **kwargs):
        self.calls.append(("close", args, kwargs, None))

    def __getattr__(self, name):
        def method(*args, **kwargs):
            token = object()
            self.calls.append((name, args, kwargs, token))
            return token
        return method


@pytest.fixture
def world(pkg):
    w = pkg.tracer.DeviceWorld.__new__(pkg.tracer.DeviceWorld)
    w.scene = RecordingScene()
    yield w
    w.scene = None   # (nothing for __del__ to close)


def test_the_list_is_25_names():
    assert len(FORWARDS) == 25 and len(set(FORWARDS)) == 25


@pytest.mark.parametrize("name", FORWARDS)
def test_a_forward_is_a_callable_attribute_of_the_class(pkg, name):
    T = pkg.tracer
    assert name in vars(T.DeviceWorld) and name in dir(T.DeviceWorld)
    assert callable(getattr(T.DeviceWorld, name))


@pytest.mark.parametrize("name", FORWARDS)
def test_a_forward_has_the_scenes_docstring(pkg, name):
    T = pkg.tracer
    assert getattr(T.Scene, name).__doc__
    assert getattr(T.DeviceWorld, name).__doc__ == getattr(T.Scene, name).__doc__


@pytest.mark.parametrize("name", FORWARDS)
def test_the_scene_is_called_as_the_world_was(pkg, world, name):
    """Under Scene's own signature, defaults filled in, the scene's method gets the call the world's got: with every optional
    parameter given by keyword, and with none given (a forward has no defaults of its own that could differ from Scene's)."""
    signature = inspect.signature(getattr(pkg.tracer.Scene, name))
    parameters = list(signature.parameters.values())[1:]
    required = tuple(object() for p in parameters if p.default is p.empty)
    optional = {p.name: object() for p in parameters if p.default is not p.empty}
    for kwargs in (optional, {}):
        del world.scene.calls[:]
        got = getattr(world, name)(*required, **kwargs)
        (called, got_args, got_kwargs, token), = world.scene.calls
        assert called == name and got is token
        want, seen = signature.bind(None, *required, **kwargs), signature.bind(None, *got_args, **got_kwargs)
        want.apply_defaults(), seen.apply_defaults()
        assert want.arguments.keys() == seen.arguments.keys()
        for key, value in want.arguments.items():
            assert seen.arguments[key] is value or seen.arguments[key] == value, key


@pytest.mark.parametrize("name", FORWARDS)
def test_a_forward_passes_its_arguments_on_verbatim_and_returns_the_result(world, name):
    a, b = object(), object()
    for args, kwargs in (((), {}), ((a,), {}), ((a, 2, b), {}), ((a,), {"x": b, "y": 3}), ((), {"only": a})):
        stub = world.scene
        del stub.calls[:]
        got = getattr(world, name)(*args, **kwargs)
        assert len(stub.calls) == 1
        called, got_args, got_kwargs, token = stub.calls[0]
        assert called == name and got is token
        assert len(got_args) == len(args) and all(x is y for x, y in zip(got_args, args))
        assert got_kwargs.keys() == kwargs.keys() and all(got_kwargs[k] is kwargs[k] for k in kwargs)


def test_exactly_the_listed_methods_are_forwarded(pkg, world):
    """Every public attribute of the class is tried on the stub: the ones that reach it under their own name are the list."""
    stub = world.scene
    forwarded = set()
    for name in dir(type(world)):
        if name.startswith("_") or name in NOT_FORWARDED or not callable(getattr(type(world), name)):
            continue
        del stub.calls[:]
        of_scene = getattr(pkg.tracer.Scene, name, None)
        required = [p for p in list(inspect.signature(of_scene).parameters.values())[1:] if p.default is p.empty] if of_scene else []
        try:
            getattr(world, name)(*(object() for _ in required))
        except Exception:
            pass   # (a method of the world's own, missing the state __init__ gives it)
        if [c[0] for c in stub.calls] == [name]:
            forwarded.add(name)
    assert forwarded == set(FORWARDS)
    marker = object()
    for name in NOT_FORWARDED:
        assert name in vars(type(world))
        del stub.calls[:]
        try:
            getattr(world, name)(marker, key=marker)
        except Exception:
            pass
        assert not any(c[0] == name and c[1] == (marker,) and c[2] == {"key": marker} for c in stub.calls), name
