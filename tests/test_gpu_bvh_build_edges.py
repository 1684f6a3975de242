"""The device BVH build (csrc/bvh_build.hip) where a level-parallel rebuild of the sequential make_bvh could part from it: the
inputs of tests/bvh_build_cases.py -- exact ties of the axis choice, the sweep and the partition predicate; node ranges on and
one off the multiples of a wave and a workgroup, next to whole waves and workgroups of retired positions; the partition's
extreme exchange patterns; the ends of the float range (denormals, an overflowing root area, an overflowing hi - lo, NaN bins);
a depth-18 chain; large leaves inside a tree; zeros of both signs; the build parameters' edges.  The yardstick is the host
builder, which tests/test_bvh_build_cases_reference.py pins to the compiled reference on the same inputs.  Every comparison is
a bit-for-bit equality."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import bvh_build_cases as B
from test_gpu_bvh_build import assert_same_world
from test_gpu_scene_device import assert_same_derived_arrays

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Inputs of the pipeline subset that host-path scene creation (shray_scene_create) refuses, with the error code the device path
# (shray_scene_create_from_device) must then refuse them with: none.
REFUSED_BY_SCENE_CREATION = {}


@pytest.fixture(scope="module")
def cases(pkg, tmp_path_factory):
    return B.CaseSet(pkg, tmp_path_factory.mktemp("bvh_build_cases"))


def build_and_download(pkg, path):
    """shray_bvh_build_device on the file's triangles as loaded: (the loaded triangle_vertices [T, 3], the built tree's
    triangle_vertices [T, 3], triangle_order [T])"""
    N = pkg._native
    hip, lib = N.load_hip(), N.load_host()
    handle = C.c_void_p()
    assert lib.shray_host_load_triangles(path.encode(), C.byref(handle)) == 0
    tv, vd, nt, nv = C.POINTER(C.c_int32)(), C.POINTER(C.c_float)(), C.c_int32(), C.c_int32()
    assert lib.shray_host_triangles(handle, C.byref(tv), C.byref(nt), C.byref(vd), C.byref(nv)) == 0
    loaded = np.ctypeslib.as_array(tv, shape=(nt.value, 3)).copy()
    built = C.c_void_p()
    N.check(hip.shray_bvh_build_device(tv, nt, vd, nv, 9, None, C.byref(built)))
    tree, order = N.TreeDesc(), C.POINTER(C.c_int32)()
    N.check(hip.shray_device_tree_download(built, C.byref(tree), C.byref(order)))
    assert tree.triangle_count == nt.value
    vertices = np.ctypeslib.as_array(tree.triangle_vertices, shape=(nt.value, 3)).copy()
    order = np.ctypeslib.as_array(order, shape=(nt.value,)).copy()
    hip.shray_device_tree_destroy(built)
    lib.shray_host_free_world(handle)
    return loaded, vertices, order


@pytest.mark.parametrize("name", B.NAMES)
def test_device_build_equals_the_host_build(pkg, gpu, cases, name):
    """The pre-order tree arrays, the five statistics and every flattened array; and the build's triangle_order is a permutation
    that takes the input to the tree's triangle_vertices: every triangle is in the tree exactly once."""
    path = cases.path(name)
    host, device = pkg.World(path), pkg.World(path, build="gpu")
    try:
        assert_same_world(host, device, name)
    finally:
        host.close()
        device.close()
    loaded, vertices, order = build_and_download(pkg, path)
    assert np.array_equal(np.sort(order), np.arange(len(order))), f"{name}: triangle_order is not a permutation"
    assert np.array_equal(vertices, loaded[order]), f"{name}: triangle_vertices is not the input reordered by triangle_order"


def flat_arrays_differing(want, got):
    return [key for key, value in want.items()
            if (not np.array_equal(value.view(np.uint32), got[key].view(np.uint32)) if isinstance(value, np.ndarray) else value != got[key])]


@pytest.mark.parametrize("name", B.PIPELINE_NAMES)
def test_device_pipeline_equals_the_host_path(pkg, gpu, cases, name):
    """shray_bvh_build_device -> shray_flatten_device_tree -> shray_scene_create_from_device against World + Scene: the flattened
    arrays and everything scene creation derives; for three cases a frame with its work counters, on both kernels."""
    N = pkg._native
    path, env = cases.path(name), pkg.scenes.environment_constant()
    host_world, host_scene, device = pkg.World(path), None, None
    try:
        try:
            host_scene, host_code = pkg.Scene(host_world.flatten(), env), 0
        except N.ShrayError as refused:
            host_code = refused.code
        assert host_code == REFUSED_BY_SCENE_CREATION.get(name, 0), (name, host_code)
        if host_code != 0:
            with pytest.raises(N.ShrayError) as caught:
                device = pkg.tracer.DeviceWorld(path, env)
            assert caught.value.code == host_code, (name, caught.value.code, host_code)
            return
        device = pkg.tracer.DeviceWorld(path, env)
        assert not flat_arrays_differing(host_world.arrays(), device.flat_arrays()), name
        assert_same_derived_arrays(host_scene, device.scene, name)
        assert (device.stats.node_count, device.stats.leaf_count, device.stats.max_level, device.stats.large_leaves) == \
            (host_world.info.node_count, host_world.info.leaf_count, host_world.info.max_level, host_world.info.large_leaves), name
        if name in B.FRAME_NAMES:
            params = host_world.frame_params(96, 64, material=0)
            assert bytes(params) == bytes(device.frame_params(96, 64, material=0))
            for kernel in (0, 1):
                host_scene.set_kernel(kernel)
                device.scene.set_kernel(kernel)
                want, want_counters = host_scene.render_counters(params, 96, 64, 1)
                got, got_counters = device.scene.render_counters(params, 96, 64, 1)
                assert np.array_equal(want.view(np.uint32), got.view(np.uint32)) and want_counters == got_counters, (name, kernel)
    finally:        # a failing comparison must not leave a scene's device buffers to the garbage collector while the other cases run
        for obj in (host_scene, device, host_world):
            if obj is not None:
                obj.close()


CHILD = r'''
import sys
sys.path[:0] = [%r, %r]
from __graft_entry__ import load_package
import bvh_build_cases as B
from test_gpu_bvh_build import assert_same_world
pkg = load_package()
N = pkg._native
cases = B.CaseSet(pkg, %r)
max_depth, leaf_max, ctrav, cisec = B.option_values(%r)
read = pkg.host.bvh_options_from_environment()          # what the host builder of this process goes by
assert (read.max_depth, read.leaf_max, read.sah_ctrav, read.sah_cisec) == (max_depth, leaf_max, ctrav, cisec), "the environment did not arrive"
for name in B.OPTION_INPUTS:
    options = N.BvhOptions(0, max_depth, leaf_max, ctrav, cisec)       # (leaf_max -1 goes in as -1: every node a leaf)
    host = pkg.World(cases.path(name))
    device = pkg.World(cases.path(name), build="gpu", options=options)
    assert host.info.max_level <= max_depth
    assert_same_world(host, device, name)
    print("same", name, host.info.node_count, host.info.max_level, host.info.large_leaves)
    host.close()
    device.close()
print("ok")
'''

_child_trouble = []     # a child that did not exit with 0 and a final `ok`: no further child is started


@pytest.mark.parametrize("options", list(B.OPTION_SETS))
def test_device_build_under_each_option_set(gpu, cases, options):
    """BVH_MAX_DEPTH 0, 1, 4; BVH_LEAF_MAX 0, 1, -1; SAH_CISEC 0; SAH_CTRAV 1e6 -- the host builder reads them once per process,
    so each set runs in a child of its own, under its own time limit, on the chain, a shuffled lattice, the 513-row and the
    soup; the device build takes the same values as shray_bvh_options.  Also compared: large_leaves, which the device recounts
    from the tree (a leaf above leaf_max at the depth limit is not one)."""
    assert not _child_trouble, f"not started: the child of {_child_trouble[0]} did not end cleanly"
    for name in B.OPTION_INPUTS:
        cases.path(name)
    env = {k: v for k, v in os.environ.items() if k not in ("BVH_MAX_DEPTH", "BVH_LEAF_MAX", "SAH_CTRAV", "SAH_CISEC")}
    env.update(B.option_environment(options))
    script = CHILD % (ROOT, os.path.join(ROOT, "tests"), cases.directory, options)
    run = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", script], env=env, capture_output=True, text=True)
    if run.returncode != 0 or not run.stdout.strip().endswith("ok"):      # a failed comparison and a HIP error both end with 1
        _child_trouble.append(options)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok"), (run.returncode, run.stdout[-1000:], run.stderr[-3000:])
