"""Winding-number queries on the GPU (include/shader_ray_winding.h) against the restatement (tests/winding_ref.py): the node
records and every winding number bit-equal to it for beta 2, 0.5 and the exact mode, every winding-signed value bit-equal to
it with records byte-equal to shray_closest_points, on the test scenes and the restatement's small meshes, with the point
kinds of test_gpu_point_query.  Host and device paths, DeviceWorld, a count split over launches, the re-derivation after a
device or a host refit, the first derivation on a side stream followed by unsynchronised use elsewhere, and the refusal of a
scene without a packed tree."""
import ctypes as C
import math

import numpy as np
import pytest

import point_query_ref as R
import refit_ref
import winding_ref as W
from test_gpu_point_query import BAD_TREE, _cache, assert_bits, loaded, make_points, scene_path
from test_gpu_signed_distance import assert_same_floats, moved_lobed
from test_oracle_kat import chain_scene

pytestmark = pytest.mark.gpu

F = np.float32
BETAS = (2.0, 0.5, math.inf)
_small = {}


def world_scene(pkg, tmp_path_factory, name):
    """(world, flattened arrays, resident scene) of a test scene or of one of the restatement's meshes"""
    if name in W.MESHES:
        if name not in _small:
            world = pkg.World(W.write_mesh(pkg, str(tmp_path_factory.mktemp("winding") / f"{name}.trisrc"), name))
            _small[name] = (world, world.arrays(), pkg.Scene(world.flatten()))
        return _small[name]
    arrays, scene = loaded(pkg, name)
    return _cache[name][0], arrays, scene


def dev(points):
    import torch
    return torch.from_numpy(np.ascontiguousarray(points).view(F).reshape(-1, 4).copy()).cuda()


SCENES = [("small_trisrc", 1500), ("lobed_528", 2000), ("bunny", 500), ("quads_mixed", 2000)] + [(m, 2000) for m in W.MESHES]


@pytest.mark.parametrize("name, n", SCENES)
def test_records_winding_numbers_and_signed_values(pkg, gpu, tmp_path_factory, name, n):
    import torch
    world, arrays, scene = world_scene(pkg, tmp_path_factory, name)
    ref = W.Restated(world)
    assert_same_floats(scene.winding_data(), ref.records, f"{name}, node records")
    pts = make_points(arrays, n, seed=n + 7 * len(name))
    d_pts = dev(pts)
    for beta in BETAS:
        want = ref.w(pts, beta)
        assert np.isnan(want).sum() > 0
        assert_same_floats(scene.winding_number(pts, beta=beta), want, f"{name}, beta {beta}, host path")
        got = scene.winding_number(d_pts, beta=beta)
        torch.cuda.current_stream().synchronize()
        assert_same_floats(got.cpu().numpy(), want, f"{name}, beta {beta}, device path")
    records = scene.closest_points(pts)
    want = W.winding_signed(records, ref.w(pts, 2.0))
    assert ((want < 0).sum() > 0) == (name != "inward_cube") and np.isnan(want).sum() > 0   # (w is -1 inside the inward cube)
    got, rec = scene.winding_signed_distance(pts, closest=True)
    assert_bits(rec, records, f"{name}, host path records")
    assert_same_floats(got, want, f"{name}, winding-signed, host path")
    assert_same_floats(scene.winding_signed_distance(pts), want, f"{name}, winding-signed without records")
    dgot, drec = scene.winding_signed_distance(d_pts, closest=True)
    torch.cuda.current_stream().synchronize()
    assert_bits(np.ascontiguousarray(drec.cpu().numpy()).view(R.CLOSEST_DTYPE).reshape(-1), records, f"{name}, device path records")
    assert_same_floats(dgot.cpu().numpy(), want, f"{name}, winding-signed, device path")


def test_device_world_matches_host_scene(pkg, gpu):
    import torch
    arrays, scene = loaded(pkg, "lobed_528")
    dw = pkg.tracer.DeviceWorld(scene_path("lobed_528"))
    try:
        pts = make_points(arrays, 3000, seed=21)
        assert_same_floats(dw.winding_data(), scene.winding_data(), "DeviceWorld, node records")
        want = scene.winding_number(pts)
        assert_same_floats(dw.winding_number(pts), want, "DeviceWorld, host path")
        d_pts = dev(pts)
        d_out = torch.empty(len(pts), dtype=torch.float32, device="cuda")
        dw.winding_number_into(d_pts.data_ptr(), len(pts), d_out.data_ptr(), 2.0, torch.cuda.current_stream().cuda_stream)
        torch.cuda.current_stream().synchronize()
        assert_same_floats(d_out.cpu().numpy(), want, "DeviceWorld, device path")
        assert_same_floats(dw.winding_signed_distance(pts), scene.winding_signed_distance(pts), "DeviceWorld, winding-signed")
    finally:
        dw.close()


def moved(world):
    """the lobed sphere's corners moved (test_gpu_signed_distance.moved_lobed) and the restatement of the refit scene"""
    arrays = world.arrays()
    pos = moved_lobed(np.asarray(arrays["vertex_positions"], F).reshape(-1, 3))
    tree = refit_ref.TreeArrays.of(world.export_tree())
    return pos, W.Restated(world, positions=pos, boxes=refit_ref.node_boxes(tree, pos))


def test_device_refit_then_query_rederives(pkg, gpu):
    """A device refit on a side stream, then winding queries on the same stream: the refit bumps the scene's geometry
    generation and the first query re-derives the records on its stream."""
    import torch
    world = pkg.World(scene_path("lobed_528"))
    scene = pkg.Scene(world.flatten())
    try:
        arrays = world.arrays()
        pts = make_points(arrays, 4000, seed=9)
        before = scene.winding_number(pts)
        pos, ref = moved(world)
        d_pts = dev(pts)
        d_w = torch.full((len(pts),), -7.0, dtype=torch.float32, device="cuda")
        d_s = torch.full((len(pts),), -7.0, dtype=torch.float32, device="cuda")
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            scene.refit(torch.from_numpy(pos).cuda(), stream_ptr=side.cuda_stream)
            scene.winding_number_into(d_pts.data_ptr(), len(pts), d_w.data_ptr(), 2.0, side.cuda_stream)
            scene.winding_signed_distance_into(d_pts.data_ptr(), len(pts), d_s.data_ptr(), 0, 2.0, side.cuda_stream)
        side.synchronize()
        want = ref.w(pts, 2.0)
        assert_same_floats(d_w.cpu().numpy(), want, "winding numbers after the device refit")
        assert_same_floats(scene.winding_data(), ref.records, "node records after the device refit")
        signed = W.winding_signed(R.closest(pos.reshape(-1), pts), want)
        assert_same_floats(d_s.cpu().numpy(), signed, "winding-signed after the device refit")
        assert ((before > 0.5) != (want > 0.5)).sum() > 50
    finally:
        scene.close()
        world.close()


def test_host_refit_then_query(pkg, gpu):
    world = pkg.World(scene_path("lobed_528"))
    scene = pkg.Scene(world.flatten())
    try:
        pts = make_points(world.arrays(), 4000, seed=10)
        before = scene.winding_number(pts, beta=math.inf)
        pos, ref = moved(world)
        scene.refit(pos)
        got = scene.winding_number(pts, beta=math.inf)
        assert_same_floats(scene.winding_data(), ref.records, "node records after the host refit")
        assert_same_floats(got, ref.w(pts, math.inf), "exact winding numbers after the host refit")
        assert ((before > 0.5) != (got > 0.5)).sum() > 50
    finally:
        scene.close()
        world.close()


def test_first_derivation_on_a_side_stream_orders_later_use(pkg, gpu):
    """The first query of a fresh scene runs on a non-blocking side stream, so the derivation is enqueued there; with no
    synchronisation, the download (blocking) and a query on the default stream must see it finished."""
    import torch
    world = pkg.World(scene_path("quads_mixed"))
    scene = pkg.Scene(world.flatten())
    try:
        ref = W.Restated(world)
        pts = make_points(world.arrays(), 4000, seed=44)
        want = ref.w(pts, 2.0)
        d_pts = dev(pts)
        d_side = torch.empty(len(pts), dtype=torch.float32, device="cuda")
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            scene.winding_number_into(d_pts.data_ptr(), len(pts), d_side.data_ptr(), 2.0, side.cuda_stream)
        assert_same_floats(scene.winding_data(), ref.records, "node records after a side-stream derivation")
        d_main = scene.winding_number(d_pts)
        assert_same_floats(d_main.cpu().numpy(), want, "default stream after a side-stream derivation")
        side.synchronize()
        assert_same_floats(d_side.cpu().numpy(), want, "the side stream's own query")
    finally:
        scene.close()
        world.close()


@pytest.mark.parametrize("signed", [False, True])
def test_a_count_split_over_launches(pkg, gpu, signed):
    """2^24 + 3000 points: far points (radius 0: misses for the winding-signed distance, which then goes through scratch a
    chunk at a time), the last points and points scattered over the first launch restated."""
    import torch
    world, arrays, scene = world_scene(pkg, None, "small_trisrc")
    ref = W.Restated(world)
    n = (1 << 24) + 3000
    real = make_points(arrays, 3000 + 4096, seed=33)
    tail, spread = real[:3000], real[3000:]
    far = np.zeros(1, R.POINT_DTYPE)
    far["p"] = (1e6, -2e6, 3e6)
    far["max_dist2"] = 0.0
    d_pts = dev(far).repeat(n, 1)
    d_pts[n - 3000:] = dev(tail)
    sample = torch.from_numpy(np.random.default_rng(1).choice(n - 3000, 4096, replace=False)).cuda()
    d_pts[sample] = dev(spread)
    d_out = torch.zeros(n, dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    if signed:
        scene.winding_signed_distance_into(d_pts.data_ptr(), n, d_out.data_ptr(), 0, 2.0, stream)

        def want(p):
            return W.winding_signed(R.closest(arrays["vertex_positions"], p), ref.w(p))
    else:
        scene.winding_number_into(d_pts.data_ptr(), n, d_out.data_ptr(), 2.0, stream)

        def want(p):
            return ref.w(p)
    torch.cuda.current_stream().synchronize()
    assert_same_floats(d_out[n - 3000:].cpu().numpy(), want(tail), "the last points")
    assert_same_floats(d_out[sample].cpu().numpy(), want(spread), "points of the first launch")
    rest = torch.ones(n - 3000, dtype=torch.bool, device="cuda")
    rest[sample] = False
    values = d_out[: n - 3000][rest]
    if signed:
        assert bool(torch.isnan(values).all())
    else:
        far_w = want(far)[0]
        assert bool((values == float(far_w)).all()), far_w


def test_refusals_and_no_ops(pkg, gpu):
    """A scene without a packed tree (a hand-made chain) is refused with SHRAY_ERR_BAD_TREE by every call; count 0 is a
    no-op; a NaN or negative beta and a misaligned device buffer are argument errors."""
    import torch
    hand = chain_scene(5)
    scene = pkg.Scene(hand.desc)
    try:
        for call in (lambda: scene.winding_number(np.zeros((4, 3), F)), lambda: scene.winding_signed_distance(np.zeros((4, 3), F)),
                     scene.winding_data):
            with pytest.raises(pkg._native.ShrayError) as err:
                call()
            assert err.value.code == BAD_TREE
    finally:
        scene.close()
    arrays, good = loaded(pkg, "lobed_528")
    assert len(good.winding_number(np.zeros((0, 3), F))) == 0
    for beta in (float("nan"), -1.0):
        with pytest.raises(pkg._native.ShrayError):
            good.winding_number(np.zeros((4, 3), F), beta=beta)
    lib = pkg._native.load_winding()
    d = torch.zeros((2, 8), dtype=torch.int32, device="cuda")
    assert lib.shray_winding_number_device(good._handle, C.c_void_p(d.data_ptr() + 4), 1, 2.0, C.c_void_p(d.data_ptr()), None) == -1
