"""Signed distance queries on the GPU (include/shader_ray_sdf.h) against the restatement (tests/sdf_ref.py): every
closest-point record byte-equal to shray_closest_points, every signed value and the sign data bit-equal to the restatement,
the topology report equal to it, and on the closed scenes the sign equal to the float64 winding number beyond a margin.
Host and device paths, DeviceWorld, the first derivation on a side stream followed by unsynchronised use elsewhere, the
re-derivation after a device or a host refit, a count split over launches (with and without records), misses and non-finite
points (through the point kinds of test_gpu_point_query), and the refusals of scenes without a packed tree (a chain that is not
a canonical tree, and a canonical comb deeper than scene creation packs)."""
import ctypes as C
import os

import numpy as np
import pytest

import point_query_ref as R
import sdf_ref as S
from test_gpu_point_query import BAD_TREE, assert_bits, loaded, make_points, scene_path
from test_oracle_kat import chain_scene

pytestmark = pytest.mark.gpu

F = np.float32
_small = {}


def small_scene(pkg, tmp_path_factory, name):
    """the cube and the fan spike as trisrc files, loaded like the others"""
    if name not in _small:
        path = str(tmp_path_factory.mktemp("sdf") / f"{name}.trisrc")
        pkg.scenes.write_trisrc(path, *getattr(S, name)())
        world = pkg.World(path)
        _small[name] = (world, world.arrays(), pkg.Scene(world.flatten()))
    return _small[name][1], _small[name][2]


def scene_of(pkg, tmp_path_factory, name):
    return small_scene(pkg, tmp_path_factory, name) if name in ("cube", "fan_spike") else loaded(pkg, name)


def assert_same_floats(got, want, what):
    g, w = np.asarray(got, F).reshape(-1), np.asarray(want, F).reshape(-1)
    same = (g.view(np.uint32) == w.view(np.uint32)) | (np.isnan(g) & np.isnan(w))
    bad = np.nonzero(~same)[0]
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(g)} values differ, first {bad[:5]}: got {g[bad[:3]]} want {w[bad[:3]]}"


def device_signed(scene, points, closest=True):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(points).view(F).reshape(-1, 4).copy()).cuda()
    out, rec = scene.signed_distance(t, closest=True)
    torch.cuda.current_stream().synchronize()
    return out.cpu().numpy(), np.ascontiguousarray(rec.cpu().numpy()).view(R.CLOSEST_DTYPE).reshape(-1)


SCENES = [("small_trisrc", 20000, True), ("lobed_528", 20000, True), ("bunny", 20000, True), ("quads_mixed", 3000, False),
          ("cube", 4000, True), ("fan_spike", 4000, True)]


@pytest.mark.parametrize("name, n, closed", SCENES)
def test_records_values_sign_data_and_topology(pkg, gpu, tmp_path_factory, name, n, closed):
    arrays, scene = scene_of(pkg, tmp_path_factory, name)
    positions = np.asarray(arrays["vertex_positions"], F)
    want = S.derive(positions)
    assert want["info"]["closed"] == int(closed)
    assert scene.surface_info() == want["info"]
    assert_same_floats(scene.sign_data(), want["sign_data"], f"{name}, sign data")

    pts = make_points(arrays, n, seed=n + 3 * len(name))
    records = scene.closest_points(pts)
    got, rec = scene.signed_distance(pts, closest=True)
    assert_bits(rec, records, f"{name}, host path records")
    expect = S.signed(pts, records, want["sign_data"])
    assert np.isnan(expect).sum() > 0 and (expect < 0).sum() > 0
    assert_same_floats(got, expect, f"{name}, host path")
    assert_same_floats(scene.signed_distance(pts), expect, f"{name}, host path without records")
    dgot, drec = device_signed(scene, pts)
    assert_bits(drec, records, f"{name}, device path records")
    assert_same_floats(dgot, expect, f"{name}, device path")


@pytest.mark.parametrize("name", ["small_trisrc", "lobed_528", "bunny", "cube", "fan_spike"])
def test_sign_matches_the_winding_number_on_closed_scenes(pkg, gpu, tmp_path_factory, name):
    arrays, scene = scene_of(pkg, tmp_path_factory, name)
    positions = np.asarray(arrays["vertex_positions"], F)
    tris = positions.reshape(-1, 3)
    lo, hi = tris.min(0), tris.max(0)
    extent = float(np.linalg.norm(hi - lo))
    rng = np.random.default_rng(11)
    n = 400 if name == "bunny" else 3000
    p = ((lo + hi) / 2 + (rng.random((n, 3)) * 2 - 1) * 0.65 * (hi - lo)).astype(F)
    s = scene.signed_distance(pkg.tracer.make_points(p))
    keep = np.abs(s) > 1e-3 * extent
    inside = S.winding_number(positions, p[keep]) > 0.5
    assert inside.any() and (~inside).any()
    assert np.array_equal(s[keep] < 0, inside)


def test_device_world_matches_host_scene(pkg, gpu):
    arrays, scene = loaded(pkg, "lobed_528")
    dw = pkg.tracer.DeviceWorld(scene_path("lobed_528"))
    try:
        pts = make_points(arrays, 6000, seed=21)
        want = scene.signed_distance(pts)
        assert_same_floats(dw.signed_distance(pts), want, "DeviceWorld, host path")
        assert_same_floats(device_signed(dw, pts)[0], want, "DeviceWorld, device path")
        assert dw.surface_info() == scene.surface_info()
        assert_same_floats(dw.sign_data(), scene.sign_data(), "DeviceWorld, sign data")
    finally:
        dw.close()


def moved_lobed(pos):
    """the lobed sphere scaled and pushed: a point near the old surface changes side"""
    scale = np.array([1.35, 0.8, 1.1], F)
    return (pos * scale + np.sin(pos[:, 1:2] * F(3)) * F(0.15) + F(0.2)).astype(F)


def test_first_derivation_on_a_side_stream_orders_later_use(pkg, gpu):
    """The first signed query of a fresh scene runs on a non-blocking side stream, so the derivation is enqueued there; with
    no synchronisation, surface_info and sign_data (blocking) and a query on the default stream must see it finished."""
    import torch
    world = pkg.World(scene_path("quads_mixed"))
    scene = pkg.Scene(world.flatten())
    try:
        arrays = world.arrays()
        want = S.derive(np.asarray(arrays["vertex_positions"], F))
        assert want["info"]["closed"] == 0
        pts = make_points(arrays, 4000, seed=44)
        d_pts = torch.from_numpy(np.ascontiguousarray(pts).view(F).reshape(-1, 4).copy()).cuda()
        d_side = torch.empty(len(pts), dtype=torch.float32, device="cuda")
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            scene.signed_distance_into(d_pts.data_ptr(), len(pts), d_side.data_ptr(), 0, side.cuda_stream)
        assert scene.surface_info() == want["info"]
        assert_same_floats(scene.sign_data(), want["sign_data"], "sign data after a side-stream derivation")
        d_main = scene.signed_distance(d_pts)
        expect = S.signed(pts, scene.closest_points(pts), want["sign_data"])
        assert_same_floats(d_main.cpu().numpy(), expect, "default stream after a side-stream derivation")
        side.synchronize()
        assert_same_floats(d_side.cpu().numpy(), expect, "the side stream's own query")
    finally:
        scene.close()
        world.close()


def test_device_refit_then_signed_query_rederives(pkg, gpu):
    """A device refit on a side stream, then a signed query on the same stream: the refit bumps the scene's geometry
    generation and the query re-derives the sign data on its stream.  (shray_scene_refit_device returns once its work is
    done, so this checks the invalidation, not stream ordering; the side-stream test above checks that.)"""
    import torch
    world = pkg.World(scene_path("lobed_528"))
    scene = pkg.Scene(world.flatten())
    try:
        arrays = world.arrays()
        pos = np.asarray(arrays["vertex_positions"], F).reshape(-1, 3)
        pts = make_points(arrays, 6000, seed=9)
        before = scene.signed_distance(pts)
        moved = moved_lobed(pos)
        d_moved = torch.from_numpy(moved).cuda()
        d_pts = torch.from_numpy(np.ascontiguousarray(pts).view(F).reshape(-1, 4).copy()).cuda()
        d_out = torch.full((len(pts),), -7.0, dtype=torch.float32, device="cuda")
        d_rec = torch.full((len(pts), 8), -7, dtype=torch.int32, device="cuda")
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            scene.refit(d_moved, stream_ptr=side.cuda_stream)
            scene.signed_distance_into(d_pts.data_ptr(), len(pts), d_out.data_ptr(), d_rec.data_ptr(), side.cuda_stream)
        side.synchronize()
        got = d_out.cpu().numpy()
        rec = np.ascontiguousarray(d_rec.cpu().numpy()).view(R.CLOSEST_DTYPE).reshape(-1)
        assert_bits(rec, R.closest(moved.reshape(-1), pts), "records after the device refit")
        want = S.signed(pts, rec, S.derive(moved.reshape(-1))["sign_data"])
        assert_same_floats(got, want, "after the device refit")
        flipped = (np.sign(before) != np.sign(got)) & ~np.isnan(got) & ~np.isnan(before)
        assert flipped.sum() > 50
    finally:
        scene.close()
        world.close()


def test_host_refit_then_signed_query(pkg, gpu):
    world = pkg.World(scene_path("lobed_528"))
    scene = pkg.Scene(world.flatten())
    try:
        arrays = world.arrays()
        pos = np.asarray(arrays["vertex_positions"], F).reshape(-1, 3)
        pts = make_points(arrays, 6000, seed=10)
        before = scene.signed_distance(pts)
        assert scene.surface_info()["closed"] == 1
        moved = moved_lobed(pos)
        scene.refit(moved)
        got, rec = scene.signed_distance(pts, closest=True)
        want = S.derive(moved.reshape(-1))
        assert_same_floats(scene.sign_data(), want["sign_data"], "sign data after the host refit")
        assert_same_floats(got, S.signed(pts, R.closest(moved.reshape(-1), pts), want["sign_data"]), "after the host refit")
        assert ((np.sign(before) != np.sign(got)) & ~np.isnan(got) & ~np.isnan(before)).sum() > 50
    finally:
        scene.close()
        world.close()


@pytest.mark.parametrize("keep_records", [False, True])
def test_a_count_split_over_launches(pkg, gpu, keep_records):
    """2^24 + 3000 points, without records (through scratch, a chunk at a time) or with them (a launch's worth at a time): far
    points with radius 0 are misses (NaN); the last points and points scattered over the first launch are restated."""
    import torch
    arrays, scene = loaded(pkg, "small_trisrc")
    sd = S.derive(np.asarray(arrays["vertex_positions"], F))["sign_data"]
    n = (1 << 24) + 3000
    real = make_points(arrays, 3000 + 4096, seed=33)
    tail, spread = real[:3000], real[3000:]
    far = np.zeros(1, R.POINT_DTYPE)
    far["p"] = (1e6, -2e6, 3e6)
    far["max_dist2"] = 0.0

    def dev(p):
        return torch.from_numpy(np.ascontiguousarray(p).view(F).reshape(-1, 4).copy()).cuda()

    d_pts = dev(far).repeat(n, 1)
    d_pts[n - 3000:] = dev(tail)
    sample = torch.from_numpy(np.random.default_rng(1).choice(n - 3000, 4096, replace=False)).cuda()
    d_pts[sample] = dev(spread)
    d_out = torch.zeros(n, dtype=torch.float32, device="cuda")
    d_rec = torch.empty((n, 8), dtype=torch.int32, device="cuda") if keep_records else None
    scene.signed_distance_into(d_pts.data_ptr(), n, d_out.data_ptr(), d_rec.data_ptr() if keep_records else 0,
                               torch.cuda.current_stream().cuda_stream)
    torch.cuda.current_stream().synchronize()
    if keep_records:
        tail_records = np.ascontiguousarray(d_rec[n - 3000:].cpu().numpy()).view(R.CLOSEST_DTYPE).reshape(-1)
        assert_bits(tail_records, R.closest(arrays["vertex_positions"], tail), "the last points' records")
        del d_rec

    def want(p):
        return S.signed(p, R.closest(arrays["vertex_positions"], p), sd)

    assert_same_floats(d_out[n - 3000:].cpu().numpy(), want(tail), "the last points")
    assert_same_floats(d_out[sample].cpu().numpy(), want(spread), "points of the first launch")
    rest = torch.ones(n - 3000, dtype=torch.bool, device="cuda")
    rest[sample] = False
    assert bool(torch.isnan(d_out[: n - 3000][rest]).all())


def test_refusals_and_no_ops(pkg, gpu):
    """A scene without a packed tree (a hand-made chain) is refused with SHRAY_ERR_BAD_TREE; count 0 is a no-op; a GPU tensor
    of the wrong shape is refused by the binding; a misaligned device buffer is an argument error."""
    import torch
    hand = chain_scene(5)
    scene = pkg.Scene(hand.desc)
    try:
        with pytest.raises(pkg._native.ShrayError) as err:
            scene.signed_distance(np.zeros((4, 3), F))
        assert err.value.code == BAD_TREE
    finally:
        scene.close()
    arrays, good = loaded(pkg, "lobed_528")
    assert len(good.signed_distance(np.zeros((0, 3), F))) == 0
    with pytest.raises(ValueError):
        good.signed_distance(torch.zeros((4, 5), device="cuda"))
    lib = pkg._native.load_sdf()
    d = torch.zeros((2, 8), dtype=torch.int32, device="cuda")
    assert lib.shray_signed_distance_device(good._handle, C.c_void_p(d.data_ptr() + 4), 1, C.c_void_p(d.data_ptr()), None, None) == -1


def test_a_deep_canonical_tree_without_a_packed_tree_is_refused(pkg, gpu):
    """A comb of 150 branches (test_oracle_kat.comb_scene: each branch a leaf and the next branch) is a canonical threaded
    tree 150 levels deep.  Scene creation from host arrays keeps no packed tree for it, so the signed and the closest-point
    queries refuse it with SHRAY_ERR_BAD_TREE before anything is launched; surface_info, which does not walk, answers."""
    import test_oracle_kat as kat
    scene = pkg.Scene(kat.comb_scene(150).desc)
    try:
        for query in (scene.signed_distance, scene.closest_points):
            with pytest.raises(pkg._native.ShrayError) as err:
                query(np.zeros((4, 3), F))
            assert err.value.code == BAD_TREE, str(err.value)
        assert scene.surface_info() == {"vertices": 3, "edges": 3, "boundary_edges": 3, "nonmanifold_edges": 0, "misoriented_edges": 0,
                                        "degenerate_triangles": 0, "closed": 0}
    finally:
        scene.close()
