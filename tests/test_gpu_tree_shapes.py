"""The refit, the winding-number derivation and every walk on the GPU over the hand-shaped trees of tests/tree_shapes.py, which
sit on the edges of the bottom-up schedule (csrc/tree_order.h): a root that is a leaf, a tail that is the root alone, a height
of exactly 1024 branches (all in the one-workgroup tail) and of 1025 (a wide launch whose last workgroup has one live
thread), two wide launches before a tail that starts full, and branches whose children were written one by a wide launch and
one by the tail.  Everything is compared bit for bit with the restatements the other GPU modules use (refit_ref, winding_ref,
point_query_ref, sdf_ref, near_ref, multi_hit_ref, ray_query_ref, scene_ref.half_bits); the only tolerance is the SAH cost's
rel=1e-12 of test_gpu_refit.  Every message names the shape.

A scene is made from a shape as test_gpu_refit.expected_scene makes one: refit_ref.tree_desc -> shray_flatten_device ->
shray_scene_create.  shray_scene_create_from_device takes only a tree shray_bvh_build_device made, so it sees the one shape the
builder reproduces: leaf_root's three triangles, which it leaves in one leaf (checked on the downloaded tree)."""
import ctypes as C
import math

import numpy as np
import pytest

import multi_hit_ref as M
import near_cases
import near_ref as NR
import point_query_ref as PQ
import ray_query_ref as RQ
import refit_ref as R
import scene_ref
import sdf_ref as S
import tree_shapes as T
import winding_ref as W
from test_gpu_multi_hit import assert_same_records
from test_gpu_point_query import assert_bits, make_points
from test_gpu_ray_query import assert_same_hits, random_rays
from test_gpu_refit import Positions, assert_same_scene, deform, expected_scene, snapshot, assert_unchanged
from test_gpu_signed_distance import assert_same_floats

pytestmark = pytest.mark.gpu

F = np.float32
INVALID = -1
BETAS = (2.0, 0.5, math.inf)
N_RAYS = 4096
WALK_SHAPES = ("leaf_root", "one_branch", "wide_by_one")


class Shape:
    """A resident scene of a hand-shaped tree, the tree, its vertex data [V, 9] and its flattened arrays as loaded."""

    def __init__(self, pkg, name):
        self.name = name
        self.env = pkg.scenes.environment_constant()
        self.tree, self.vertex_data = T.build(name)
        flat = pkg.tracer.DeviceFlat(R.tree_desc(self.tree, self.tree.box, self.vertex_data))
        self.arrays = flat.arrays()
        self.scene = pkg.Scene(flat.download(), self.env)
        flat.close()

    def corners(self, vd=None):
        vd = self.vertex_data if vd is None else vd
        return np.ascontiguousarray(vd[self.tree.triangle_vertices][:, :, :3])

    def refit(self, vd, how="host", stream=None):
        """the host path, or the device path on the non-null `stream`"""
        tv = self.tree.triangle_vertices
        if how == "host":
            return self.scene.refit(vd, tv, normal_offset=6)
        import torch
        with torch.cuda.stream(stream):
            d_vd, d_tv = torch.from_numpy(np.ascontiguousarray(vd)).cuda(), torch.from_numpy(tv.copy()).cuda()
            return self.scene.refit(d_vd, d_tv, normal_offset=6, stream_ptr=stream.cuda_stream)

    def restated(self, vd=None):
        """(winding_ref.Restated, node boxes) of the tree over `vd`"""
        corners = self.corners(vd)
        boxes = self.tree.box if vd is None else R.node_boxes(self.tree, corners)
        return W.Restated.of_tree(self.tree, corners, boxes), boxes

    def arrays_of(self, vd):
        """what the point generators read of the flattened arrays, for the tree over `vd`"""
        corners = self.corners(vd)
        bmin, bmax = R.flat_boxes(self.tree, R.node_boxes(self.tree, corners))
        return {"vertex_positions": corners.reshape(-1), "group_boxmin": bmin, "group_boxmax": bmax}

    def close(self):
        self.scene.close()


@pytest.fixture(scope="module")
def shapes(pkg, gpu):
    """shapes(name): one Shape per name for this module, refit to its loaded vertices whenever it is handed out and when the
    module ends its use of it (every test restores it as well), closed at the module's end"""
    made = {}

    def get(name):
        if name not in made:
            made[name] = Shape(pkg, name)
        s = made[name]
        s.refit(s.vertex_data)
        return s

    yield get
    for s in made.values():
        s.close()


def dev(records, width):
    import torch
    return torch.from_numpy(np.ascontiguousarray(records).view(F).reshape(-1, width).copy()).cuda()


def same_ray_results(pkg, got, want, corners, seed, what):
    """4096 seeded rays about `corners`, closest and any hit, kernels 0 and 1: equal hits and counters on both scenes"""
    o, d, tmax = random_rays(Positions(corners), N_RAYS, seed=seed)
    rays = pkg.tracer.make_rays(o, d, tmax)
    for kernel in (0, 1):
        got.set_kernel(kernel)
        want.set_kernel(kernel)
        for any_hit in (False, True):
            a, ac = got.trace_rays(rays, any_hit=any_hit, counters=True)
            b, bc = want.trace_rays(rays, any_hit=any_hit, counters=True)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and ac == bc, (what, kernel, any_hit, ac, bc)
    got.set_kernel(0)
    want.set_kernel(0)


# a. the refit ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", T.NAMES)
def test_refit_equals_the_rebuilt_scene(pkg, gpu, shapes, name):
    """twist, collapse and identity, each by the host path and by the device path on a side stream; the two paths take turns so
    that every refit starts from another geometry than the one it must produce"""
    import torch
    s = shapes(name)
    stream = torch.cuda.Stream()
    wanted = {}
    try:
        for deformation in ("twist", "collapse", "identity"):
            vd = deform(s.vertex_data, deformation)
            wanted[deformation] = (vd,) + expected_scene(pkg, s, vd)
        turn = 0
        for _ in range(2):
            for deformation in ("twist", "collapse", "identity"):
                how = ("host", "device")[turn % 2]
                turn += 1
                vd, want, boxes = wanted[deformation]
                what = f"{name}/{how}/{deformation}"
                stats = s.refit(vd, how, stream)
                assert_same_scene(s.scene, want, what)
                assert stats["exact_div_ok"] == int(R.exact_div_ok(boxes)) == 1, what
                assert stats["sah_cost"] == pytest.approx(R.sah_cost(s.tree, boxes), rel=1e-12, abs=0.0), what
                same_ray_results(pkg, s.scene, want, s.corners(vd), 40 + turn, what)
    finally:
        for _, want, _ in wanted.values():
            want.close()
        s.refit(s.vertex_data)


def test_leaf_root_through_the_device_pipeline(pkg, gpu, shapes):
    """shray_bvh_build_device + shray_flatten_device_tree + shray_scene_create_from_device over leaf_root's triangles: the builder
    leaves three triangles in one leaf, so this is the shape again, created on the other path.  The records and two walks equal
    the restatement, and a device refit equals the rebuilt scene."""
    import torch
    s = shapes("leaf_root")
    hip = pkg._native.load_hip()
    tv = np.ascontiguousarray(s.tree.triangle_vertices, np.int32)
    vd = np.ascontiguousarray(s.vertex_data, F)
    tree_handle, flat_handle = C.c_void_p(), C.c_void_p()
    i32, f32 = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    pkg._native.check(hip.shray_bvh_build_device(tv.ctypes.data_as(i32), len(tv), vd.ctypes.data_as(f32), len(vd), 9, None,
                                                 C.byref(tree_handle)))
    scene = None
    try:
        pkg._native.check(hip.shray_flatten_device_tree(tree_handle, 2048, C.byref(flat_handle)))
        scene = pkg.tracer.Scene.from_device(tree_handle, flat_handle, s.env)
        desc = pkg._native.TreeDesc()
        pkg._native.check(hip.shray_device_tree_download(tree_handle, C.byref(desc), None))
        built = R.TreeArrays.of(desc)
        assert built.node_count == 1 and built.negative[0] < 0 and built.triangles[0] == 3, "the builder's tree of leaf_root's triangles"
        assert sorted(map(tuple, built.triangle_vertices)) == sorted(map(tuple, tv))
        assert list(T.height_profile(built)) == [1]
        corners = vd[built.triangle_vertices][:, :, :3]
        ref = W.Restated.of_tree(built, corners, R.node_boxes(built, corners))
        assert_same_floats(scene.winding_data(), ref.records, "leaf_root from the device: node records")
        pts = make_points(s.arrays, 1000, seed=5)
        assert_bits(scene.closest_points(pts), PQ.closest(corners.reshape(-1), pts), "leaf_root from the device: closest points")
        for beta in BETAS:
            assert_same_floats(scene.winding_number(pts, beta=beta), ref.w(pts, beta), f"leaf_root from the device: beta {beta}")
        # the device refit of the device-created scene
        moved = deform(vd, "twist")
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            stats = scene.refit(torch.from_numpy(moved).cuda(), torch.from_numpy(built.triangle_vertices.copy()).cuda(), normal_offset=6,
                                stream_ptr=stream.cuda_stream)
        subject = type("Built", (), {"tree": built, "env": s.env})
        want, boxes = expected_scene(pkg, subject, moved)
        assert_same_scene(scene, want, "leaf_root from the device: twist")
        assert stats["exact_div_ok"] == 1 and stats["sah_cost"] == pytest.approx(R.sah_cost(built, boxes), rel=1e-12, abs=0.0)
        mcorners = moved[built.triangle_vertices][:, :, :3]
        same_ray_results(pkg, scene, want, mcorners, 9, "leaf_root from the device: twist")
        want.close()
        assert_same_floats(scene.winding_data(), W.Restated.of_tree(built, mcorners, boxes).records, "leaf_root from the device: records after the refit")
    finally:
        if scene is not None:
            scene.close()
        if flat_handle:
            hip.shray_device_flat_destroy(flat_handle)
        hip.shray_device_tree_destroy(tree_handle)


# b. the winding records and numbers ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", T.NAMES)
def test_winding_records_and_numbers(pkg, gpu, shapes, name):
    import torch
    s = shapes(name)
    try:
        ref, _ = s.restated()
        assert_same_floats(s.scene.winding_data(), ref.records, f"{name}: node records")
        pts = make_points(s.arrays, 1000, seed=17 + len(name))
        d_pts = dev(pts, 4)
        for beta in BETAS:
            # (the exact mode's restatement sums every triangle for every point: a quarter of the points on the large shapes)
            n = 250 if math.isinf(beta) and len(s.tree.triangle_vertices) > 5000 else len(pts)
            want = ref.w(pts[:n], beta)
            assert np.isnan(want).sum() > 0 and np.isfinite(want).sum() > 0.8 * n
            assert_same_floats(s.scene.winding_number(pts[:n], beta=beta), want, f"{name}: beta {beta}, host path")
            got = s.scene.winding_number(d_pts[:n], beta=beta)
            torch.cuda.current_stream().synchronize()
            assert_same_floats(got.cpu().numpy(), want, f"{name}: beta {beta}, device path")
        moved = deform(s.vertex_data, "twist")
        s.refit(moved)
        ref, _ = s.restated(moved)
        assert_same_floats(s.scene.winding_data(), ref.records, f"{name}: node records after the refit to twist")
        assert_same_floats(s.scene.winding_number(pts, beta=2.0), ref.w(pts, 2.0), f"{name}: beta 2 after the refit to twist")
    finally:
        s.refit(s.vertex_data)


# c. every walk on the two tiny shapes and on wide_by_one ------------------------------------------------------------------------

@pytest.mark.parametrize("name", WALK_SHAPES)
def test_point_walks(pkg, gpu, shapes, name):
    """closest_points, signed_distance, winding_signed_distance and triangles_within (K = 8, with counts), host and device paths"""
    import torch
    s = shapes(name)
    positions = s.arrays["vertex_positions"]
    pts = make_points(s.arrays, 1500, seed=3 + len(name))
    d_pts = dev(pts, 4)
    records = PQ.closest(positions, pts)
    assert (records["triangle"] >= 0).sum() > 700 and (records["triangle"] < 0).sum() > 0
    assert_bits(s.scene.closest_points(pts), records, f"{name}: closest points, host path")
    got = s.scene.closest_points(d_pts)
    torch.cuda.current_stream().synchronize()
    assert_bits(np.ascontiguousarray(got.cpu().numpy()).view(PQ.CLOSEST_DTYPE).reshape(-1), records, f"{name}: closest points, device path")

    derived = S.derive(np.asarray(positions, F))
    assert s.scene.surface_info() == derived["info"], name
    assert_same_floats(s.scene.sign_data(), derived["sign_data"], f"{name}: sign data")
    want = S.signed(pts, records, derived["sign_data"])
    got, rec = s.scene.signed_distance(pts, closest=True)
    assert_bits(rec, records, f"{name}: signed distance records")
    assert_same_floats(got, want, f"{name}: signed distance, host path")
    got = s.scene.signed_distance(d_pts)
    torch.cuda.current_stream().synchronize()
    assert_same_floats(got.cpu().numpy(), want, f"{name}: signed distance, device path")

    ref, _ = s.restated()
    want = W.winding_signed(records, ref.w(pts, 2.0))
    got, rec = s.scene.winding_signed_distance(pts, closest=True)
    assert_bits(rec, records, f"{name}: winding-signed records")
    assert_same_floats(got, want, f"{name}: winding-signed distance, host path")
    got = s.scene.winding_signed_distance(d_pts)
    torch.cuda.current_stream().synchronize()
    assert_same_floats(got.cpu().numpy(), want, f"{name}: winding-signed distance, device path")

    near_pts = near_cases.make_points(s.arrays, 1500, seed=8 + len(name))
    want8, want_n = NR.near(positions, near_pts, 8)
    assert (want_n > 0).sum() > 500 and (want_n == 0).sum() > 0
    got, n = s.scene.triangles_within(near_pts, max_near=8, counts=True)
    assert got.shape == want8.shape and np.array_equal(NR.as_bits(got), NR.as_bits(want8)), f"{name}: triangles within, host path"
    assert np.array_equal(n, want_n), f"{name}: counts within, host path"
    got, n = s.scene.triangles_within(dev(near_pts, 4), max_near=8, counts=True)
    torch.cuda.current_stream().synchronize()
    got = np.ascontiguousarray(got.cpu().numpy()).view(PQ.CLOSEST_DTYPE).reshape(-1, 8)
    assert np.array_equal(NR.as_bits(got), NR.as_bits(want8)), f"{name}: triangles within, device path"
    assert np.array_equal(n.cpu().numpy(), want_n), f"{name}: counts within, device path"


@pytest.mark.parametrize("name", WALK_SHAPES)
def test_ray_walks(pkg, gpu, shapes, name):
    """trace_all_hits (K = 8, with counts) and trace_rays (kernels 0 and 1, with the work counters), host and device paths"""
    import torch
    s = shapes(name)
    arrays = RQ.SceneArrays(s.arrays)
    o, d, tmax = random_rays(arrays, 2000, seed=23 + len(name))
    rays = pkg.tracer.make_rays(o, d, tmax)
    d_rays = dev(rays, 8)
    want, want_counts, _ = M.all_hits(arrays, o, d, tmax, max_hits=8)
    print(f"{name}: {int((want_counts > 0).sum())} of {len(rays)} rays cross a triangle")
    assert (want_counts > 0).sum() > 0 and (want_counts == 0).sum() > 0, name
    hits, counts = s.scene.trace_all_hits(rays, max_hits=8, counts=True)
    assert_same_records(hits, want, f"{name}: all hits, host path")
    assert np.array_equal(counts, want_counts), f"{name}: crossing counts, host path"
    d_hits, d_counts = s.scene.trace_all_hits(d_rays, max_hits=8, counts=True)
    torch.cuda.current_stream().synchronize()
    got = np.ascontiguousarray(d_hits.cpu().numpy()).view(RQ.HIT_DTYPE).reshape(len(rays), 8)
    assert_same_records(got, want, f"{name}: all hits, device path")
    assert np.array_equal(d_counts.cpu().numpy(), want_counts), f"{name}: crossing counts, device path"

    closest, tallies = RQ.trace(arrays, o, d, tmax)
    for kernel in (0, 1):
        s.scene.set_kernel(kernel)
        try:
            got, counters = s.scene.trace_rays(rays, counters=True)
            assert_same_hits(got, closest, f"{name}: closest hits, kernel {kernel}")
            for k in RQ.COUNTER_NAMES:
                assert counters[k] == tallies[k], (name, kernel, k, counters, tallies)
            assert_same_hits(s.scene.trace_rays(rays), closest, f"{name}: closest hits, kernel {kernel}, without counters")
        finally:
            s.scene.set_kernel(0)


# d. generations, on wide_by_one -------------------------------------------------------------------------------------------------

def test_two_refits_before_the_next_query(pkg, gpu, shapes):
    s = shapes("wide_by_one")
    try:
        pts = make_points(s.arrays, 1000, seed=61)
        first_w, first_records, first_sign = s.scene.winding_number(pts), s.scene.winding_data(), s.scene.sign_data()
        first_signed = s.scene.signed_distance(pts)
        s.refit(deform(s.vertex_data, "twist"))
        collapsed = deform(s.vertex_data, "collapse")
        s.refit(collapsed)
        ref, _ = s.restated(collapsed)
        assert_same_floats(s.scene.winding_number(pts), ref.w(pts, 2.0), "wide_by_one: numbers after twist, then collapse")
        assert_same_floats(s.scene.winding_data(), ref.records, "wide_by_one: records after twist, then collapse")
        derived = S.derive(s.corners(collapsed).reshape(-1))
        assert_same_floats(s.scene.sign_data(), derived["sign_data"], "wide_by_one: sign data after twist, then collapse")
        # ... and back: the derived data of the loaded vertices again, bit for bit
        s.refit(s.vertex_data)
        assert_same_floats(s.scene.winding_data(), first_records, "wide_by_one: records after the refit back")
        assert_same_floats(s.scene.sign_data(), first_sign, "wide_by_one: sign data after the refit back")
        assert_same_floats(s.scene.winding_number(pts), first_w, "wide_by_one: numbers after the refit back")
        assert_same_floats(s.scene.signed_distance(pts), first_signed, "wide_by_one: signed distances after the refit back")
    finally:
        s.refit(s.vertex_data)


def test_a_refused_refit_leaves_the_derived_state(pkg, gpu, shapes):
    """An index out of range is found by the validation pass, before the geometry generation is bumped: the scene's arrays, the
    records, the sign data and both queries are as before"""
    s = shapes("wide_by_one")
    pts = make_points(s.arrays, 1000, seed=62)
    before = snapshot(s.scene)
    records, sign = s.scene.winding_data(), s.scene.sign_data()
    w, signed = s.scene.winding_number(pts), s.scene.signed_distance(pts)
    bad = s.tree.triangle_vertices.copy()
    bad[len(bad) // 2, 1] = len(s.vertex_data)
    with pytest.raises(pkg._native.ShrayError) as err:
        s.scene.refit(deform(s.vertex_data, "twist"), bad, normal_offset=6)
    assert err.value.code == INVALID
    assert_unchanged(s.scene, before, "wide_by_one: a refused refit")
    assert_same_floats(s.scene.winding_data(), records, "wide_by_one: records after a refused refit")
    assert_same_floats(s.scene.sign_data(), sign, "wide_by_one: sign data after a refused refit")
    assert_same_floats(s.scene.winding_number(pts), w, "wide_by_one: numbers after a refused refit")
    assert_same_floats(s.scene.signed_distance(pts), signed, "wide_by_one: signed distances after a refused refit")


def test_device_refit_and_queries_on_a_side_stream(pkg, gpu, shapes):
    """A device refit on side stream A, then winding_number_into and signed_distance_into on A; then, with no host
    synchronisation, a blocking winding_data() and a query on the default stream: all of them see the refit geometry"""
    import torch
    s = shapes("wide_by_one")
    try:
        pts = make_points(s.arrays, 1000, seed=63)
        s.scene.winding_number(pts)            # the state exists, derived from the loaded vertices
        s.scene.signed_distance(pts)
        moved = deform(s.vertex_data, "twist")
        ref, _ = s.restated(moved)
        want = ref.w(pts, 2.0)
        corners = s.corners(moved).reshape(-1)
        want_signed = S.signed(pts, PQ.closest(corners, pts), S.derive(corners)["sign_data"])
        d_pts = dev(pts, 4)
        d_w = torch.full((len(pts),), -7.0, dtype=torch.float32, device="cuda")
        d_s = torch.full((len(pts),), -7.0, dtype=torch.float32, device="cuda")
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            d_vd, d_tv = torch.from_numpy(moved).cuda(), torch.from_numpy(s.tree.triangle_vertices.copy()).cuda()
            s.scene.refit(d_vd, d_tv, normal_offset=6, stream_ptr=side.cuda_stream)
            s.scene.winding_number_into(d_pts.data_ptr(), len(pts), d_w.data_ptr(), 2.0, side.cuda_stream)
            s.scene.signed_distance_into(d_pts.data_ptr(), len(pts), d_s.data_ptr(), 0, side.cuda_stream)
        assert_same_floats(s.scene.winding_data(), ref.records, "wide_by_one: records, blocking, after the side stream's refit")
        d_main = s.scene.winding_number(d_pts)
        assert_same_floats(d_main.cpu().numpy(), want, "wide_by_one: the default stream after the side stream's refit")
        side.synchronize()
        assert_same_floats(d_w.cpu().numpy(), want, "wide_by_one: the side stream's winding numbers")
        assert_same_floats(d_s.cpu().numpy(), want_signed, "wide_by_one: the side stream's signed distances")
    finally:
        s.refit(s.vertex_data)


# e. fp16 normals at the conversion's edges --------------------------------------------------------------------------------------

HALF_EDGES = np.array([
    0x00000000,                          # 0
    0x33000000, 0x32ffffff, 0x33000001,  # 2^-25 (a tie with 0: to even, 0), the float below it, the float above it (the first to round up)
    0x33800000,                          # 2^-24, the smallest subnormal half
    0x33c00000, 0x34200000,              # 1.5 and 2.5 * 2^-24: ties between subnormals, to 2 from the odd 1 and to 2 from the even 2
    0x38800000, 0x387fffff,              # 2^-14, the smallest normal half, and the float below it (rounds up to it)
    0x3f801000, 0x3f803000,              # 1 + 2^-11 and 1 + 3 * 2^-11: ties in the normal range with an even and an odd kept bit
    0x477fe000, 0x477fefff, 0x477ff000,  # 65504 (the largest half), 65519.996 (rounds down to it), 65520 (a tie: to infinity)
    0x7149f2ca,                          # 1e30: infinity
    0x3f000000, 0x3eaaaaab, 0x358637bd, 0x447a0666, 0x3dcccccd, 0x45001000, 0x477fd000, 0x0da24260,   # ordinary values, a tie at 2049, 1e-30
    0x387fe000, 0x387ff000, 0x33ffffff, 0x34000001,   # more about the subnormal range's ends and its first tie
], np.uint32)


@pytest.mark.parametrize("how", ["host", "device"])
def test_half_normals_at_the_conversions_edges(pkg, gpu, shapes, how):
    """one_branch's 27 normal components are the table, signs alternating (the host path starts with +, the device path with -, so
    that every value is converted with both signs, -0 among them)"""
    import torch
    s = shapes("one_branch")
    assert len(HALF_EDGES) == 27 == s.vertex_data[:, 6:9].size
    try:
        signs = ((np.arange(27) + (how == "device")) % 2).astype(np.uint32) << 31
        table = (HALF_EDGES | signs).view(F)
        assert np.isfinite(table).all()
        vd = s.vertex_data.copy()
        corner_normals = table.reshape(3, 3, 3)                        # [triangle, corner, xyz], the scene's order
        vd[s.tree.triangle_vertices.reshape(-1), 6:9] = corner_normals.reshape(9, 3)
        want = scene_ref.half_bits(table)
        with np.errstate(over="ignore"):
            assert np.array_equal(want, table.astype(np.float16).view(np.uint16))      # (numpy's own round-to-nearest-even)
        assert {0x0000, 0x8000, 0x0001, 0x8001, 0x0002, 0x0400, 0x3c00, 0x3c02, 0x7bff, 0x7c00, 0xfc00} <= set(
            int(x) for x in np.concatenate([want, want ^ 0x8000]))
        s.refit(vd, how, torch.cuda.Stream())
        got = s.scene.derived_arrays()["normals16"]
        assert np.array_equal(got, want), f"one_branch/{how}: halves {[hex(x) for x in got]}, expected {[hex(x) for x in want]}"
        assert np.array_equal(s.scene.geometry()["vertex_normals"].view(np.uint32), table.view(np.uint32)), f"one_branch/{how}: fp32 normals"
        rebuilt, _ = expected_scene(pkg, s, vd)                        # sd_half_normals, the other device caller
        try:
            assert np.array_equal(rebuilt.derived_arrays()["normals16"], want), f"one_branch/{how}: the rebuilt scene's halves"
            assert_same_scene(s.scene, rebuilt, f"one_branch/{how}: the table as normals")
        finally:
            rebuilt.close()
    finally:
        s.refit(s.vertex_data)
