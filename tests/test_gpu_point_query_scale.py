"""The point-query family on scenes scaled by S = 2^k, on the GPU, every byte against the restatements: the cells of
tests/point_scale_cases.py (scenes loaded under GEOMETRY_SCALE, the restatement run on that world's own arrays) through
closest_points (host and device paths), triangles_within (K 1, 8, SHRAY_NEAR_MAX, with and without counts) and near_counts,
signed_distance with sign_data and surface_info, winding_data, winding_number (beta 2, 0.5, inf) and winding_signed_distance;
the S = 1 class of special coordinates through all four; a refit that changes the scene's magnitude by 2^-40 and 2^40 under
all four on one stream; DeviceWorld under GEOMETRY_SCALE; a count split over two launches at an outside cell; and the counters
where every dist2 ties.  tests/test_point_scale_reference.py pins the cells and the restatements on the CPU.

Outside the covariant range the products underflow to subnormals and 0 and overflow to inf and NaN: what is compared is the
header's arithmetic itself -- no flushed subnormal, no approximate reciprocal or square root, the selects (not min / max
instructions) over NaN, and a walk that prunes nothing on 0 > 0 or inf > inf."""
import math

import numpy as np
import pytest

import near_ref as NR
import point_query_ref as R
import point_scale_cases as PC
import ray_scale_cases as X
import refit_ref
import sdf_ref as SD
import winding_ref as W
from test_gpu_near import assert_bits as assert_near_bits
from test_gpu_near import device_points, records as near_records
from test_gpu_point_query import assert_bits, device_query, scene_path
from test_gpu_signed_distance import assert_same_floats, device_signed

pytestmark = pytest.mark.gpu

F = np.float32
CASES = [(name, k) for name in PC.SCENES for k in PC.S_EXPONENTS]
NEAR_MAX = 64   # SHRAY_NEAR_MAX
BETAS = (2.0, 0.5, math.inf)
_scenes = {}
_memo = {}


def memo(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def resident(pkg, name, k):
    """(world, its flattened arrays, the resident scene) of the scene loaded under GEOMETRY_SCALE = 2^k, once per module"""
    if (name, k) not in _scenes:
        world = X.load_scaled(pkg, name, k)
        arrays = world.arrays()
        want = X.base_arrays(pkg, name).positions * F(2.0 ** k)
        assert np.array_equal(X.triangle_rows(arrays["vertex_positions"]), X.triangle_rows(want)), (name, k)
        _scenes[(name, k)] = (world, arrays, pkg.Scene(world.flatten()))
    return _scenes[(name, k)]


@pytest.fixture(scope="module", autouse=True)
def close_the_module_scenes():
    yield
    for world, _, scene in _scenes.values():
        scene.close()
        world.close()
    _scenes.clear()
    _memo.clear()


def closest_want(pkg, name, k):
    """(points, the restatement's records on the scaled world's own arrays), once"""
    def make():
        pts = PC.points(pkg, name, k)
        return pts, R.closest(resident(pkg, name, k)[1]["vertex_positions"], pts)
    return memo(("closest", name, k), make)


def check_closest(pkg, scene, pts, want, what):
    assert_bits(scene.closest_points(pts), want, what + ", host path")
    assert_bits(device_query(pkg, scene, pts), want, what + ", device path")


def check_near(scene, pts, want64, want_n, what):
    import torch
    for k in (1, 8, NEAR_MAX):
        for counts in (True, False):
            got, n = scene.triangles_within(pts, max_near=k, counts=counts)
            assert_near_bits(got, want64[:, :k], f"{what}, K {k}, counts {counts}, host path")
            assert (np.array_equal(n, want_n) if counts else n is None), (what, k)
            d_got, d_n = scene.triangles_within(device_points(pts), max_near=k, counts=counts)
            torch.cuda.current_stream().synchronize()
            assert_near_bits(near_records(d_got, k), want64[:, :k], f"{what}, K {k}, counts {counts}, device path")
            assert (np.array_equal(d_n.cpu().numpy(), want_n) if counts else d_n is None), (what, k)
    assert np.array_equal(scene.near_counts(pts), want_n), what
    assert np.array_equal(scene.near_counts(device_points(pts)).cpu().numpy(), want_n), what


def check_signed(pkg, scene, pts, records, derived, what):
    assert scene.surface_info() == derived["info"], what
    assert_same_floats(scene.sign_data(), derived["sign_data"], what + ", sign data")
    expect = SD.signed(pts, records, derived["sign_data"])
    got, rec = scene.signed_distance(pts, closest=True)
    assert_bits(rec, records, what + ", host path records")
    assert_same_floats(got, expect, what + ", host path")
    dgot, drec = device_signed(scene, pts)
    assert_bits(drec, records, what + ", device path records")
    assert_same_floats(dgot, expect, what + ", device path")


def check_winding(scene, ref, pts, records, what):
    import torch
    assert_same_floats(scene.winding_data(), ref.records, what + ", node records")
    d_pts = device_points(pts)
    w2 = None
    for beta in BETAS:
        want = ref.w(pts, beta)
        w2 = want if beta == 2.0 else w2
        assert_same_floats(scene.winding_number(pts, beta=beta), want, f"{what}, beta {beta}, host path")
        got = scene.winding_number(d_pts, beta=beta)
        torch.cuda.current_stream().synchronize()
        assert_same_floats(got.cpu().numpy(), want, f"{what}, beta {beta}, device path")
    want = W.winding_signed(records, w2)
    got, rec = scene.winding_signed_distance(pts, closest=True)
    assert_bits(rec, records, what + ", winding-signed records")
    assert_same_floats(got, want, what + ", winding-signed, host path")
    dgot, drec = scene.winding_signed_distance(d_pts, closest=True)
    torch.cuda.current_stream().synchronize()
    assert_bits(np.ascontiguousarray(drec.cpu().numpy()).view(R.CLOSEST_DTYPE).reshape(-1), records, what + ", device path records")
    assert_same_floats(dgot.cpu().numpy(), want, what + ", winding-signed, device path")


@pytest.mark.parametrize("name, k", CASES)
def test_closest_points(pkg, gpu, name, k):
    scene = resident(pkg, name, k)[2]
    pts, want = closest_want(pkg, name, k)
    hits = (want["triangle"] >= 0).mean()
    assert 0.05 <= hits <= 0.95, (name, k, hits)
    check_closest(pkg, scene, pts, want, f"{name}, S 2^{k}")


@pytest.mark.parametrize("name, k", CASES)
def test_triangles_within(pkg, gpu, name, k):
    _, arrays, scene = resident(pkg, name, k)
    pts = PC.points(pkg, name, k, "near")
    want64, want_n = NR.near(arrays["vertex_positions"], pts, NEAR_MAX)
    assert (want_n > 0).mean() >= 0.05 and (want_n == 0).mean() >= 0.05 and (want_n > NEAR_MAX).mean() >= 0.05, (name, k)
    check_near(scene, pts, want64, want_n, f"{name}, S 2^{k}")
    got1, _ = scene.triangles_within(pts, max_near=1, counts=False)
    assert_bits(got1[:, 0], scene.closest_points(pts), f"{name}, S 2^{k}, K = 1 against closest_points")


@pytest.mark.parametrize("name, k", CASES)
def test_signed_distance(pkg, gpu, name, k):
    _, arrays, scene = resident(pkg, name, k)
    pts, records = closest_want(pkg, name, k)
    check_signed(pkg, scene, pts, records, SD.derive(arrays["vertex_positions"]), f"{name}, S 2^{k}")


@pytest.mark.parametrize("name, k", CASES)
def test_winding(pkg, gpu, name, k):
    world, _, scene = resident(pkg, name, k)
    pts, records = closest_want(pkg, name, k)
    check_winding(scene, W.Restated(world), pts, records, f"{name}, S 2^{k}")


@pytest.mark.parametrize("name", PC.SCENES)
def test_special_coordinates(pkg, gpu, name):
    """S = 1: coordinates of p at +-0, the smallest denormal, 2^-64, 2^63 and 2^64, through all four clients"""
    world, arrays, scene = resident(pkg, name, 0)
    pos = arrays["vertex_positions"]
    pts = PC.special_points(pkg, name)
    records = R.closest(pos, pts)
    assert 0.05 <= (records["triangle"] >= 0).mean() <= 0.95
    what = f"{name}, special coordinates"
    check_closest(pkg, scene, pts, records, what)
    npts = PC.special_points(pkg, name, "near")
    want64, want_n = NR.near(pos, npts, NEAR_MAX)
    check_near(scene, npts, want64, want_n, what)
    check_signed(pkg, scene, pts, records, SD.derive(pos), what)
    check_winding(scene, W.Restated(world), pts, records, what)


def test_a_refit_that_changes_the_magnitude(pkg, gpu):
    """A resident S = 1 lobed_528 is refit on a side stream to positions * 2^-40, then to positions * 2^40 (device form), and
    after each refit all four queries run on that stream with no host synchronisation in between.  Each equals the restatement
    of the refit scene (boxes by tests/refit_ref.py): no sign data, node record, tree height or radius survives from the old
    scale."""
    import torch
    name = "lobed_528"
    world = X.load_scaled(pkg, name, 0)
    scene = pkg.Scene(world.flatten())
    try:
        arrays = world.arrays()
        tree = refit_ref.TreeArrays.of(world.export_tree())
        pos1 = np.asarray(arrays["vertex_positions"], F).reshape(-1, 3)
        base = {"vertex_positions": pos1.reshape(-1), "group_boxmin": arrays["group_boxmin"], "group_boxmax": arrays["group_boxmax"]}
        import near_cases
        from test_gpu_point_query import make_points
        pts1, npts1 = make_points(base, 2000, seed=61), near_cases.make_points(base, 2000, seed=62)
        scene.signed_distance(pts1), scene.winding_number(pts1)     # derived at the old scale first
        n = len(pts1)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        runs = []
        with torch.cuda.stream(side):
            for k in (-40, 40):
                pts, npts = PC.scaled_points(pts1, k), PC.scaled_points(npts1, k)
                d_pos = torch.from_numpy(pos1 * F(2.0 ** k)).cuda()
                d_pts, d_npts = device_points(pts), device_points(npts)
                out = {"closest": torch.full((n, 8), -7, dtype=torch.int32, device="cuda"),
                       "near": torch.full((n, 8, 8), -7, dtype=torch.int32, device="cuda"),
                       "counts": torch.full((n,), -7, dtype=torch.int32, device="cuda"),
                       "signed": torch.full((n,), -7.0, device="cuda"), "signed_rec": torch.full((n, 8), -7, dtype=torch.int32, device="cuda"),
                       "w2": torch.full((n,), -7.0, device="cuda"), "winf": torch.full((n,), -7.0, device="cuda"),
                       "wsigned": torch.full((n,), -7.0, device="cuda")}
                s = side.cuda_stream
                scene.refit(d_pos, stream_ptr=s)
                scene.closest_points_into(d_pts.data_ptr(), n, out["closest"].data_ptr(), s)
                scene.triangles_within_into(d_npts.data_ptr(), n, out["near"].data_ptr(), out["counts"].data_ptr(), max_near=8, stream_ptr=s)
                scene.signed_distance_into(d_pts.data_ptr(), n, out["signed"].data_ptr(), out["signed_rec"].data_ptr(), s)
                scene.winding_number_into(d_pts.data_ptr(), n, out["w2"].data_ptr(), 2.0, s)
                scene.winding_number_into(d_pts.data_ptr(), n, out["winf"].data_ptr(), math.inf, s)
                scene.winding_signed_distance_into(d_pts.data_ptr(), n, out["wsigned"].data_ptr(), 0, 2.0, s)
                runs.append((k, pts, npts, out, d_pos, d_pts, d_npts))
        side.synchronize()
        for k, pts, npts, out, *_ in runs:
            what = f"after the refit to 2^{k}"
            pos = (pos1 * F(2.0 ** k)).reshape(-1)
            want = R.closest(pos, pts)
            assert 0.05 <= (want["triangle"] >= 0).mean() <= 0.95
            got = np.ascontiguousarray(out["closest"].cpu().numpy()).view(R.CLOSEST_DTYPE).reshape(-1)
            assert_bits(got, want, what + ", closest")
            want8, want_n = NR.near(pos, npts, 8)
            assert_near_bits(near_records(out["near"], 8), want8, what + ", near")
            assert np.array_equal(out["counts"].cpu().numpy(), want_n), what
            derived = SD.derive(pos)
            rec = np.ascontiguousarray(out["signed_rec"].cpu().numpy()).view(R.CLOSEST_DTYPE).reshape(-1)
            assert_bits(rec, want, what + ", signed records")
            assert_same_floats(out["signed"].cpu().numpy(), SD.signed(pts, want, derived["sign_data"]), what + ", signed")
            ref = W.Restated(world, positions=pos, boxes=refit_ref.node_boxes(tree, pos.reshape(-1, 3)))
            w2 = ref.w(pts, 2.0)
            assert_same_floats(out["w2"].cpu().numpy(), w2, what + ", winding beta 2")
            assert_same_floats(out["winf"].cpu().numpy(), ref.w(pts, math.inf), what + ", winding exact")
            assert_same_floats(out["wsigned"].cpu().numpy(), W.winding_signed(want, w2), what + ", winding-signed")
        # the scene now holds the last refit's derived state
        k, pos = 40, (pos1 * F(2.0 ** 40)).reshape(-1)
        derived = SD.derive(pos)
        assert scene.surface_info() == derived["info"]
        assert_same_floats(scene.sign_data(), derived["sign_data"], "sign data after the refits")
        ref = W.Restated(world, positions=pos, boxes=refit_ref.node_boxes(tree, pos.reshape(-1, 3)))
        assert_same_floats(scene.winding_data(), ref.records, "node records after the refits")
        assert derived["info"]["degenerate_triangles"] == len(pos) // 9     # the old scale had none: the count is re-derived
    finally:
        scene.close()
        world.close()


@pytest.mark.parametrize("k", [-40, 40])
def test_device_world_built_under_geometry_scale(pkg, gpu, k):
    """DeviceWorld parses the file under GEOMETRY_SCALE and builds the tree on the device: the same triangle order as the
    host-built scene's at that scale, and the same answers from all four clients, byte for byte"""
    import os
    name = "lobed_528"
    _, arrays, scene = resident(pkg, name, k)
    before = os.environ.get("GEOMETRY_SCALE")
    os.environ["GEOMETRY_SCALE"] = X.scale_string(k)
    try:
        dw = pkg.tracer.DeviceWorld(scene_path(name))
    finally:
        if before is None:
            del os.environ["GEOMETRY_SCALE"]
        else:
            os.environ["GEOMETRY_SCALE"] = before
    try:
        flat = dw.flat_arrays()
        assert np.array_equal(np.asarray(flat["vertex_positions"], F).view(np.uint32), np.asarray(arrays["vertex_positions"], F).view(np.uint32))
        pts, want = closest_want(pkg, name, k)
        check_closest(pkg, dw, pts, want, f"DeviceWorld, S 2^{k}")
        npts = PC.points(pkg, name, k, "near")
        got, n = dw.triangles_within(npts, max_near=8)
        host, host_n = scene.triangles_within(npts, max_near=8)
        assert_near_bits(got, host, f"DeviceWorld, S 2^{k}, near")
        assert np.array_equal(n, host_n)
        assert dw.surface_info() == scene.surface_info()
        assert_same_floats(dw.sign_data(), scene.sign_data(), "DeviceWorld, sign data")
        assert_same_floats(dw.signed_distance(pts), scene.signed_distance(pts), "DeviceWorld, signed")
        assert_same_floats(dw.winding_data(), scene.winding_data(), "DeviceWorld, node records")
        for beta in BETAS:
            assert_same_floats(dw.winding_number(pts, beta=beta), scene.winding_number(pts, beta=beta), f"DeviceWorld, beta {beta}")
        assert_same_floats(dw.winding_signed_distance(pts), scene.winding_signed_distance(pts), "DeviceWorld, winding-signed")
    finally:
        dw.close()


def test_a_count_split_over_launches_at_an_outside_cell(pkg, gpu):
    """2^24 + 3000 points (one launch holds 2^24) on small_trisrc at S = 2^-40, an outside cell: far points with radius 0 are
    misses; the last launch's points and cell points scattered over the first launch are restated."""
    import torch
    name, k = "small_trisrc", -40
    assert PC.flag("closest", name, k) == PC.OUTSIDE
    _, arrays, scene = resident(pkg, name, k)
    pos = arrays["vertex_positions"]
    n = (1 << 24) + 3000
    from test_gpu_point_query import make_points
    real = PC.scaled_points(make_points(PC.as_dict(X.base_arrays(pkg, name)), 3000 + 1024, seed=33), k)
    tail, spread = real[:3000], real[3000:]
    far = np.zeros(1, R.POINT_DTYPE)
    far["p"] = (1e6, -2e6, 3e6)
    far = PC.scaled_points(far, k)
    d_pts = device_points(far).repeat(n, 1)
    d_pts[n - 3000:] = device_points(tail)
    sample = torch.from_numpy(np.random.default_rng(1).choice(n - 3000, len(spread), replace=False)).cuda()
    d_pts[sample] = device_points(spread)
    d_out = torch.empty((n, 8), dtype=torch.int32, device="cuda")
    scene.closest_points_into(d_pts.data_ptr(), n, d_out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.current_stream().synchronize()

    def rec(t):
        return np.ascontiguousarray(t.cpu().numpy()).view(R.CLOSEST_DTYPE).reshape(-1)

    assert_bits(rec(d_out[n - 3000:]), R.closest(pos, tail), "the last launch's points")
    assert_bits(rec(d_out[sample]), R.closest(pos, spread), "points of the first launch")
    rest = torch.ones(n - 3000, dtype=torch.bool, device="cuda")
    rest[sample] = False
    far_record = torch.from_numpy(R.as_bits(R.closest(pos, far)).view(np.int32).copy()).cuda()
    assert far_record[0, 6] == -1
    assert bool((d_out[: n - 3000][rest] == far_record).all())


@pytest.mark.parametrize("name", PC.SCENES)
@pytest.mark.parametrize("k", [PC.ALL_TIES_UNDERFLOW, 64])
def test_nothing_is_pruned_where_every_dist2_ties(pkg, gpu, name, k):
    """Where every triangle's dist2 is one value c for a point (0 at S = 2^-90 for every point; +inf at S = 2^64 for the far
    points) and max_dist2 >= c, the definition is "lowest index over the whole scene", every box bound is at most c, and
    `bound > best` is false at 0 > 0 and inf > inf: the walk may skip nothing.  The expected count is derived here from the
    pairs' dist2 (the brute force of the definition), not from the kernel: triangle_tests = tied points x triangles, and
    leaf_visits = tied points x leaves."""
    world = X.load_scaled(pkg, name, k)
    scene = pkg.Scene(world.flatten())
    try:
        arrays = world.arrays()
        pos = arrays["vertex_positions"]
        T = len(pos) // 9
        pts = PC.points(pkg, name, k)
        with np.errstate(all="ignore"):
            d2 = NR.pair_dist2(R.NumpyOps, pos, pts)
            tied = NR.walked(pts) & (d2 == d2[:, :1]).all(1) & (d2[:, 0] <= pts["max_dist2"])
        if k == PC.ALL_TIES_UNDERFLOW:
            assert np.array_equal(tied, NR.walked(pts)) and (d2[tied] == 0).all()
        else:
            assert tied.sum() >= 100 and np.isinf(d2[tied]).all()
        tree = refit_ref.TreeArrays.of(world.export_tree())
        leaves = int((tree.negative < 0).sum())
        for subset in (pts[tied], pts) if k == PC.ALL_TIES_UNDERFLOW else (pts[tied],):
            walked = int(NR.walked(subset).sum())
            got, c = scene.closest_points(subset, counters=True)
            assert_bits(got, R.closest(pos, subset), f"{name}, S 2^{k}, the tied points")
            assert (got["triangle"][NR.walked(subset)] == 0).all()
            assert c["triangle_tests"] == walked * T and c["leaf_visits"] == walked * leaves, (c, walked, T, leaves)
            assert c["node_visits"] == walked * tree.node_count and c["samples"] == len(subset), (c, walked, tree.node_count)
    finally:
        scene.close()
        world.close()
