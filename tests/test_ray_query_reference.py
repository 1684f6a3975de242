"""The CPU restatement of the ray query (tests/ray_query_ref.py) pinned to analytic answers and to the CPU oracle:
hand-built one-leaf scenes with known t, u, v; and on two scene files, the camera rays of a frame give the oracle's first
triangle per pixel and its work counters for a frame that traces exactly those rays."""
import os

import numpy as np
import pytest

import helpers
import ray_query_ref as R

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def hand_arrays(scene: helpers.HandScene) -> dict:
    """The dict World.arrays() gives, for a hand-built scene."""
    k, d = scene.keep, scene.desc
    ng = d.group_count
    out = {"vertex_positions": k["pos"][:d.vertex_count].reshape(-1), "group_boxmin": k["bmin"][:ng].reshape(-1),
           "group_boxmax": k["bmax"][:ng].reshape(-1), "group_objects": k["obj"][:ng].reshape(-1), "tree_root": d.tree_root}
    for code in range(8):
        out[f"group_hitmiss_{code}"] = k["hm"][code, :ng].reshape(-1)
    return out


# v0 = origin, v1 on x, v2 on y: a point (x, y, 0) inside has uvw = (1 - x - y, x, y)
XY_TRIANGLE = [[0, 0, 0], [1, 0, 0], [0, 1, 0]]
YZ_TRIANGLE = [[0, 0, 0], [0, 1, 0], [0, 0, 1]]


def one_ray(arrays, origin, direction, tmax=1e7, **kw):
    hits, counts = R.trace(arrays, [origin], [direction], [tmax], **kw)
    return hits[0], counts


def test_analytic_hit_down_the_z_axis():
    arrays = hand_arrays(helpers.single_leaf_scene([XY_TRIANGLE]))
    h, c = one_ray(arrays, (0.25, 0.5, 2.0), (0.0, 0.0, -1.0))
    assert h["triangle"] == 0
    assert h["t"] == F(2.0) and h["u"] == F(0.25) and h["v"] == F(0.5), h
    assert c == {"node_visits": 1, "leaf_visits": 1, "triangle_tests": 1, "traversals": 1, "bad_hits": 0}


@pytest.mark.parametrize("dx,dy", [(-0.0, 0.0), (0.0, -0.0), (-0.0, -0.0)])
def test_negative_zero_component_misses_the_box(dx, dy):
    # the shader's slab test (fs:204-213): d >= 0 holds for -0, so the low plane is taken as the entry plane, and its
    # quotient (lo - o) / -0 with o inside the slab is +inf: the box is missed
    arrays = hand_arrays(helpers.single_leaf_scene([XY_TRIANGLE]))
    h, c = one_ray(arrays, (0.25, 0.5, 2.0), (dx, dy, -1.0))
    assert h["triangle"] == R.HIT_MISS and h["t"] == F(1e7)
    assert c == {"node_visits": 1, "leaf_visits": 1, "triangle_tests": 0, "traversals": 1, "bad_hits": 0}


def test_analytic_hit_along_the_x_axis():
    arrays = hand_arrays(helpers.single_leaf_scene([YZ_TRIANGLE]))
    h, _ = one_ray(arrays, (-3.0, 0.125, 0.375), (1.0, 0.0, 0.0))
    assert h["triangle"] == 0
    assert h["t"] == F(3.0)
    # within 1 ulp of the analytic barycentrics
    assert abs(int(np.float32(h["u"]).view(np.int32)) - int(F(0.125).view(np.int32))) <= 1
    assert abs(int(np.float32(h["v"]).view(np.int32)) - int(F(0.375).view(np.int32))) <= 1


def test_analytic_scaled_direction_is_not_normalised():
    arrays = hand_arrays(helpers.single_leaf_scene([XY_TRIANGLE]))
    h, _ = one_ray(arrays, (0.25, 0.25, 2.0), (0.0, 0.0, -4.0))
    assert h["triangle"] == 0 and h["t"] == F(0.5)


def test_tmax_cuts_the_hit_off():
    arrays = hand_arrays(helpers.single_leaf_scene([XY_TRIANGLE]))
    o, d = (0.25, 0.5, 2.0), (0.0, 0.0, -1.0)
    h, _ = one_ray(arrays, o, d, tmax=1.5)
    assert h["triangle"] == R.HIT_MISS and h["t"] == F(1.5)
    # a hit exactly at tmax is accepted by the walk (fs:327 rejects only d > hit.t) but not reported: t < tmax fails
    h, _ = one_ray(arrays, o, d, tmax=2.0)
    assert h["triangle"] == R.HIT_MISS and h["t"] == F(2.0) and h["u"] == F(0.25)
    h, _ = one_ray(arrays, o, d, tmax=np.nextafter(F(2.0), F(3.0)))
    assert h["triangle"] == 0 and h["t"] == F(2.0)


@pytest.mark.parametrize("tmax", [0.0, -0.0, -1.0, float("nan"), -float("inf")])
def test_tmax_not_positive_is_a_miss_without_traversal(tmax):
    arrays = hand_arrays(helpers.single_leaf_scene([XY_TRIANGLE]))
    h, c = one_ray(arrays, (0.25, 0.5, 2.0), (0.0, 0.0, -1.0), tmax=tmax)
    assert h["triangle"] == R.HIT_MISS
    assert np.array_equal(np.array([h["t"]], F), np.array([tmax], F), equal_nan=True)
    assert c["traversals"] == 0 and c["node_visits"] == 0


def test_infinite_tmax_hits_and_misses():
    arrays = hand_arrays(helpers.single_leaf_scene([XY_TRIANGLE]))
    h, _ = one_ray(arrays, (0.25, 0.5, 2.0), (0.0, 0.0, -1.0), tmax=np.inf)
    assert h["triangle"] == 0 and h["t"] == F(2.0)
    h, c = one_ray(arrays, (0.25, 0.5, 2.0), (0.0, 0.0, 1.0), tmax=np.inf)
    assert h["triangle"] == R.HIT_MISS and h["t"] == np.inf and c["traversals"] == 1


def test_leaf_cap_limits_the_triangles_tested():
    # three stacked triangles in one leaf, the nearest last: max_leaf_tests = 2 never sees it
    tris = [[[x + 0 * z for x in v[:2]] + [z] for v in XY_TRIANGLE] for z in (0.0, 0.5, 1.0)]
    arrays = hand_arrays(helpers.single_leaf_scene(tris))
    h, c = one_ray(arrays, (0.25, 0.25, 2.0), (0.0, 0.0, -1.0))
    assert h["triangle"] == 2 and h["t"] == F(1.0) and c["triangle_tests"] == 3
    h, c = one_ray(arrays, (0.25, 0.25, 2.0), (0.0, 0.0, -1.0), max_leaf_tests=2)
    assert h["triangle"] == 1 and h["t"] == F(1.5) and c["triangle_tests"] == 2


def test_iteration_cap_is_the_bad_hit(pkg):
    world = pkg.World(helpers.small_trisrc())
    arrays = world.arrays()
    params = world.frame_params(16, 16, material=0)
    o, d = R.camera_rays(_oracle(), params, 16, 16)
    hits, c = R.trace(arrays, o, d, F(1e7), max_bvh_iterations=1)
    # the root is a branch: after one visit every ray that has not finished is a bad hit
    capped = hits["triangle"] == R.HIT_CAP
    assert capped.sum() == c["bad_hits"] > 0
    assert (hits["t"][capped] == F(-1)).all()
    full, c_full = R.trace(arrays, o, d, F(1e7), max_bvh_iterations=0)
    assert c_full["bad_hits"] == 0 and (full["triangle"] != R.HIT_CAP).all()


def _oracle():
    import oracle
    oracle.load()
    return oracle


@pytest.mark.parametrize("scene", ["small_trisrc", "lobed_528"])
def test_camera_rays_match_the_oracle(pkg, oracle_mod, scene):
    path = helpers.small_trisrc() if scene == "small_trisrc" else os.path.join(GOLDEN, "lobed_528.trisrc")
    world = pkg.World(path)
    W = H = 128
    params = world.frame_params(W, H, material=0)
    params.bounce_count = 1                       # the frame traces the camera rays and nothing else
    params.diffuse_color[:] = [0.0, 0.0, 0.0]
    env = pkg.scenes.environment_constant()
    desc = world.flatten()
    _, counters, _, first, _, _ = oracle_mod.render_with_paths(desc, env, params, W, H)
    _, counters_plain = oracle_mod.render(desc, env, params, W, H)
    o, d = R.camera_rays(oracle_mod, params, W, H)
    hits, c = R.trace(world.arrays(), o, d, F(1e7), max_bvh_iterations=params.max_bvh_iterations,
                      max_leaf_tests=params.max_leaf_tests)
    tri = np.where(hits["triangle"] == R.HIT_CAP, -1, hits["triangle"]).reshape(H, W)
    assert (tri >= 0).sum() > W * H // 10, "the frame should show the object"
    bad = np.argwhere(tri != first)
    assert not len(bad), f"{len(bad)} pixels disagree with the oracle's first triangle, first {bad[:5].tolist()}"
    for name in R.COUNTER_NAMES:
        assert c[name] == counters_plain[name] == counters[name], (name, c, counters_plain)
