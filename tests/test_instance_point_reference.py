"""The CPU side of the instanced closest-point query (include/shader_ray_instance_point.h), on
tests/instance_point_ref.py: the exactness of the image-box cull bit for bit (every fp32 world corner lies in the image box of
any box of exact vertex minima and maxima, and the box bound of the image box is never above a dist2 below it) over maps of
every kind at scales 2^-30 to 2^30; a numpy restatement of the walk that skips only by that bound and returns the brute-force
record byte for byte; the identity, signed-zero and power-of-two scaling consequences of the header."""
import os

import numpy as np
import pytest

import instance_point_ref as IP
import point_query_ref as R

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EYE = np.eye(3, 4, dtype=F)


def rotation(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def signed_permutation(rng):
    A = np.zeros((3, 3))
    A[np.arange(3), rng.permutation(3)] = rng.choice([-1.0, 1.0], 3)
    return A


KINDS = ("rotation_scale", "sheared", "sparse", "signed_permutation", "general")


def random_map(rng, kind, scale=1.0):
    """a [3, 4] float32 map of `kind` (a rotation times a scale, sheared, sparse, a signed permutation, general) at overall
    scale `scale`"""
    if kind == "rotation_scale":
        A = rotation(rng) * rng.uniform(0.5, 2.0)
    elif kind == "sheared":
        A = rotation(rng) @ (np.eye(3) + np.triu(rng.normal(size=(3, 3)), 1)) @ np.diag(rng.uniform(0.5, 2.0, 3))
    elif kind == "sparse":
        A = rng.normal(size=(3, 3)) * (rng.random((3, 3)) < 0.5)
        A[np.arange(3), rng.permutation(3)] += rng.choice([-1.0, 1.0], 3) * rng.uniform(0.5, 2.0, 3)
    elif kind == "signed_permutation":
        A = signed_permutation(rng)
    else:
        A = rng.normal(size=(3, 3))
    b = rng.normal(size=3) * 2 * (rng.random(3) < 0.8)
    return (np.concatenate([A, b[:, None]], axis=1) * scale).astype(F)


bound, pair_dist2, median_tree, restated_walk = IP.bound, IP.pair_dist2, IP.median_tree, IP.restated_walk      # (they live there)


# 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_the_image_box_bound_is_exact(kind):
    """Per map 8 "nodes" of 1 to 11 random triangles with the exact minima and maxima of their object corners, 16 points each,
    around and inside the world node."""
    rng = np.random.default_rng(KINDS.index(kind) + 200)
    pairs = 0
    for m in range(60):
        M = random_map(rng, kind, 2.0 ** rng.integers(-30, 31))
        for _ in range(8):
            t = int(rng.integers(1, 12))
            obj = (rng.normal(size=(1, 1, 3)) * 2 + rng.normal(size=(t, 3, 3)) * rng.choice([1e-3, 0.1, 1.0])).astype(F)
            lo, hi = obj.reshape(-1, 3).min(0), obj.reshape(-1, 3).max(0)
            world = IP.map_corners(M, obj).reshape(t, 3, 3)
            ilo, ihi = IP.image_box(M, lo, hi)
            flat = world.reshape(-1, 3)
            assert (flat >= ilo).all() and (flat <= ihi).all(), (kind, m, M, lo, hi)
            centre, size = flat.mean(0).astype(np.float64), float(np.abs(flat - flat.mean(0)).max()) + float(np.abs(M[:, 3]).max()) * 1e-3
            p = (centre + rng.normal(size=(16, 3)) * size * rng.choice([0.3, 1.0, 10.0], (16, 1))).astype(F)
            p[0] = flat[rng.integers(len(flat))]
            p[1] = np.where(rng.random(3) < 0.5, ilo, ihi)
            lb = bound(p, ilo, ihi)
            d2 = pair_dist2(p, world)[1]
            assert (lb[:, None] <= d2).all(), (kind, m, M)
            pairs += d2.size
    assert pairs > 30000


# 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lobed_positions(pkg):
    world = pkg.World(os.path.join(GOLDEN, "lobed_528.trisrc"))
    try:
        return np.asarray(world.arrays()["vertex_positions"], F).copy()
    finally:
        world.close()


def set_maps(n, seed):
    """n maps around the origin: general rotations with non-uniform scale, then a mirrored one, a sheared one and an exact
    duplicate of map 0 placed after it, as far as n allows"""
    rng = np.random.default_rng(seed)
    maps = np.zeros((n, 3, 4), F)
    for i in range(n):
        A = rotation(rng) @ np.diag(rng.uniform(0.6, 1.6, 3))
        maps[i, :, :3] = A
        maps[i, :, 3] = rng.uniform(-2.5, 2.5, 3) * (n > 1)
    if n >= 2:
        maps[1, :, :3] = (maps[1, :, :3].astype(np.float64) @ np.diag([-1.0, 1.0, 1.0])).astype(F)       # a mirror
    if n >= 5:
        maps[3, :, :3] = (rotation(rng) @ (np.eye(3) + np.triu(rng.normal(size=(3, 3)), 1) * 0.5)).astype(F)   # a shear
        maps[4] = maps[0]                                                                               # an exact duplicate
    return maps


def set_points(positions, maps, n, seed):
    """world points for the set: on the mapped surfaces, near them, far away, with radii +inf, finite (hits and misses), 0,
    negative, NaN, and a few non-finite points"""
    rng = np.random.default_rng(seed)
    tris = positions.reshape(-1, 3, 3)
    i = rng.integers(0, len(maps), n)
    t = rng.integers(0, len(tris), n)
    b = rng.random((n, 2))
    b = np.where(b.sum(1, keepdims=True) > 1, 1 - b, b)
    v = tris[t].astype(np.float64)
    on = v[:, 0] + b[:, :1] * (v[:, 1] - v[:, 0]) + b[:, 1:] * (v[:, 2] - v[:, 0])
    A = np.asarray(maps, np.float64)
    world = np.einsum("nrc,nc->nr", A[i, :, :3], on) + A[i, :, 3]
    extent = float(np.linalg.norm(positions.reshape(-1, 3).max(0) - positions.reshape(-1, 3).min(0)))
    kind = rng.integers(0, 4, n)
    world[kind == 1] += rng.normal(size=((kind == 1).sum(), 3)) * extent / 100
    world[kind == 2] += rng.normal(size=((kind == 2).sum(), 3)) * extent / 3
    world[kind == 3] = rng.normal(size=((kind == 3).sum(), 3)) * extent * 30
    pts = np.zeros(n, R.POINT_DTYPE)
    pts["p"] = world.astype(F)
    md = np.full(n, np.inf, F)
    r = rng.random(n)
    sel = (r >= 0.55) & (r < 0.85)
    md[sel] = (rng.random(sel.sum()) * extent / 8) ** 2
    md[(r >= 0.85) & (r < 0.88)] = 0.0
    md[(r >= 0.88) & (r < 0.91)] = -1.0
    md[(r >= 0.91) & (r < 0.93)] = np.nan
    bad = np.nonzero((r >= 0.93) & (r < 0.96))[0]
    pts["max_dist2"] = md
    pts["p"][bad, rng.integers(0, 3, len(bad))] = rng.choice(np.array([np.nan, np.inf, -np.inf], F), len(bad))
    return pts


@pytest.mark.parametrize("n", [1, 2, 17])
def test_the_restated_walk_returns_the_brute_force_bytes(lobed_positions, n):
    maps = set_maps(n, seed=n)
    pts = set_points(lobed_positions, maps, 160, seed=n + 40)
    want, want_inst = IP.closest_over_instances([lobed_positions], [0] * n, maps, pts)
    order = np.random.default_rng(n).permutation(n)[::-1]       # (not the index order: the tie rule must not lean on it)
    got, got_inst, tests = restated_walk(lobed_positions.reshape(-1, 3, 3), maps, pts, order)
    assert np.array_equal(R.as_bits(got), R.as_bits(want)), np.nonzero((R.as_bits(got) != R.as_bits(want)).any(1))[0][:8]
    assert np.array_equal(got_inst, want_inst)
    hit = want["triangle"] >= 0
    assert 0.25 < hit.mean() < 0.95 and np.array_equal(want_inst >= 0, hit)
    assert tests < 0.6 * len(pts) * n * 528, "the image-box cull skips something"
    if n >= 5:
        assert (want_inst == 0).sum() > 3 and (want_inst == 4).sum() == 0, "the duplicate never wins against its original"
        assert len(set(want_inst[hit].tolist())) > 5


# 3 ---------------------------------------------------------------------------------------------------------------------------
def test_an_identity_map_gives_the_plain_query(lobed_positions):
    pts = set_points(lobed_positions, EYE[None], 300, seed=5)
    got, inst = IP.closest_over_instances([lobed_positions], [0], EYE[None], pts)
    want = R.closest(lobed_positions, pts)
    assert np.array_equal(R.as_bits(got), R.as_bits(want))
    assert np.array_equal(inst, np.where(want["triangle"] >= 0, 0, -1))
    assert np.array_equal(IP.map_corners(EYE, lobed_positions).view(np.uint32).reshape(-1), lobed_positions.view(np.uint32))


def test_a_signed_permutation_keeps_the_zeros_signs():
    v = np.array([[0.0, -0.0, 1.5], [-0.0, 0.0, -2.0], [3.0, -0.0, 0.0], [-0.0, -0.0, -0.0]], F)
    M = np.array([[0, 0, -1, 0], [1, 0, 0, 0], [0, -1, 0, 0]], F)
    w = IP.map_corners(M, v)
    want = np.stack([-v[:, 2], v[:, 0], -v[:, 1]], axis=1)
    assert np.array_equal(w.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(np.signbit(w), np.signbit(want))
    assert np.array_equal(IP.map_corners(EYE, v).view(np.uint32), v.view(np.uint32))
    # a row with nothing to add gives +0; a row with the translation alone gives the translation
    Z = np.array([[0, 0, 0, 0], [0, 0, 0, -0.5], [0, 2, 0, 0]], F)
    z = IP.map_corners(Z, v)
    assert not np.signbit(z[:, 0]).any() and (z[:, 0] == 0).all() and (z[:, 1] == F(-0.5)).all()
    lo, hi = IP.image_box(M, v.min(0), v.max(0))
    assert (w >= lo).all() and (w <= hi).all()


@pytest.mark.parametrize("k", [-20, 20])
def test_scaling_by_a_power_of_two_scales_the_answer_exactly(lobed_positions, k):
    maps = set_maps(5, seed=9)
    pts = set_points(lobed_positions, maps, 200, seed=10)
    want, want_inst = IP.closest_over_instances([lobed_positions], [0] * 5, maps, pts)
    s = F(2.0) ** F(k)
    scaled = pts.copy()
    scaled["p"] = pts["p"] * s
    scaled["max_dist2"] = pts["max_dist2"] * s * s
    got, got_inst = IP.closest_over_instances([lobed_positions], [0] * 5, maps * s, scaled)
    assert np.array_equal(got_inst, want_inst)
    hit = want["triangle"] >= 0
    assert hit.sum() > 60
    for f in ("u", "v", "triangle", "region"):
        assert np.array_equal(got[f].view(np.uint32), want[f].view(np.uint32)), f
    with np.errstate(invalid="ignore"):
        assert np.array_equal((want["q"] * s).view(np.uint32), got["q"].view(np.uint32))
        assert np.array_equal((want["dist2"] * s * s).view(np.uint32), got["dist2"].view(np.uint32))


# 4 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["leaf_root", "one_branch", "wide_by_one"])
def test_the_walk_with_counters_answers_like_the_brute_force(name):
    """instance_point_ref.walk_counters over a hand-shaped tree and refit_ref.node_boxes: its own answer is the restatement's
    triangle under every kind of map, a point that is not walked counts nothing, a walked one counts the root, two bounds a
    branch entered and every triangle of a leaf entered; where every dist2 is 0 nothing is culled."""
    import instance_point_cases as IC
    import refit_ref
    import tree_shapes as T
    tree, vertex_data = T.build(name)
    corners = np.ascontiguousarray(vertex_data[tree.triangle_vertices][:, :, :3])
    positions = corners.reshape(-1)
    boxes = refit_ref.node_boxes(tree, corners)
    rng = np.random.default_rng(len(name))
    leaves = tree.negative < 0
    for kind in ("identity", "rotation_nonuniform", "mirror", "shear", "signed_permutation"):
        M = IC.map_of(kind, rng, positions, 1.5).astype(F)
        pts, _, _ = IC.world_points([positions], [0], M[None], 160, seed=3)
        want, _ = IP.closest_over_instances([positions], [0], M[None], pts)
        w = IP.walk_counters(tree, boxes, corners, M, pts)
        assert np.array_equal(w["triangle"], want["triangle"]), (name, kind)
        go = np.isfinite(pts["p"]).all(1) & (pts["max_dist2"] >= 0)
        assert np.array_equal(w["traversals"], go.astype(np.int64)) and (w["node_visits"][~go] == 0).all()
        assert (w["node_visits"][go] % 2 == 1).all() and (w["node_visits"] <= tree.node_count).all()
        assert (w["leaf_visits"] <= leaves.sum()).all() and (w["triangle_tests"] <= len(corners)).all()
        assert (w["triangle_tests"][want["triangle"] >= 0] >= 1).all()
        if tree.node_count > 3:
            assert w["triangle_tests"][go].mean() < 0.5 * len(corners), "the image-box cull skips something"
        tied = pts.copy()
        tied["p"] = pts["p"] * F(2.0 ** -100)
        tied["max_dist2"] = np.where(pts["max_dist2"] > 0, F(np.inf), pts["max_dist2"])
        z = IP.walk_counters(tree, boxes, corners, M * F(2.0 ** -100), tied)
        assert (z["triangle"][go] == 0).all() and (z["triangle_tests"][go] == len(corners)).all()
        assert (z["node_visits"][go] == tree.node_count).all() and (z["leaf_visits"][go] == leaves.sum()).all()
