"""The restatement of the instanced signed distance query (tests/instance_sdf_ref.py, include/shader_ray_instance_sdf.h) pinned
on the CPU: one identity instance is sdf_ref's answer byte for byte; on closed meshes under maps of every kind the sign is
negative exactly where the float64 winding number of the nearest instance's world mesh says inside; and on a steep spike under
a non-uniform scale and under a shear, where carrying the object pseudonormal to the world like a normal signs points wrong,
which is why the sign is taken in object space."""
import numpy as np
import pytest

import instance_point_cases as IC
import instance_point_ref as IP
import instance_ref as IR
import instance_sdf_ref as IS
import point_query_ref as R
import sdf_ref as S

F = np.float32
EYE = IC.EYE


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def mesh_positions(pkg, name):
    if name == "lobed 8x16":
        pos, tri = pkg.scenes.lobed_sphere_mesh(8, 16, ears=False)
        return S.corners_of(pos.astype(F), tri)
    return S.corners_of(*getattr(S, name)())


# 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cube", "fan_spike"])
def test_one_identity_instance_is_the_signed_distance_restatement(name):
    positions = mesh_positions(None, name)
    pts, kind, radius = IC.world_points([positions], [0], EYE[None], 600, seed=11)
    got, rec, inst = IS.signed_over_instances([positions], [0], EYE[None], EYE[None], pts)
    want_rec = R.closest(positions, pts)
    want = S.signed(pts, want_rec, S.derive(positions)["sign_data"])
    assert np.array_equal(R.as_bits(rec), R.as_bits(want_rec)) and np.array_equal(inst, np.where(want_rec["triangle"] >= 0, 0, -1))
    assert np.array_equal(bits(got), bits(want))
    hit = want_rec["triangle"] >= 0
    assert (got[hit] < 0).sum() > 20 and (got[hit] > 0).sum() > 20 and np.isnan(got[~hit]).all() and (~hit).sum() > 20


# 2 ---------------------------------------------------------------------------------------------------------------------------
def displaced_points(world, sizes, n, rng):
    """n surface points of the world meshes (a list of [t, 3, 3]), each displaced by o * size * (a random unit vector) with o
    uniform in [2e-3, 0.3] and size its instance's world size"""
    p = np.zeros((n, 3))
    for j in range(n):
        i = int(rng.integers(len(world)))
        tri = world[i][rng.integers(len(world[i]))].astype(np.float64)
        b = rng.random(2)
        b = 1 - b if b.sum() > 1 else b
        on = tri[0] + b[0] * (tri[1] - tri[0]) + b[1] * (tri[2] - tri[0])
        u = rng.normal(size=3)
        p[j] = on + rng.uniform(2e-3, 0.3) * sizes[i] * u / np.linalg.norm(u)
    return p.astype(F)


def world_meshes(positions_of, of, maps):
    world = [IP.map_corners(maps[i], positions_of[s]).reshape(-1, 3, 3) for i, s in enumerate(of)]
    sizes = np.array([np.linalg.norm(w.reshape(-1, 3).max(0).astype(np.float64) - w.reshape(-1, 3).min(0)) for w in world])
    return world, sizes


def assert_sign_is_the_winding_number(positions_of, of, maps, p, what, values=None):
    """for the points kept (at least 1e-3 world sizes from the nearest instance's surface; at most 10 % may be left out): the
    value is negative exactly when |winding number| of the nearest instance's world mesh is above 0.5.  Returns (kept,
    inside, instances)."""
    world, sizes = world_meshes(positions_of, of, maps)
    pts = np.zeros(len(p), R.POINT_DTYPE)
    pts["p"], pts["max_dist2"] = p, np.inf
    got, rec, inst = IS.signed_over_instances(positions_of, of, maps, IR.world_to_object(maps), pts)
    if values is not None:
        got = values(pts)
    hit = inst >= 0
    assert hit.all()
    keep = np.abs(got) >= 1e-3 * sizes[inst]
    left_out = 1.0 - keep.mean()
    print(f"{what}: {left_out:.3%} of {len(p)} points left out")
    assert left_out <= 0.10, (what, left_out)
    inside = np.zeros(len(p), bool)
    for i in sorted(set(inst.tolist())):
        at = np.nonzero(inst == i)[0]
        inside[at] = np.abs(S.winding_number(world[i].reshape(-1), p[at])) > 0.5
    return keep, inside, inst, got


@pytest.mark.parametrize("name", ["cube", "tetrahedron", "lobed 8x16"])
def test_the_sign_agrees_with_the_winding_number_under_every_kind_of_map(pkg, name):
    positions = mesh_positions(pkg, name)
    assert S.derive(positions)["info"]["closed"] == 1
    rng = np.random.default_rng(len(name))
    maps = np.stack([IC.map_of(kind, rng, positions, 1.2) for kind in IC.MAP_KINDS]).astype(F)
    of = [0] * len(maps)
    world, sizes = world_meshes([positions], of, maps)
    p = displaced_points(world, sizes, 1600, rng)
    keep, inside, inst, got = assert_sign_is_the_winding_number([positions], of, maps, p, name)
    assert set(inst.tolist()) == set(range(len(maps))), "every kind of map is some point's nearest instance"
    for i in range(len(maps)):
        mine = keep & (inst == i)
        assert inside[mine].sum() > 5 and (~inside[mine]).sum() > 5, (IC.MAP_KINDS[i], inside[mine].sum(), (~inside[mine]).sum())
    bad = np.nonzero(keep & ((got < 0) != inside))[0]
    assert len(bad) == 0, (name, [(IC.MAP_KINDS[inst[j]], p[j], got[j]) for j in bad[:5]])


# 3 ---------------------------------------------------------------------------------------------------------------------------
SPIKE_MAPS = {
    "diag(8, 1, 1)": np.array([[8, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], F),
    "shear": np.array([[1, 0, 0.75, 0.5], [0, 1, 0.25, -1], [0, 0, 1, 2]], F),
}


@pytest.mark.parametrize("which", sorted(SPIKE_MAPS))
def test_a_spike_under_a_non_conformal_map_needs_the_object_space_sign(which):
    """fan_spike placed by a non-uniform scale and by a shear.  Points above the apex are outside, points just under it are
    inside, and points displaced from the whole surface agree with the winding number.  The variant that takes the sign in world
    space, from the member's pseudonormal carried over like a normal, gets points wrong: a pseudonormal is a sum weighted by
    angles and unit lengths that the map does not keep, and at a sharp feature a wrongly weighted sum leaves the region where
    the test is valid."""
    pos, tri = S.fan_spike()
    positions = S.corners_of(pos, tri)
    M = SPIKE_MAPS[which]
    maps = M[None]
    A, b = M[:, :3].astype(np.float64), M[:, 3].astype(np.float64)
    rng = np.random.default_rng(9)
    apex = pos[4].astype(np.float64)
    above_o = apex + np.stack([(rng.random(200) * 2 - 1) * 0.3, (rng.random(200) * 2 - 1) * 0.3, np.ones(200)], axis=1) * rng.uniform(0.05, 0.5, (200, 1))
    under_o = apex - np.stack([np.zeros(100), np.zeros(100), rng.uniform(0.05, 0.4, 100)], axis=1)
    to_world = lambda x: (x @ A.T + b).astype(F)
    pts = np.zeros(300, R.POINT_DTYPE)
    pts["p"], pts["max_dist2"] = np.concatenate([to_world(above_o), to_world(under_o)]), np.inf
    got, rec, inst = IS.signed_over_instances([positions], [0], maps, IR.world_to_object(maps), pts)
    assert (inst == 0).all() and (got[:200] > 0).all() and (got[200:] < 0).all(), which
    # the whole surface: the restatement agrees with the winding number, the world-normal variant does not
    world, sizes = world_meshes([positions], [0], maps)
    p = displaced_points(world, sizes, 1500, rng)
    keep, inside, _, ours = assert_sign_is_the_winding_number([positions], [0], maps, p, which)
    assert np.array_equal(ours[keep] < 0, inside[keep])
    variant = lambda q: IS.signed_with_world_normals([positions], [0], maps, q)[0]
    vkeep, vinside, _, theirs = assert_sign_is_the_winding_number([positions], [0], maps, p, which + ", world normals", values=variant)
    wrong = vkeep & ((theirs < 0) != vinside)
    print(f"{which}: the world-normal variant signs {int(wrong.sum())} of {int(vkeep.sum())} points wrong")
    assert wrong.sum() >= 1 and np.array_equal(np.abs(theirs), np.abs(ours))
