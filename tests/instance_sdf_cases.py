"""The sets and points of the instanced signed distance edge tests, made without a device so that what they cover can be checked
on the restatement alone (tests/instance_sdf_ref.py): the shared case generator of tests/test_instance_sdf_cases_reference.py
(CPU) and tests/test_gpu_instance_sdf_edges.py, tests/test_gpu_instance_sdf_scale.py (GPU).  No test and no GPU in here.

The hollow member.  hollow() is a box with a spike-shaped cavity, 64 triangles, closed; hollow_set() places it nine times (the
eight kinds of instance_point_cases.MAP_KINDS and an exact duplicate of instance 1 at instance 4), and hollow_points() are
HOLLOW_POINTS points of feature_points(): a third displaced from corners, a third from edge points, a third from face points of
the world meshes, by at most 0.04, 0.1 and 0.3 world sizes.  Inside a convex member the nearest feature is always a face, and
for a face-region point no other slot of its triangle changes the sign, so a kernel that read the wrong pseudonormal slot
passes on convex members; the cavity's reflex edges and corners are what makes the slot matter.
MEASURED on the restatement (instance_sdf_ref.signed_parts, W by instance_ref.world_to_object; the CPU test asserts each
figure's consequence), 4,096 points, every one a hit, the duplicate never the nearest:
  slot                         face      a      b      c     AB     AC     BC
  negative values             1,716     94     18     25    146    234    220
  positive values             1,356     12     17     11    128     45     74
  slot-decided points             1     91     24     27    185    145    170      (some other slot of the point's own object
                                                                                      triangle gives the other sign)
  values changed by each of instance_sdf_ref.WRONG_VARIANTS: the face normal for every region 80, vertex a for every vertex
  37, AC and BC swapped 89, the edge slots shifted by one 109, the world record's (triangle, region) 16, b and c swapped 23.
  6.9 % of the points lie within 1e-3 world sizes of the surface; on every other point the sign agrees with the float64
  winding number of the nearest instance's world mesh.

The peel shapes.  peel_set() is PEEL_INSTANCES = 72 one-leaf members (tetrahedron, cube, and both wound inward, so that members
differ by scene as well as by instance) on a grid; peel_points() are 357 points whose aligned waves are, on the restatement:
64 distinct instances in descending order, 64 distinct instances in a seeded permutation, the only hit at lane 63, the only hit
at lane 0, all misses, and a last wave of 37 lanes (82 negative, 75 positive, 200 misses).

More than 256 scene slots.  many_scene_set() is MANY_SCENES = 260 distinct one-leaf tetrahedra, one instance each in slot
order, slot j wound inward when (j + (j >> 8)) & 1, with one point inside and one outside each: a sign-data pointer taken from
slot j - 256 or from a neighbouring slot flips both signs (the pair 255, 256 agrees with each other: the parity restarts there).

The scale cells.  scale_cells() is instance_point_scale_cases.CELLS and SIGN_KEEPING_CELLS.  NEGATIVE_SHARE holds the share
of the hits that are negative per cell, MEASURED on the restatement; NO_SIGN lists the cells where none is and why.
"""
from __future__ import annotations

import numpy as np

import instance_point_cases as IC
import instance_point_ref as IP
import instance_ref as IR
import instance_sdf_ref as IS
import point_query_ref as R
import sdf_ref as S

F = np.float32
SLOTS = ("face", "a", "b", "c", "AB", "AC", "BC")
VARIANTS = IS.WRONG_VARIANTS


# the hollow member -----------------------------------------------------------------------------------------------------------
def hollow():
    """(positions float32 [V, 3], triangles int32 [64, 3]) of a box with a spike-shaped cavity: sdf_ref.cube() scaled to
    [-2, 2] x [-2, 2] x [-1.5, 7.5], and sdf_ref.fan_spike() inside it with every triangle's winding reversed, so that the
    spike is empty space.  Closed.  Every edge and corner of the spike is a reflex feature of the solid: the nearest feature
    of an inside point is there a vertex or an edge, which no convex member offers.  Triangle t's corner order is rotated
    cyclically by t % 3, which keeps the winding and spreads the roles a, b and c (fan_spike's apex is always c)."""
    box_pos, box_tri = S.cube()
    box_pos = (box_pos * np.array([4, 4, 9], F) + np.array([-2, -2, -1.5], F)).astype(F)
    spike_pos, spike_tri = S.fan_spike()
    pos = np.concatenate([box_pos, spike_pos]).astype(F)
    tri = np.concatenate([box_tri, spike_tri[:, ::-1] + len(box_pos)]).astype(np.int32)
    for t in range(len(tri)):
        tri[t] = np.roll(tri[t], -(t % 3))
    return pos, tri


HOLLOW_KINDS = list(IC.MAP_KINDS[:4]) + ["identity"] + list(IC.MAP_KINDS[4:])   # instance 4 becomes the duplicate of instance 1
HOLLOW_SEED, HOLLOW_POINT_SEED, HOLLOW_POINTS, HOLLOW_SPREAD = 61, 63, 4096, 1.2
DISPLACEMENTS = {"corner": 0.04, "edge": 0.1, "face": 0.3}          # the largest, in world sizes of the point's instance


def hollow_set():
    """(positions of the one scene, scene of every instance, maps, kinds): the hollow member under the eight kinds of map and
    an exact duplicate of instance 1 at instance 4"""
    positions = S.corners_of(*hollow())
    of, maps, kinds = IC.make_set([positions], [0] * 9, seed=HOLLOW_SEED, spread=HOLLOW_SPREAD, kinds=HOLLOW_KINDS)
    return positions, of, maps, kinds


def world_meshes(scene_positions, of, maps):
    """(the mapped fp32 corners of every instance, [t, 3, 3] each; the world size of every instance)"""
    world = [IP.map_corners(maps[i], scene_positions[s]).reshape(-1, 3, 3) for i, s in enumerate(of)]
    sizes = np.array([np.linalg.norm(w.reshape(-1, 3).max(0).astype(np.float64) - w.reshape(-1, 3).min(0)) for w in world])
    return world, sizes


def feature_points(scene_positions, of, maps, n, seed):
    """(POINT_DTYPE points with radius +inf, the feature each started from: 0 corner, 1 edge, 2 face).  Point j starts from
    feature j % 3 of a random triangle of a random instance's world mesh (a corner, a point on an edge, a point in the face)
    and is displaced along a random direction by a length uniform in [0, DISPLACEMENTS] world sizes of that instance."""
    rng = np.random.default_rng(seed)
    world, sizes = world_meshes(scene_positions, of, maps)
    limit = [DISPLACEMENTS[k] for k in ("corner", "edge", "face")]
    p = np.zeros((n, 3))
    feature = np.arange(n) % 3
    for j in range(n):
        i = int(rng.integers(len(world)))
        tri = world[i][rng.integers(len(world[i]))].astype(np.float64)
        if feature[j] == 0:
            on = tri[rng.integers(3)]
        elif feature[j] == 1:
            k = int(rng.integers(3))
            s = rng.random()
            on = tri[k] + s * (tri[(k + 1) % 3] - tri[k])
        else:
            b = rng.random(2)
            b = 1 - b if b.sum() > 1 else b
            on = tri[0] + b[0] * (tri[1] - tri[0]) + b[1] * (tri[2] - tri[0])
        u = rng.normal(size=3)
        p[j] = on + rng.uniform(0.0, limit[feature[j]]) * sizes[i] * u / np.linalg.norm(u)
    pts = np.zeros(n, R.POINT_DTYPE)
    pts["p"], pts["max_dist2"] = p.astype(F), np.inf
    return pts, feature


def hollow_points():
    positions, of, maps, _ = hollow_set()
    return feature_points([positions], of, maps, HOLLOW_POINTS, HOLLOW_POINT_SEED)


# what the restatement says of a set of points --------------------------------------------------------------------------------
def slot_figures(parts):
    """Per pseudonormal slot of the object record, on the intermediate results (instance_sdf_ref.signed_parts): the numbers of
    negative and of positive values, and of slot-decided points: those for which some other slot of the point's own object
    triangle gives the other sign.  {"negative": [7], "positive": [7], "decided": [7]}"""
    triangle, slot = IS.object_slots(parts)
    value = IS.values_of(parts)
    hit = triangle >= 0
    other = np.zeros(len(value), bool)
    for k in range(7):
        with np.errstate(invalid="ignore"):
            other |= (IS.values_of(parts, lambda q, k=k: (triangle, np.full(len(triangle), k))) < 0) != (value < 0)
    out = {"negative": [], "positive": [], "decided": []}
    for k in range(7):
        mine = hit & (slot == k)
        with np.errstate(invalid="ignore"):
            out["negative"].append(int((mine & (value < 0)).sum()))
            out["positive"].append(int((mine & (value > 0)).sum()))
        out["decided"].append(int((mine & other).sum()))
    return out


def changed_by(parts):
    """{variant: the number of values it changes}"""
    base = IS.values_of(parts).view(np.uint32)
    return {name: int((IS.values_of(parts, pick).view(np.uint32) != base).sum()) for name, pick in VARIANTS.items()}


def reproduced_by(parts, got):
    """the names of the variants whose values are `got`'s, bit for bit (for a failure message)"""
    g = np.ascontiguousarray(got, F).view(np.uint32)
    return [name for name, pick in VARIANTS.items() if np.array_equal(IS.values_of(parts, pick).view(np.uint32), g)]


def winding_agreement(scene_positions, of, maps, points, values, instances):
    """(kept: at least 1e-3 world sizes from the surface, inside: |float64 winding number| of the nearest instance's world mesh
    above 0.5), per point; every point must be a hit"""
    world, sizes = world_meshes(scene_positions, of, maps)
    assert (instances >= 0).all()
    keep = np.abs(values) >= 1e-3 * sizes[instances]
    inside = np.zeros(len(points), bool)
    for i in sorted(set(instances.tolist())):
        at = np.nonzero(instances == i)[0]
        inside[at] = np.abs(S.winding_number(world[i].reshape(-1), points["p"][at])) > 0.5
    return keep, inside


# the peel shapes -------------------------------------------------------------------------------------------------------------
PEEL_INSTANCES, PEEL_PITCH, PEEL_SEED = 72, 4.0, 71
PEEL_SCENES = ("tetrahedron", "cube", "tetrahedron wound inward", "cube wound inward")
PEEL_WAVES = ("descending", "permutation", "only lane 63", "only lane 0", "all misses", "partial")
PEEL_PARTIAL = 37


def inward(positions):
    """the same triangles, each wound the other way (corners a, c, b): closed, with every pseudonormal pointing inward"""
    return np.ascontiguousarray(np.asarray(positions, F).reshape(-1, 3, 3)[:, [0, 2, 1]]).reshape(-1)


def peel_scenes():
    """the four member scenes' positions, one leaf each (4 or 12 triangles)"""
    tet, cube = S.corners_of(*S.tetrahedron()), S.corners_of(*S.cube())
    return [tet, cube, inward(tet), inward(cube)]


def placed(kind, rng, positions, centre):
    """a float32 map of `kind` (instance_point_cases.map_of) whose translation puts the image of the scene's box centre at
    `centre`"""
    lo, hi = IC.extent_of(positions)
    M = IC.map_of(kind, rng, positions, 0.0)
    M[:, 3] = np.asarray(centre, np.float64) - M[:, :3] @ ((lo + hi) / 2)
    return M.astype(F)


INSIDE_AT, OUTSIDE_AT = np.array([0.2, 0.25, 0.15]), np.array([-0.25, 0.3, 0.2])   # object points of tetrahedron and cube alike


def peel_set():
    """(scene positions, scene of every instance, maps): PEEL_INSTANCES instances on a 9 x 8 grid of pitch PEEL_PITCH, instance
    i over scene i % 4 under map kind i % 8 (a member's world size is below 3.2, so each instance keeps to its own cell)"""
    rng = np.random.default_rng(PEEL_SEED)
    scenes = peel_scenes()
    of = [i % len(scenes) for i in range(PEEL_INSTANCES)]
    maps = np.stack([placed(IC.MAP_KINDS[i % 8], rng, scenes[of[i]], (PEEL_PITCH * (i % 9), PEEL_PITCH * (i // 9), 0.0))
                     for i in range(PEEL_INSTANCES)])
    return scenes, of, maps


def peel_points():
    """(POINT_DTYPE points, the instance each point is meant to hit or -1): the waves of PEEL_WAVES in turn, 64 points each but
    the last (PEEL_PARTIAL).  A hit's point is the image of INSIDE_AT (even index) or OUTSIDE_AT (odd) under its instance's
    map, with radius +inf; a miss is one of: a far point with radius 0, a negative radius, a NaN radius, a non-finite point."""
    rng = np.random.default_rng(PEEL_SEED + 1)
    _, of, maps = peel_set()
    n = PEEL_INSTANCES
    wanted = np.full(64 * (len(PEEL_WAVES) - 1) + PEEL_PARTIAL, -1, np.int64)
    wanted[0:64] = np.arange(n - 1, n - 65, -1)
    wanted[64:128] = rng.permutation(n)[:64]
    wanted[128 + 63] = 5
    wanted[192] = 66
    part = rng.integers(0, n, PEEL_PARTIAL)
    part[rng.random(PEEL_PARTIAL) < 0.3] = -1
    wanted[320:] = part
    pts = np.zeros(len(wanted), R.POINT_DTYPE)
    for j, i in enumerate(wanted.tolist()):
        if i >= 0:
            M = maps[i].astype(np.float64)
            pts["p"][j] = M[:, :3] @ (INSIDE_AT if j % 2 == 0 else OUTSIDE_AT) + M[:, 3]
            pts["max_dist2"][j] = np.inf
        else:
            kind = j % 4
            pts["p"][j] = (1e6, -2e6, 3e6) if kind == 0 else maps[j % n][:, 3]
            pts["max_dist2"][j] = (0.0, -1.0, np.nan, np.inf)[kind]
            if kind == 3:
                pts["p"][j][j % 3] = np.inf
    return pts, wanted


def assert_peel_shapes(instances, wanted):
    """the restatement's instances are the ones meant, and the waves have the shapes PEEL_WAVES names"""
    assert np.array_equal(instances, wanted), np.nonzero(instances != wanted)[0][:8]
    assert len(instances) % 64 != 0
    wave = [instances[64 * w:64 * w + 64] for w in range(len(PEEL_WAVES))]
    assert len(set(wave[0].tolist())) == 64 and (np.diff(wave[0]) < 0).all() and wave[0].min() >= 0
    assert len(set(wave[1].tolist())) == 64 and wave[1].min() >= 0 and not (np.diff(wave[1]) < 0).all() and not (np.diff(wave[1]) > 0).all()
    assert (wave[2][:63] == -1).all() and wave[2][63] >= 0
    assert wave[3][0] >= 0 and (wave[3][1:] == -1).all()
    assert (wave[4] == -1).all()
    assert len(wave[5]) == PEEL_PARTIAL and (wave[5] >= 0).sum() >= 8 and (wave[5] < 0).sum() >= 4


# more than 256 scene slots ---------------------------------------------------------------------------------------------------
MANY_SCENES, MANY_PITCH = 260, 4.0


def wound_inward(j):
    """slot j's tetrahedron is wound inward: j and j + 256 disagree, and so do j and j + 1 except the pair (255, 256), where the
    second launch's parity starts"""
    return bool((j + (j >> 8)) & 1)


def many_scene_positions():
    """MANY_SCENES one-leaf tetrahedra, sdf_ref.tetrahedron() times 1 + (j % 7) / 8, wound inward where wound_inward(j)"""
    tet = S.corners_of(*S.tetrahedron())
    out = []
    for j in range(MANY_SCENES):
        p = (tet * F(1 + (j % 7) / 8)).astype(F)
        out.append(inward(p) if wound_inward(j) else p)
    return out


def many_scene_set():
    """(scene positions, scene of every instance, maps, points): instance j is scene j (so scene slot j) under a translation to
    a 20 x 13 grid; point 2 j is inside tetrahedron j and point 2 j + 1 outside it, radius +inf"""
    scenes = many_scene_positions()
    of = list(range(MANY_SCENES))
    maps = np.repeat(IC.EYE[None], MANY_SCENES, axis=0).copy()
    maps[:, 0, 3] = MANY_PITCH * (np.arange(MANY_SCENES) % 20)
    maps[:, 1, 3] = MANY_PITCH * (np.arange(MANY_SCENES) // 20)
    pts = np.zeros(2 * MANY_SCENES, R.POINT_DTYPE)
    pts["max_dist2"] = np.inf
    for j in range(MANY_SCENES):
        scale = 1 + (j % 7) / 8
        pts["p"][2 * j] = maps[j, :, 3] + (INSIDE_AT * scale).astype(F)
        pts["p"][2 * j + 1] = maps[j, :, 3] + (OUTSIDE_AT * scale).astype(F)
    return scenes, of, maps, pts


def assert_many_scene_shapes(values, instances):
    """on the restatement: point 2 j and 2 j + 1 hit instance j, the inside point is negative exactly when tetrahedron j is
    wound outward and the outside point exactly when it is wound inward, so that a sign-data pointer taken from slot j - 256
    or from a neighbouring slot (but for the pair 255, 256) flips both; both signs occur among slots 0 to 255 and among slots
    256 to 259"""
    assert MANY_SCENES > 256
    assert np.array_equal(instances, np.repeat(np.arange(MANY_SCENES), 2))
    inw = np.array([wound_inward(j) for j in range(MANY_SCENES)])
    assert np.array_equal(values[0::2] < 0, ~inw) and np.array_equal(values[1::2] < 0, inw) and (values != 0).all()
    for lo, hi in ((0, 256), (256, MANY_SCENES)):
        assert inw[lo:hi].any() and (~inw[lo:hi]).any()
    for j in range(MANY_SCENES):
        for other in (j - 1, j + 1, j - 256):
            assert not 0 <= other < MANY_SCENES or inw[other] != inw[j] or {j, other} == {255, 256}, (j, other)


# the scale cells -------------------------------------------------------------------------------------------------------------
# instance_point_scale_cases.CELLS, and the cells below, where a member's scale is moderate and the sign survives
SIGN_KEEPING_CELLS = [("cancel", a) for a in (-30, -20, 20, 30)] + [("scene", k) for k in (-20, 20, 30)]


def scale_cells():
    import instance_point_scale_cases as SC
    return list(SC.CELLS) + SIGN_KEEPING_CELLS


_cell_memo = {}


def cell_parts(pkg, key):
    """instance_sdf_ref.signed_parts of a cell on the CPU (W by instance_ref.world_to_object), once per process"""
    import instance_point_scale_cases as SC
    if key not in _cell_memo:
        c = SC.cell(pkg, key)
        with np.errstate(all="ignore"):
            _cell_memo[key] = IS.signed_parts(c.positions(pkg), c.of, c.maps, IR.world_to_object(c.maps), c.points, closest=SC.restated(pkg, c))
    return _cell_memo[key]


def negative_share(parts):
    """the share of the hits whose value is negative"""
    hit = parts["instances"] >= 0
    with np.errstate(invalid="ignore"):
        return float((IS.values_of(parts)[hit] < 0).mean())


# MEASURED on the restatement, in per cent of the cell's hits (tests/test_instance_sdf_cases_reference.py asserts each to 0.05):
NEGATIVE_SHARE = {
    ("world", -70): 7.7, ("world", -64): 24.2, ("world", -40): 24.5, ("world", -31): 24.1, ("world", -20): 20.7, ("world", 0): 20.7,
    ("world", 20): 20.7, ("world", 32): 20.7, ("world", 33): 20.7, ("world", 40): 24.8, ("world", 63): 24.8, ("world", 64): 24.8,
    ("far", 12): 21.5, ("far", 20): 6.2, ("far", 23): 5.2, ("ill", 6): 15.4, ("ill", 12): 24.6, ("ill", 20): 25.5,
    ("negzero", 0): 23.1, ("negzero", 1): 23.1,
    ("cancel", -30): 21.4, ("cancel", -20): 20.7, ("cancel", 20): 20.7, ("cancel", 30): 20.7,
    ("scene", -20): 20.7, ("scene", 20): 20.7, ("scene", 30): 20.7,
}
MIN_NEGATIVE_SHARE = 0.03
# Cells where no value is negative, and why.  "no sign vector": at a member scale of 2^+-40 or beyond, the face normal's
# length sqrtf(dot(n, n)) is +inf or 0, the header then stores a zero normal, and all 7 x T pseudonormals of both scenes are
# zero vectors: sigma is +-0 and never below 0.  "every dist2 is 0": the world dist2 is 0 on every hit, and a point on the
# surface is never inside.  (("subnormal", -70) has both reasons.)
NO_SIGN = {
    ("scene", -64): "no sign vector", ("scene", -40): "no sign vector", ("scene", 40): "no sign vector", ("scene", 64): "no sign vector",
    ("cancel", -64): "no sign vector", ("cancel", -40): "no sign vector", ("cancel", 40): "no sign vector", ("cancel", 64): "no sign vector",
    ("ties", -90): "every dist2 is 0", ("subnormal", -70): "every dist2 is 0",
}


def usable_sign_vectors(parts):
    """the number of finite nonzero pseudonormals in the cell's sign data"""
    return sum(int((np.isfinite(x).all(-1) & (x != 0).any(-1)).sum()) for x in parts["sign_data"])
