"""The sets and points of the instanced closest-point tests (tests/test_gpu_instance_point.py), made without a device so that
what they cover can be checked on the restatement alone: maps of every kind the header's formula treats differently, and
world points of every kind mixed in one wave."""
from __future__ import annotations

import numpy as np

import point_query_ref as R

F = np.float32
EYE = np.eye(3, 4, dtype=F)
KINDS = ("on_surface", "near", "far", "box_corner", "duplicate")

TINY = {
    "one triangle": [[[0.25, 0.5, 1.0], [2.0, 0.75, 1.5], [1.0, 3.0, -0.5]]],
    "11-triangle leaf": [[[-5, -5, -float(k)], [5, -5, -float(k)], [0, 5, -float(k)]] for k in range(10)] +
                        [[[-5, -5, 1.0], [5, -5, 1.0], [0, 5, 1.0]]],
}


def rotation(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def extent_of(positions):
    v = np.asarray(positions, np.float64).reshape(-1, 3)
    return v.min(0), v.max(0)


MAP_KINDS = ("identity", "translation", "rotation_uniform", "rotation_nonuniform", "shear", "mirror", "signed_permutation", "flip")


def map_of(kind, rng, positions, spread):
    """a [3, 4] float64 map of `kind` that brings the scene to a world size near 1 (the rigid kinds keep its size) and places it
    within `spread` of the origin"""
    lo, hi = extent_of(positions)
    size = float((hi - lo).max())
    b = rng.uniform(-spread, spread, 3)
    if kind == "identity":
        return np.eye(3, 4)
    if kind == "translation":
        return np.concatenate([np.eye(3), (b * size)[:, None]], axis=1)
    if kind == "signed_permutation":
        A = np.zeros((3, 3))
        A[np.arange(3), rng.permutation(3)] = rng.choice([-1.0, 1.0], 3)
        return np.concatenate([A, np.zeros((3, 1))], axis=1)          # translation-free: every coordinate keeps its bits
    if kind == "flip":
        return np.concatenate([np.diag(rng.choice([-1.0, 1.0], 3)), (np.round(b * size * 4) / 4)[:, None]], axis=1)
    if kind == "rotation_uniform":
        A = rotation(rng) * rng.uniform(0.6, 1.6) / size
    elif kind == "rotation_nonuniform":
        A = rotation(rng) @ np.diag(rng.uniform(0.5, 1.8, 3)) / size
    elif kind == "shear":
        A = rotation(rng) @ (np.eye(3) + np.triu(rng.normal(size=(3, 3)), 1) * 0.6) / size
    elif kind == "mirror":
        A = rotation(rng) @ np.diag([-1.0, 1.0, 1.0]) @ np.diag(rng.uniform(0.6, 1.5, 3)) / size
        assert np.linalg.det(A) < 0
    else:
        raise KeyError(kind)
    return np.concatenate([A, (b - A @ ((lo + hi) / 2))[:, None]], axis=1)


def make_set(scene_positions, scene_of_instance, seed, spread=1.5, kinds=None):
    """maps [n, 3, 4] float32 for the instances: the kinds in turn (or `kinds`), and from five instances on instance 4 an exact
    duplicate of instance 1 (the same scene, the same floats), placed after its original"""
    rng = np.random.default_rng(seed)
    n = len(scene_of_instance)
    scene_of_instance = list(scene_of_instance)
    kinds = list(kinds) if kinds is not None else [MAP_KINDS[i % len(MAP_KINDS)] for i in range(n)]
    maps = np.stack([map_of(kinds[i], rng, scene_positions[scene_of_instance[i]], spread) for i in range(n)]).astype(F)
    if n >= 5:
        scene_of_instance[4], maps[4], kinds[4] = scene_of_instance[1], maps[1], "duplicate of 1"
    return scene_of_instance, maps, kinds


def world_points(scene_positions, scene_of_instance, maps, n, seed):
    """(POINT_DTYPE points, kind per point, radius class per point): points on the mapped surfaces (half of them exactly at a
    mapped corner), near them, far away, at the corners of an instance's world box or of the whole set's, and duplicates of
    others; radii +inf, finite (sized so that both hits and misses occur), 0, negative and NaN; some points made non-finite.
    The kinds are drawn per point, so every wave mixes them."""
    import instance_point_ref as IP
    rng = np.random.default_rng(seed)
    world = [IP.map_corners(maps[i], scene_positions[s]).reshape(-1, 3, 3) for i, s in enumerate(scene_of_instance)]
    boxes = np.array([[w.reshape(-1, 3).min(0), w.reshape(-1, 3).max(0)] for w in world], np.float64)
    sizes = np.linalg.norm(boxes[:, 1] - boxes[:, 0], axis=1)
    whole = np.array([boxes[:, 0].min(0), boxes[:, 1].max(0)])
    kind = rng.choice(len(KINDS), n, p=[0.3, 0.3, 0.15, 0.15, 0.1])
    p = np.zeros((n, 3), F)
    for j in range(n):
        i = int(rng.integers(len(world)))
        tri = world[i][rng.integers(len(world[i]))].astype(np.float64)
        b = rng.random(2)
        b = 1 - b if b.sum() > 1 else b
        on = tri[0] + b[0] * (tri[1] - tri[0]) + b[1] * (tri[2] - tri[0])
        if kind[j] == 0:
            p[j] = tri[rng.integers(3)] if rng.random() < 0.5 else on
        elif kind[j] == 1:
            p[j] = on + rng.normal(size=3) * sizes[i] / 60
        elif kind[j] == 2:
            p[j] = whole.mean(0) + rng.normal(size=3) * np.linalg.norm(whole[1] - whole[0]) * 40
        elif kind[j] == 3:
            box = whole if rng.random() < 0.3 else boxes[i]
            p[j] = np.where(rng.random(3) < 0.5, box[0], box[1]).astype(F)
    dup = np.nonzero(kind == 4)[0]
    p[dup] = p[rng.integers(0, n, len(dup))]
    typical = float(np.median(sizes))
    md = np.full(n, np.inf, F)
    r = rng.random(n)
    radius = np.zeros(n, np.int8)                       # 0: +inf, 1: finite, 2: zero, 3: negative, 4: NaN, 5: a non-finite point
    sel = (r >= 0.4) & (r < 0.7)
    md[sel] = (rng.random(sel.sum()) ** 2 * typical / 4) ** 2
    radius[sel] = 1
    md[(r >= 0.7) & (r < 0.74)] = 0.0
    radius[(r >= 0.7) & (r < 0.74)] = 2
    md[(r >= 0.74) & (r < 0.82)] = rng.choice(np.array([-1.0, -0.0, -np.inf, -1e-30], F), ((r >= 0.74) & (r < 0.82)).sum())
    radius[(r >= 0.74) & (r < 0.82)] = 3
    md[(r >= 0.82) & (r < 0.86)] = np.nan
    radius[(r >= 0.82) & (r < 0.86)] = 4
    bad = np.nonzero((r >= 0.86) & (r < 0.94))[0]
    p[bad, rng.integers(0, 3, len(bad))] = rng.choice(np.array([np.nan, np.inf, -np.inf], F), len(bad))
    radius[bad] = 5
    out = np.zeros(n, R.POINT_DTYPE)
    out["p"], out["max_dist2"] = p, md
    return out, kind, radius


def assert_mixed(points, kind, radius, records, what):
    """over 5 % of each kind of point and of each outcome, on the restatement's records"""
    n = len(points)
    hit = records["triangle"] >= 0
    ok = radius != 5
    shares = {k: float(((kind == j) & ok).mean()) for j, k in enumerate(KINDS)}
    shares["non_finite_point"] = float((radius == 5).mean())
    shares["negative_radius"] = float((radius == 3).mean())
    shares["finite_radius_hit"] = float(((radius == 1) & hit).mean())
    shares["finite_radius_miss"] = float(((radius == 1) & ~hit).mean())
    shares["unlimited_hit"] = float(((radius == 0) & hit).mean())
    shares["exactly_on_surface"] = float((hit & (records["dist2"] == 0)).mean())
    low = {k: v for k, v in shares.items() if v <= 0.05}
    assert not low, f"{what}: under 5 % of {n} points: {low} (all: {shares})"
    # -0.0 as a radius is not negative: 0 >= -0 holds, the point walks (and hits only a surface it lies on)
    assert not hit[(radius == 3) & (points["max_dist2"] != 0)].any() and not hit[radius == 4].any() and not hit[radius == 5].any()
