"""The instanced query's CPU restatement (tests/instance_ref.py): the object-ray rule keeps the signed zeros of a direction
under identity, translation, permutation and flip rows; and on two scene files the composition over instances agrees with
the ray query's restatement on one merged world-space scene written as a trisrc."""
import os
import tempfile

import numpy as np
import pytest

import helpers
import instance_ref as I
import ray_query_ref as R

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def signs(a):
    return np.signbit(np.asarray(a, F))


@pytest.mark.parametrize("W", [
    np.eye(3, 4),                                                   # identity
    np.hstack([np.eye(3), [[2.5], [-1.0], [0.0]]]),                 # translation
    np.array([[0, 1, 0, 0], [0, 0, 1, 0], [1, 0, 0, 0]], float),    # axis permutation
    np.array([[-1, 0, 0, 0], [0, 1, 0, 3], [0, 0, -1, 0]], float),  # flips
])
def test_object_rows_keep_signed_zeros(W):
    d = np.array([[0.0, -0.0, 1.0], [-0.0, 0.0, -1.0], [-0.0, -0.0, 0.5], [1.0, 0.0, -0.0]], F)
    o = np.array([[0.25, -0.0, 0.0]] * 4, F)
    Po, Do = I.object_rays(W, o, d)
    # each row has one nonzero entry: the result is that one product, signed zeros and all
    lin = np.asarray(W, F)[:, :3]
    cols = [int(np.nonzero(lin[r])[0][0]) for r in range(3)]
    want = np.stack([lin[r, cols[r]] * d[:, cols[r]] for r in range(3)], axis=1)
    assert np.array_equal(Do, want) and np.array_equal(signs(Do), signs(want)), (Do, want)
    # the origin: a zero translation adds nothing, so -0 stays -0 through an identity row
    if np.array_equal(W, np.eye(3, 4)):
        assert np.array_equal(signs(Po), signs(o)) and np.array_equal(Po, o)


def test_zero_entries_are_skipped_not_added():
    # a naive dot product 0 * x + 1 * (-0) + 0 * y gives +0; the rule gives -0
    W = np.array([[0, 1, 0, 0], [1, 0, 0, 0], [0, 0, 1, 0]], F)
    _, Do = I.object_rays(W, np.zeros((1, 3), F), np.array([[5.0, -0.0, 2.0]], F))
    assert Do[0, 0] == 0 and np.signbit(Do[0, 0])


def rotation(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def placements(rng, extent):
    """object-to-world maps: a translation, a rotation with a non-uniform scale, a mirror, and a duplicate of the first"""
    out = [np.hstack([np.eye(3), [[0.1 * extent], [0.0], [-0.2 * extent]]])]
    out.append(np.hstack([rotation(rng) @ np.diag([1.5, 0.7, 1.1]), [[1.2 * extent], [0.3 * extent], [0.0]]]))
    out.append(np.hstack([np.diag([-1.0, 1.0, 1.0]) @ rotation(rng), [[-0.9 * extent], [0.0], [0.5 * extent]]]))
    out.append(out[0].copy())
    return np.asarray(out, np.float32)


SCENES = {"small_trisrc": helpers.small_trisrc, "lobed_528": lambda: os.path.join(GOLDEN, "lobed_528.trisrc")}


@pytest.mark.parametrize("name", sorted(SCENES))
def test_composition_equals_the_merged_scene(pkg, name):
    rng = np.random.default_rng(11)
    world = pkg.World(SCENES[name]())
    arrays = R.SceneArrays(world.arrays())
    corners = arrays.positions.reshape(-1, 3).astype(np.float64)
    extent = float(np.ptp(corners, axis=0).max())
    M = placements(rng, extent)
    W = I.world_to_object(M)
    # the merged scene: every instance's triangles mapped to the world in double, rounded to float32
    world_corners = [(corners @ m[:, :3].astype(np.float64).T + m[:, 3].astype(np.float64)).astype(F) for m in M]
    key = {}
    for i, wc in enumerate(world_corners):
        for k, tri in enumerate(wc.reshape(-1, 9)):
            key.setdefault(tri.tobytes(), (i, k))
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "merged.trisrc")
        allc = np.concatenate(world_corners)
        pkg.scenes.write_trisrc(path, allc, np.arange(len(allc)).reshape(-1, 3))
        merged = R.SceneArrays(pkg.World(path).arrays())
    lo, hi = np.concatenate(world_corners).min(0), np.concatenate(world_corners).max(0)
    n = 3000
    o = (lo + (hi - lo) * (rng.random((n, 3)) * 1.6 - 0.3)).astype(F)
    tris = allc.reshape(-1, 3, 3).astype(np.float64)[rng.integers(0, len(allc) // 3, n)]
    b = rng.random((n, 2))
    b = np.where(b.sum(1, keepdims=True) > 1, 1 - b, b)
    aim = tris[:, 0] + b[:, :1] * (tris[:, 1] - tris[:, 0]) + b[:, 1:] * (tris[:, 2] - tris[:, 0])   # points inside triangles
    d = (aim - o).astype(np.float64)
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
    tmax = np.full(n, F(1e7))
    want, _ = R.trace(merged, o, d, tmax, max_bvh_iterations=0)
    got, inst = I.trace([arrays] * len(M), W, o, d, tmax, max_bvh_iterations=0)
    hit_g, hit_w = got["triangle"] >= 0, want["triangle"] >= 0
    assert hit_g.sum() > n // 3
    # a hit or miss may part only where the ray grazes an edge (a barycentric coordinate near 0: the scaled instances see
    # the triangle test's fixed determinant threshold at another scale)
    parted = np.nonzero(hit_g != hit_w)[0]
    for j in parted:
        h = got[j] if hit_g[j] else want[j]
        assert min(h["u"], h["v"], 1 - h["u"] - h["v"]) < 1e-3, f"ray {j}: {got[j]} vs merged {want[j]}"
    assert len(parted) <= n // 500
    both = np.nonzero(hit_g & hit_w)[0]
    source = np.array([key.get(merged.positions[t].tobytes(), (-1, -1)) for t in want["triangle"][both]])
    same = (source[:, 0] == inst[both]) & (source[:, 1] == got["triangle"][both])
    # t to 3e-5 (the roundings of a rotated, scaled copy; and 1e-6 of the scene near the origin), except on rays nearly parallel to the triangle (|cos| < 0.05), where t is ill-conditioned: 1e-3 there
    k = both[same]
    v = merged.positions[want["triangle"][k]].astype(np.float64)
    normal = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    cos = np.abs((normal * d[k]).sum(1)) / np.linalg.norm(normal, axis=1)
    flat = cos < 0.05
    np.testing.assert_allclose(got["t"][k[~flat]], want["t"][k[~flat]], rtol=3e-5, atol=1e-6 * extent)   # (unit directions)
    np.testing.assert_allclose(got["t"][k[flat]], want["t"][k[flat]], rtol=1e-3)
    assert flat.sum() <= n // 50
    # another instance or triangle: a near-tie (the two t agree to 1e-5; the duplicate instance ties exactly), or a ray that
    # grazes an edge of one of the two triangles and goes through to a neighbour
    graze = lambda h: min(h["u"], h["v"], 1 - h["u"] - h["v"]) < 1e-3
    for j in both[~same]:
        tie = abs(float(got["t"][j]) - float(want["t"][j])) <= 1e-5 * abs(float(want["t"][j]))
        assert tie or graze(got[j]) or graze(want[j]), (j, got[j], want[j])
    assert (~same).sum() <= n // 100
    # the duplicate (instance 3) never wins its exact ties against instance 0
    assert not np.any(inst == 3)
