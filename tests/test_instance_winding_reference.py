"""The restatement of the instanced winding-number query (tests/instance_winding_ref.py,
include/shader_ray_instance_winding.h) pinned on the CPU: one identity instance is winding_ref's answer byte for byte; on closed
meshes under maps of every kind the orientation is the sign of the float64 determinant of the object-to-world map, the sum is
the float64 winding number of the placed world meshes within bounds measured here, and the inside test
agrees with float64 away from the surfaces; a mirrored cube is +1 inside (and -1 without the orientation); overlapping
instances give 2, an inward-wound member -1 and is not "contained"; an exact duplicate is contained by the lower index; an open
member equals the world value under similarity maps and its own-frame value under the others; non-finite and overflowing
points give NaN."""
import math

import numpy as np
import pytest

import instance_point_cases as IC
import instance_point_ref as IP
import instance_ref as IR
import instance_winding_ref as IW
import point_query_ref as R
import sdf_ref as S
import winding_ref as WR
from test_instance_sdf_reference import displaced_points, world_meshes

F = np.float32
EYE = IC.EYE
# the restatement against the float64 sum over the world meshes at the kept points: measured maxima over the three closed
# meshes under all of MAP_KINDS 1.43e-6 (exact) and 2.14e-2 (beta 2), both on the lobed sphere; each bound is
# twice its measured value: the inputs are seeded, so the margin covers only a numpy version's summation
EXACT_BOUND, BETA2_BOUND = 2.9e-6, 4.3e-2
SIMILARITIES = ("identity", "translation", "rotation_uniform", "signed_permutation", "flip")
_members = {}


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same(got, want):
    g, w = np.asarray(got, F).reshape(-1), np.asarray(want, F).reshape(-1)
    return bool(((bits(g) == bits(w)) | (np.isnan(g) & np.isnan(w))).all())


def member(pkg, tmp_path_factory, name):
    """winding_ref.Restated of a named mesh, loaded once"""
    if name not in _members:
        if name == "lobed 8x16":
            pos, tri = pkg.scenes.lobed_sphere_mesh(8, 16, ears=False)
            pos = pos.astype(F)
        elif name in WR.MESHES:
            pos, tri = getattr(WR, name)()
        else:
            pos, tri = getattr(S, name)()
        path = str(tmp_path_factory.mktemp("instance_winding_ref") / f"{name.replace(' ', '_')}.trisrc")
        pkg.scenes.write_trisrc(path, pos, tri, normals=np.tile(np.array([0, 0, 1], F), (len(pos), 1)))
        world = pkg.World(path)
        _members[name] = WR.Restated(world)
        world.close()
    return _members[name]


def make_points(p):
    pts = np.zeros(len(p), R.POINT_DTYPE)
    pts["p"], pts["max_dist2"] = p, np.inf
    return pts


# 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cube", "open_cube"])
def test_one_identity_instance_is_the_winding_restatement(pkg, tmp_path_factory, name):
    ref = member(pkg, tmp_path_factory, name)
    pts, _, _ = IC.world_points([ref.positions], [0], EYE[None], 600, seed=11)
    assert np.array_equal(IW.orientations(EYE[None]), [1.0])
    for beta in (2.0, 0.5, math.inf):
        want = ref.w(pts, beta)
        got, containing = IW.winding_over_instances([ref], [0], EYE[None], pts, beta)
        assert same(got, want) and np.isnan(want).sum() > 20 and ((want > 0.5).sum() > 20 or beta == 0.5)
        assert np.array_equal(containing, np.where(want > F(0.5), 0, -1))
        records = R.closest(ref.positions, pts)
        signed, rec, inst = IW.winding_signed_over_instances([ref], [0], EYE[None], EYE[None], pts, beta)
        assert np.array_equal(R.as_bits(rec), R.as_bits(records)) and np.array_equal(inst, np.where(records["triangle"] >= 0, 0, -1))
        assert same(signed, WR.winding_signed(records, want))
        assert ((signed < 0).sum() > 10 or beta == 0.5) and (signed > 0).sum() > 20 and np.isnan(signed).sum() > 20


# 2 ---------------------------------------------------------------------------------------------------------------------------
def kept_points(positions, of, maps, p, sizes, what):
    """the points at least 1e-3 world sizes of the nearest instance from every surface; at most 10 % may be left out"""
    rec, inst = IP.closest_over_instances(positions, of, maps, make_points(p))
    assert (inst >= 0).all()
    keep = np.sqrt(rec["dist2"].astype(np.float64)) >= 1e-3 * sizes[inst]
    print(f"{what}: {1 - keep.mean():.3%} of {len(p)} points left out")
    assert 1 - keep.mean() <= 0.10, what
    return keep


def world_winding(world, p):
    """the float64 sum of the winding numbers of the world meshes"""
    return sum(S.winding_number(w.reshape(-1), p) for w in world)


@pytest.mark.parametrize("name", ["cube", "tetrahedron", "lobed 8x16"])
def test_closed_members_under_every_kind_of_map(pkg, tmp_path_factory, name):
    ref = member(pkg, tmp_path_factory, name)
    assert S.derive(ref.positions)["info"]["closed"] == 1
    rng = np.random.default_rng(len(name))
    maps = np.stack([IC.map_of(kind, rng, ref.positions, 1.2) for kind in IC.MAP_KINDS]).astype(F)
    of = [0] * len(maps)
    W = IR.world_to_object(maps)
    s = IW.orientations(W)
    assert np.array_equal(s, np.sign(np.linalg.det(maps[:, :, :3].astype(np.float64)))), "the orientation is the forward map's"
    assert s[IC.MAP_KINDS.index("mirror")] == -1 and (s == 1).sum() >= 5
    world, sizes = world_meshes([ref.positions], of, maps)
    p = displaced_points(world, sizes, 1600, rng)
    keep = kept_points([ref.positions], of, maps, p, sizes, name)
    w64 = world_winding(world, p)
    print(f"{name}: {int((w64[keep] > 1.5).sum())} kept points in overlaps, {int((w64[keep] < -0.5).sum())} inside the mirrored instances only")
    assert (w64[keep] > 0.5).sum() > 50 and (np.abs(w64[keep]) < 0.5).sum() > 50 and (w64[keep] < -0.5).sum() > 5
    for beta, bound in ((math.inf, EXACT_BOUND), (2.0, BETA2_BOUND)):
        w, containing = IW.winding_over_instances([ref], of, W, p, beta)
        err = float(np.abs(w[keep] - w64[keep]).max())
        print(f"{name}, beta {beta}: max |w - float64 world sum| = {err:.3g} over {int(keep.sum())} kept points")
        assert err <= bound, (name, beta, err)
        assert np.array_equal(w[keep] > 0.5, w64[keep] > 0.5), (name, beta)
        # the containing instance is the lowest whose own world mesh winds around the point
        own = np.stack([S.winding_number(m.reshape(-1), p) for m in world])
        sure = keep & (np.abs(np.abs(own) - 0.5) > 0.1).all(0)
        want = np.where((own > 0.5).any(0), (own > 0.5).argmax(0), -1)
        assert sure.sum() > 1000 and np.array_equal(containing[sure], want[sure]), (name, beta)


# 3 ---------------------------------------------------------------------------------------------------------------------------
GRID = np.stack(np.meshgrid(*[np.linspace(0.1, 0.9, 5)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(F)
MIRROR_X = np.array([[-1, 0, 0, 3], [0, 1, 0, 0], [0, 0, 1, 0]], F)          # the unit cube to [2, 3] x [0, 1]^2, mirrored
INSIDE_MIRRORED = (GRID * F([-1, 1, 1]) + F([3, 0, 0])).astype(F)


def test_a_mirrored_cube_that_is_outward_in_the_world_is_plus_one_inside(pkg, tmp_path_factory):
    """A mirror reverses the winding of what it places.  The cube whose mirror image is wound outward in the world (the member
    is wound inward) is +1 inside, as the float64 winding number of its world mesh says; a restatement without s_i gives -1
    there and fails.  The mirror image of the outward-wound member is an inward-wound world mesh: -1, again the world's
    value."""
    inward, cube = member(pkg, tmp_path_factory, "inward_cube"), member(pkg, tmp_path_factory, "cube")
    maps = MIRROR_X[None]
    W = IR.world_to_object(maps)
    assert np.array_equal(IW.orientations(W), [-1.0])
    for ref, value in ((inward, 1.0), (cube, -1.0)):
        w64 = S.winding_number(IP.map_corners(maps[0], ref.positions), INSIDE_MIRRORED)
        assert np.abs(w64 - value).max() < 1e-12
        for beta, tol in ((math.inf, EXACT_BOUND), (2.0, BETA2_BOUND)):
            w, containing = IW.winding_over_instances([ref], [0], W, INSIDE_MIRRORED, beta)
            assert np.abs(w - value).max() <= tol and (containing == (0 if value > 0 else -1)).all()
            v, vc = IW.winding_over_instances([ref], [0], W, INSIDE_MIRRORED, beta, signs=[1.0])
            assert np.abs(v + value).max() <= tol and (vc == (-1 if value > 0 else 0)).all(), "without s_i the sign is the member's, not the world's"
            assert not np.array_equal(v > 0.5, w > 0.5), "the variant without s_i fails the inside test"


# 4 ---------------------------------------------------------------------------------------------------------------------------
def test_overlaps_count_and_an_inward_member_is_not_contained(pkg, tmp_path_factory):
    cube, inward = member(pkg, tmp_path_factory, "cube"), member(pkg, tmp_path_factory, "inward_cube")
    # the cube, and a mirrored one, outward in the world, at [0.5, 1.5]^3: the overlap is [0.5, 1]^3
    second = np.array([[-1, 0, 0, 1.5], [0, 1, 0, 0.5], [0, 0, 1, 0.5]], F)
    maps = np.stack([EYE, second])
    W = IR.world_to_object(maps)
    members, of = [cube, inward], [0, 1]
    assert np.array_equal(IW.orientations(W), [1.0, -1.0])
    both = GRID[(GRID > 0.5).all(1)]
    first_only = GRID[(GRID < 0.5).any(1)]
    second_only = np.array([[1.25, 1.25, 1.25], [1.4, 0.7, 0.8]], F)
    outside = np.array([[-0.5, 0.5, 0.5], [0.5, 1.7, 0.5], [2, 2, 2], [10, -4, 7]], F)
    for beta, tol in ((math.inf, EXACT_BOUND), (2.0, BETA2_BOUND)):
        for p, value, inst in ((both, 2.0, 0), (first_only, 1.0, 0), (second_only, 1.0, 1), (outside, 0.0, -1)):
            w, containing = IW.winding_over_instances(members, of, W, p, beta)
            assert np.abs(w - value).max() <= 2 * tol and (containing == inst).all(), (beta, value)
        signed = IW.winding_signed_over_instances(members, of, maps, W, make_points(both), beta)[0]
        assert (signed < 0).all(), "the union's sign is negative in the overlap"
        w, containing = IW.winding_over_instances([inward], [0], EYE[None], GRID, beta)
        assert np.abs(w + 1).max() <= tol and (containing == -1).all(), "-1 is not contained"
        # an inward member inside an outward one cancels it: 0, yet the outward instance contains the point
        w, containing = IW.winding_over_instances(members, [1, 0], np.stack([EYE, EYE]), GRID, beta)
        assert np.abs(w).max() <= 2 * tol and (containing == 1).all()


# 5 ---------------------------------------------------------------------------------------------------------------------------
def test_containing_is_the_lowest_instance_on_an_exact_duplicate(pkg, tmp_path_factory):
    cube = member(pkg, tmp_path_factory, "cube")
    of, maps, kinds = IC.make_set([cube.positions], [0] * 6, seed=5, spread=0.4)
    assert kinds[4] == "duplicate of 1" and kinds[1] == "translation"
    W = IR.world_to_object(maps)
    p = (GRID.astype(np.float64) @ maps[1][:, :3].astype(np.float64).T + maps[1][:, 3]).astype(F)      # inside instances 1 and 4
    w, containing = IW.winding_over_instances([cube], of, W, p, 2.0)
    t = IW.terms([cube], of, W, p, 2.0)
    assert same(t[1], t[4]) and (t[1] > 0.5).all()
    assert (containing <= 1).all() and (containing == 1).sum() > 10, "never the duplicate at instance 4"
    alone, only = IW.winding_over_instances([cube], [0, 0], W[[1, 4]], p, 2.0)
    assert (alone > 1.5).all() and (only == 0).all()


# 6 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", IC.MAP_KINDS)
def test_an_open_member_is_the_world_value_under_similarities_and_its_own_frame_value_otherwise(pkg, tmp_path_factory, kind):
    """open_cube (5/6 at its centre).  Under the similarity kinds the restatement is compared with the float64 winding number of
    the world mesh; under rotation_nonuniform, shear and mirror (a non-uniform one) with s * the float64 winding number of the
    object mesh at the object point, the value the header defines; its difference from the world value is printed (DESIGN
    section 28), not asserted."""
    ref = member(pkg, tmp_path_factory, "open_cube")
    rng = np.random.default_rng(60 + IC.MAP_KINDS.index(kind))
    maps = IC.map_of(kind, rng, ref.positions, 1.2)[None].astype(F)
    W = IR.world_to_object(maps)
    world, sizes = world_meshes([ref.positions], [0], maps)
    p = displaced_points(world, sizes, 600, rng)
    keep = kept_points([ref.positions], [0], maps, p, sizes, f"open_cube, {kind}")
    w_world = S.winding_number(world[0].reshape(-1), p)
    w_frame = float(IW.orientations(W)[0]) * S.winding_number(ref.positions, IW.IS.object_points(W[0], p))
    gap = float(np.abs(w_frame - w_world)[keep].max())
    print(f"open_cube, {kind}: max |own-frame value - world value| = {gap:.3g}")
    want = w_world if kind in SIMILARITIES else w_frame
    for beta, bound in ((math.inf, EXACT_BOUND), (2.0, BETA2_BOUND)):
        w = IW.winding_over_instances([ref], [0], W, p, beta)[0]
        err = float(np.abs(w - want)[keep].max())
        print(f"open_cube, {kind}, beta {beta}: max error {err:.3g}")
        assert err <= bound, (kind, beta, err)


# 7 ---------------------------------------------------------------------------------------------------------------------------
def test_non_finite_and_overflowing_points_are_nan(pkg, tmp_path_factory):
    cube = member(pkg, tmp_path_factory, "cube")
    grown = (EYE * F(2.0 ** 20)).astype(F)              # W scales by 2^-20
    squeezed = EYE.copy()
    squeezed[0, 0] = F(2.0 ** -70)                      # W scales x by 2^70
    maps = np.stack([grown, squeezed])
    W = IR.world_to_object(maps)
    assert W[1, 0, 0] == F(2.0 ** 70) and W[0, 0, 0] == F(2.0 ** -20)
    p = np.array([[np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [0.5, 0.5, -np.inf],      # non-finite world points: no walk
                  [2.0 ** 60, 0.5, 0.5], [-2.0 ** 62, 0.25, 2.0]], F)               # p_o overflows in instance 1 only
    with np.errstate(all="ignore"):
        assert np.isfinite(IR.object_vectors(W[0], p[3:], True)).all() and not np.isfinite(IR.object_vectors(W[1], p[3:5], True)).all(1).any()
    for beta in (2.0, math.inf):
        w, containing = IW.winding_over_instances([cube], [0, 0], W, p, beta)
        assert np.isnan(w).all() and (containing == -1).all()
        t = IW.terms([cube], [0, 0], W, p[3:5], beta)
        assert np.isfinite(t[0]).all() and np.isnan(t[1]).all(), "only the squeezed instance's term is NaN"
        signed, rec, inst = IW.winding_signed_over_instances([cube], [0, 0], maps, W, make_points(p), beta)
        assert np.isnan(signed[:3]).all() and (inst[:3] == -1).all(), "a non-finite point is a miss"
        assert (inst[3:] >= 0).all() and (signed[3:] > 0).all(), "a NaN sum is not above 0.5: the value is positive"
