"""The cases of tests/instance_sdf_cases.py on the CPU, on the restatement alone (tests/instance_sdf_ref.py): the hollow member's
conditions (both signs at every pseudonormal slot, slot-decided points at every non-face slot, every named wrong variant
changing values, the sign agreeing with the float64 winding number); the shapes of the peel waves and of the set with more than
256 scene slots; and at the scale cells the share of negative hits, the reason where there is none, and the relations between
cells that the GPU must then keep.  The GPU tests (tests/test_gpu_instance_sdf_edges.py, tests/test_gpu_instance_sdf_scale.py)
compare bytes with the restatement on these same cases, so what is pinned here is what they cover."""
import numpy as np
import pytest

import instance_point_scale_cases as SC
import instance_ref as IR
import instance_sdf_cases as C
import instance_sdf_ref as IS
import point_query_ref as R
import sdf_ref as S

F = np.float32


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# the hollow member -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hollow():
    positions, of, maps, kinds = C.hollow_set()
    pts, feature = C.hollow_points()
    W = IR.world_to_object(maps)
    parts = IS.signed_parts([positions], of, maps, W, pts)
    return dict(positions=positions, of=of, maps=maps, kinds=kinds, pts=pts, feature=feature, W=W, parts=parts)


def test_the_hollow_member_is_closed_and_spreads_the_corner_roles():
    pos, tri = C.hollow()
    positions = S.corners_of(pos, tri)
    info = S.derive(positions)["info"]
    assert len(tri) == 64 and info["closed"] == 1 and info["degenerate_triangles"] == 0
    lo, hi = pos.min(0), pos.max(0)
    assert np.array_equal(lo, F([-2, -2, -1.5])) and np.array_equal(hi, F([2, 2, 7.5]))
    # the winding is the unrotated mesh's: the same face normals, triangle by triangle
    box_pos, box_tri = S.cube()
    spike_pos, spike_tri = S.fan_spike()
    plain = np.concatenate([S.corners_of(box_pos * F([4, 4, 9]) + F([-2, -2, -1.5]), box_tri), S.corners_of(spike_pos, spike_tri[:, ::-1])])
    n0, n1 = S.face_normals(plain.reshape(-1, 3, 3))[0], S.face_normals(positions.reshape(-1, 3, 3))[0]
    assert np.abs(n0 - n1).max() < 1e-6
    apex = np.nonzero((positions.reshape(-1, 3, 3) == F([0, 0, 6])).all(2))
    assert set(apex[1].tolist()) == {0, 1, 2}, "the apex is corner a, b and c of some triangle"
    assert abs(S.winding_number(positions, [[0, 0, 3.0]])[0]) < 1e-9 and abs(S.winding_number(positions, [[1.5, 1.5, 3.0]])[0] - 1) < 1e-9


def test_values_of_is_the_restatement(hollow):
    h = hollow
    want, rec, inst = IS.signed_over_instances([h["positions"]], h["of"], h["maps"], h["W"], h["pts"])
    assert np.array_equal(bits(IS.values_of(h["parts"])), bits(want))
    assert np.array_equal(R.as_bits(rec), R.as_bits(h["parts"]["records"])) and np.array_equal(inst, h["parts"]["instances"])


def test_the_torch_restatement_is_the_numpy_one(hollow):
    """signed_over_instances(device=...) runs both brute forces through torch (each fp32 operation in float64, rounded): the
    same bytes, here on the CPU device"""
    h = hollow
    some = h["pts"][:600]
    a = IS.signed_over_instances([h["positions"]], h["of"], h["maps"], h["W"], some)
    b = IS.signed_over_instances([h["positions"]], h["of"], h["maps"], h["W"], some, device="cpu")
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(R.as_bits(a[1]), R.as_bits(b[1])) and np.array_equal(a[2], b[2])
    assert (a[0] < 0).sum() > 100 and (a[0] > 0).sum() > 100


def test_both_signs_at_every_slot_and_slot_decided_points_at_every_non_face_slot(hollow):
    f = C.slot_figures(hollow["parts"])
    print(f)
    assert len(hollow["pts"]) <= 4096
    for k, name in enumerate(C.SLOTS):
        assert f["negative"][k] >= 5 and f["positive"][k] >= 5, (name, f)
        if k > 0:
            assert f["decided"][k] >= 15, (name, f)
    assert f == {"negative": [1716, 94, 18, 25, 146, 234, 220], "positive": [1356, 12, 17, 11, 128, 45, 74],
                 "decided": [1, 91, 24, 27, 185, 145, 170]}, "the figures of the module's docstring"


def test_every_named_variant_changes_values(hollow):
    changed = C.changed_by(hollow["parts"])
    print(changed)
    assert set(changed) == set(C.VARIANTS) and len(changed) == 6
    for name, count in changed.items():
        assert count >= 15, (name, changed)
    assert list(changed.values()) == [80, 37, 89, 109, 16, 23], "the figures of the module's docstring"
    base = IS.values_of(hollow["parts"])
    assert C.reproduced_by(hollow["parts"], base) == []
    for name, pick in C.VARIANTS.items():
        assert C.reproduced_by(hollow["parts"], IS.values_of(hollow["parts"], pick)) == [name]


def test_the_hollow_sign_agrees_with_the_winding_number(hollow):
    h = hollow
    parts = h["parts"]
    inst = parts["instances"]
    values = IS.values_of(parts)
    assert set(inst.tolist()) == set(range(9)) - {4}, "every kind of map is some point's nearest instance, the duplicate never"
    assert np.array_equal(h["maps"][4].view(np.uint32), h["maps"][1].view(np.uint32))
    keep, inside = C.winding_agreement([h["positions"]], h["of"], h["maps"], h["pts"], values, inst)
    left_out = 1.0 - keep.mean()
    print(f"{left_out:.3%} of {len(keep)} points left out")
    assert left_out <= 0.10 and abs(left_out - 0.069) < 0.001
    bad = np.nonzero(keep & ((values < 0) != inside))[0]
    assert len(bad) == 0, [(h["kinds"][inst[j]], h["pts"]["p"][j], values[j]) for j in bad[:5]]
    for f in range(3):
        assert ((h["feature"] == f) & (values < 0)).sum() > 200 and ((h["feature"] == f) & (values > 0)).sum() > 200


# the peel shapes and the many-scene set --------------------------------------------------------------------------------------
def test_the_peel_waves_have_their_shapes():
    scenes, of, maps = C.peel_set()
    assert len(of) >= 64 and len(set(of)) == 4 and all(S.derive(p)["info"]["closed"] == 1 for p in scenes)
    pts, wanted = C.peel_points()
    values, rec, inst = IS.signed_over_instances(scenes, of, maps, IR.world_to_object(maps), pts)
    C.assert_peel_shapes(inst, wanted)
    assert ((values < 0).sum(), (values > 0).sum(), np.isnan(values).sum()) == (82, 75, 200)
    for w in (0, 1):        # both signs and every scene in the two full waves
        lanes = slice(64 * w, 64 * w + 64)
        assert (values[lanes] < 0).sum() >= 16 and (values[lanes] > 0).sum() >= 16 and {of[i] for i in inst[lanes]} == {0, 1, 2, 3}


def test_the_many_scene_set_has_its_shape():
    scenes, of, maps, pts = C.many_scene_set()
    assert len(scenes) == 260 and of == list(range(260))
    assert len({p.tobytes() for p in scenes}) >= 14
    values, rec, inst = IS.signed_over_instances(scenes, of, maps, IR.world_to_object(maps), pts)
    C.assert_many_scene_shapes(values, inst)


# the scale cells -------------------------------------------------------------------------------------------------------------
def test_the_tables_name_every_cell():
    cells = C.scale_cells()
    assert len(set(cells)) == len(cells) == len(SC.CELLS) + 7
    assert set(C.NEGATIVE_SHARE) | set(C.NO_SIGN) == set(cells) and not set(C.NEGATIVE_SHARE) & set(C.NO_SIGN)
    assert {k for k in cells if k[0] in ("world", "far", "ill", "negzero")} | set(C.SIGN_KEEPING_CELLS) == set(C.NEGATIVE_SHARE)


@pytest.mark.parametrize("key", C.scale_cells(), ids=lambda k: f"{k[0]} {k[1]}")
def test_the_share_of_negative_hits_at_a_cell(pkg, key):
    parts = C.cell_parts(pkg, key)
    share = C.negative_share(parts)
    hit = parts["instances"] >= 0
    print(f"{key}: {share:.2%} of {int(hit.sum())} hits are negative")
    assert hit.sum() > 900
    if key in C.NEGATIVE_SHARE:
        assert share >= C.MIN_NEGATIVE_SHARE and abs(100 * share - C.NEGATIVE_SHARE[key]) <= 0.05, (key, share)
        assert C.usable_sign_vectors(parts) == sum(x.shape[0] * 7 for x in parts["sign_data"])
    else:
        assert share == 0.0, (key, share)
        if C.NO_SIGN[key] == "no sign vector":
            assert C.usable_sign_vectors(parts) == 0 and not (parts["records"]["dist2"][hit] == 0).all()
            sigma = IS.sigma_of(parts, *IS.object_slots(parts))
            assert (sigma[hit & (parts["object"]["triangle"] >= 0)] == 0).all()
        else:
            assert (parts["records"]["dist2"][hit] == 0).all()


@pytest.mark.parametrize("k", (20, 32))
def test_a_covariant_world_scale_scales_the_values(pkg, k):
    base, scaled = IS.values_of(C.cell_parts(pkg, ("world", 0))), IS.values_of(C.cell_parts(pkg, ("world", k)))
    assert np.array_equal(bits(scaled), bits(base * F(2.0 ** k)))


@pytest.mark.parametrize("a", (-64, -40, -30, -20, 20, 30, 40, 64))
def test_a_cancelling_scale_keeps_the_records_and_loses_the_sign_beyond_2_to_the_30(pkg, a):
    base, cell = C.cell_parts(pkg, ("world", 0)), C.cell_parts(pkg, ("cancel", a))
    assert np.array_equal(R.as_bits(cell["records"]), R.as_bits(base["records"])) and np.array_equal(cell["instances"], base["instances"])
    v0, v = IS.values_of(base), IS.values_of(cell)
    same = float((bits(v) == bits(v0)).mean())
    print(f"a = {a}: {same:.2%} of the values are the base's")
    if a in (-20, 20, 30):
        assert np.array_equal(bits(v), bits(v0))
    elif a == -30:
        assert 0.95 < same < 1.0       # measured: 96.94 %
    else:
        assert np.array_equal(bits(v), bits(np.abs(v0))) and (v0 < 0).sum() > 100
