"""Instanced signed distance queries on the GPU at the scale cells: those of tests/instance_point_scale_cases.py and the
sign-keeping cells of tests/instance_sdf_cases.py (member scales of 2^+-20 and 2^+-30, where the sign data is still usable), with
the member scenes that tests/test_gpu_instance_point_scale.py makes for them.  Per cell every byte of the values, the records
and the instance indices against the restatement (tests/instance_sdf_ref.py, with the set's own W) on the host and the device
path with 1, 63, 64, 65 and all points.  tests/test_instance_sdf_cases_reference.py pins on the CPU what the sign half does
there: at least 3 % of the hits are negative at the world, far, ill-conditioned, negative-zero and sign-keeping cells, and none
is where a member at 2^+-40 or beyond has no sign vector left or every dist2 is 0, cells the kernel reaches with a NaN or
infinite seed, an object dist2 of 0 or +inf and a sigma of +-0.  Then the relations between cells that the GPU must keep: a
covariant world scale scales the values, a cancelling scale of 2^+-20 or 2^30 keeps their bytes, and one of 2^+-40 or 2^+-64
keeps the records and loses the sign; and one set taken from the k = 0 maps to the k = 40 maps by a device update and back by a
host update."""
import numpy as np
import pytest

import instance_point_scale_cases as SC
import instance_sdf_cases as C
import instance_sdf_ref as IS
import point_query_ref as R
import test_gpu_instance_point as G
import test_gpu_instance_point_scale as PS
from test_gpu_instance_point_scale import members_of
from test_gpu_instance_sdf import assert_records, assert_values, dev_points, device_form, host_records

pytestmark = pytest.mark.gpu

F = np.float32
COUNTS = (1, 63, 64, 65)
_sets = []
_memo = {}


@pytest.fixture(scope="module", autouse=True)
def close_what_the_module_made():
    yield
    for s in _sets + PS._sets + G._sets:
        s.close()
    _sets.clear()
    PS._sets.clear()
    G._sets.clear()
    for _, scene, world in PS._scenes.values():
        scene.close()
        if world is not None:
            world.close()
    PS._scenes.clear()
    for _, sc in G._members.values():
        sc.close()
    G._members.clear()
    _memo.clear()


def restate(members, of, maps, s, pts):
    with np.errstate(all="ignore"):
        return IS.signed_over_instances([m[0] for m in members], of, maps, s.world_to_object(), pts, device="cuda")


def run(pkg, key, c, trees=False):
    """(cell, set, restated values, records, instances) of a cell, once per module; `key` (cancel, 0) is the a = 0 twin: the
    ("world", 0) cell over the unscaled scenes' own trees"""
    if key not in _memo:
        members = members_of(pkg, c, trees=trees)
        s = pkg.tracer.InstanceSet([members[k][1] for k in c.of], c.maps)
        _sets.append(s)
        _memo[key] = (c, s) + restate(members, c.of, c.maps, s, c.points)
    return _memo[key]


def cell_run(pkg, key):
    return run(pkg, key, SC.cell(pkg, key))


def twin_run(pkg):
    return run(pkg, ("cancel", 0), SC.cell(pkg, ("world", 0)), trees=True)


def check_every_count(s, pts, want, want_rec, want_inst, what):
    for count in COUNTS + (len(pts),):
        got, rec, inst = s.signed_distance(pts[:count], closest=True)
        assert_records(rec, inst, want_rec[:count], want_inst[:count], f"{what}, {count} points, host path")
        assert_values(got, want[:count], f"{what}, {count} points, host path")
        got, rec, inst = device_form(s, pts[:count])
        assert_records(rec, inst, want_rec[:count], want_inst[:count], f"{what}, {count} points, device path")
        assert_values(got, want[:count], f"{what}, {count} points, device path")
    got, _, _ = device_form(s, pts, records=False, instances=False)
    assert_values(got, want, f"{what}, device path, buffers omitted")


# 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", C.scale_cells(), ids=lambda k: f"{k[0]} {k[1]}")
def test_a_cell_equals_the_restatement(pkg, gpu, key):
    c, s, want, want_rec, want_inst = cell_run(pkg, key)
    hit = want_inst >= 0
    with np.errstate(invalid="ignore"):
        share = float((want[hit] < 0).mean())
    print(f"{c}: {share:.2%} of {int(hit.sum())} hits are negative")
    # the CPU test's table, on the GPU's own W and scenes
    if key in C.NEGATIVE_SHARE:
        assert share >= C.MIN_NEGATIVE_SHARE, (key, share)
    else:
        assert share == 0.0 and hit.sum() > 900, (key, share)
    check_every_count(s, c.points, want, want_rec, want_inst, str(c))


# 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (20, 32))
def test_a_covariant_world_scale_scales_the_values(pkg, gpu, k):
    c0, s0, *_ = cell_run(pkg, ("world", 0))
    c, s, *_ = cell_run(pkg, ("world", k))
    base, scaled = s0.signed_distance(c0.points), s.signed_distance(c.points)
    assert (base < 0).sum() > 100
    assert_values(scaled, base * F(2.0 ** k), f"world 2^{k} against 2^{k} times world 2^0")
    got, _, _ = device_form(s, c.points)
    assert_values(got, base * F(2.0 ** k), f"world 2^{k}, device path")


@pytest.mark.parametrize("a", (-64, -40, -20, 20, 30, 40, 64))
def test_a_cancelling_scale_against_its_twin(pkg, gpu, a):
    """The scenes at 2^a under linear parts x 2^-a, against the a = 0 set made the same way: the records and instances are the
    twin's; the values are the twin's bytes while the sign data survives (a = -20, 20, 30) and the twin's absolute values where
    none is left (2^+-40, 2^+-64)."""
    c, s, want, want_rec, want_inst = cell_run(pkg, ("cancel", a))
    c0, s0, want0, want_rec0, want_inst0 = twin_run(pkg)
    base, rec0, inst0 = s0.signed_distance(c0.points, closest=True)
    assert_records(rec0, inst0, want_rec0, want_inst0, "the a = 0 twin")
    assert_values(base, want0, "the a = 0 twin")
    assert (base < 0).sum() > 100
    expect = base if abs(a) <= 30 else np.abs(base)
    got, rec, inst = s.signed_distance(c.points, closest=True)
    assert_records(rec, inst, rec0, inst0, f"{c} against the a = 0 set")
    assert_values(got, expect, f"{c} against the a = 0 set")
    got, rec, inst = device_form(s, c.points)
    assert_records(rec, inst, rec0, inst0, f"{c} against the a = 0 set, device path")
    assert_values(got, expect, f"{c} against the a = 0 set, device path")


# 3 ---------------------------------------------------------------------------------------------------------------------------
def test_a_device_update_across_magnitudes_and_a_host_update_back(pkg, gpu):
    """One set goes from the k = 0 maps to the k = 40 maps by update_into on a side stream with the signed query behind it on
    that stream, and back by the host update: each state against its restatement."""
    import torch
    c0, c40 = SC.cell(pkg, ("world", 0)), SC.cell(pkg, ("world", 40))
    members = members_of(pkg, c0)
    s = pkg.tracer.InstanceSet([members[k][1] for k in c0.of], c0.maps)
    _sets.append(s)
    first = s.signed_distance(c0.points)
    n = len(c40.points)
    d_maps, d_pts = torch.from_numpy(c40.maps).cuda(), dev_points(c40.points)
    d_out = torch.full((n,), -7.0, dtype=torch.float32, device="cuda")
    d_rec = torch.full((n, 8), -7, dtype=torch.int32, device="cuda")
    d_inst = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s.update_into(d_maps.data_ptr(), side.cuda_stream)
        s.signed_distance_into(d_pts.data_ptr(), n, d_out.data_ptr(), d_rec.data_ptr(), d_inst.data_ptr(), side.cuda_stream)
    side.synchronize()
    assert s.update_status() == -1
    want, want_rec, want_inst = restate(members, c40.of, c40.maps, s, c40.points)
    assert_records(host_records(d_rec), d_inst.cpu().numpy(), want_rec, want_inst, "after the device update to 2^40")
    assert_values(d_out.cpu().numpy(), want, "after the device update to 2^40")
    assert (want < 0).sum() > 100
    s.update(c0.maps)
    want0, want_rec0, want_inst0 = restate(members, c0.of, c0.maps, s, c0.points)
    assert (R.as_bits(want_rec0) != R.as_bits(want_rec)).any(1).sum() > 500
    assert_values(first, want0, "before the updates")
    check_every_count(s, c0.points, want0, want_rec0, want_inst0, "after the host update back to 2^0")
