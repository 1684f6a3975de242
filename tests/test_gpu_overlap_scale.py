"""Box-overlap queries on the GPU on scenes scaled by 2^-90 to 2^67 (tests/overlap_scale_cases.py) against the restatement
(tests/overlap_ref.py): every index and every count of every cell and of both special classes through test_gpu_overlap's
check_every_k -- the underflow end, where the later stages' products are subnormal and then 0, and the overflow end, where they
are infinite and NaN and nothing may separate; a device refit that changes a resident scene's magnitude, with the walk's
counters against overlap_ref.walk_counters over the refit boxes; DeviceWorld under GEOMETRY_SCALE; and a count split over two
launches at a scaled cell.  No tolerance anywhere."""
import os

import numpy as np
import pytest

import overlap_cases as OC
import overlap_ref as OR
import overlap_scale_cases as SC
import ray_scale_cases as X
import refit_ref as R
from test_gpu_overlap import assert_same, check_every_k, device_boxes

pytestmark = pytest.mark.gpu

F = np.float32
CELLS = [(name, k) for name in SC.SCENES for k in SC.S_EXPONENTS + tuple(SC.SPECIAL_CELLS)]


def scaled_rows(pkg, name, s_exp):
    """the unscaled triangles times S as sorted raw rows"""
    return X.triangle_rows(SC.scaled_positions(pkg, name, s_exp))


@pytest.fixture(scope="module")
def worlds(pkg, gpu):
    """worlds(name, k): (positions of the world loaded under GEOMETRY_SCALE = 2^k, its resident host-built scene), once"""
    made = {}

    def get(name, s_exp):
        if (name, s_exp) not in made:
            world = X.load_scaled(pkg, name, s_exp)
            positions = np.asarray(world.arrays()["vertex_positions"], F).copy()
            assert np.array_equal(X.triangle_rows(positions), scaled_rows(pkg, name, s_exp)), (name, s_exp)
            made[(name, s_exp)] = (world, positions, pkg.Scene(world.flatten()))
        return made[(name, s_exp)][1:]

    yield get
    for world, _, scene in made.values():
        scene.close()
        world.close()


@pytest.mark.parametrize("name, cell", CELLS)
def test_every_cell(pkg, gpu, worlds, name, cell):
    s_exp = SC.SPECIAL_CELLS.get(cell, cell)
    positions, scene = worlds(name, s_exp)
    _, boxes = SC.inputs(pkg, name, cell)
    code = OR.first_axis(positions, boxes)           # on the world's own triangle order
    member = code == OR.OVERLAP
    n = member.sum(1)
    # the same sets as the CPU's `positions * S`, triangle for triangle
    cpu = SC.codes(pkg, name, cell) == OR.OVERLAP
    assert np.array_equal(member[:, SC.row_order(positions)], cpu[:, SC.row_order(SC.scaled_positions(pkg, name, s_exp))]), (name, cell)
    base = SC.codes(pkg, name, 0) == OR.OVERLAP
    print(f"{name}, {cell}: {int(OR.walked(boxes).sum())} boxes walked, " +
          (f"{int((cpu != base).any(1).sum())} differ from S = 1, " if cell not in SC.SPECIAL_CELLS else "") +
          f"n = 0 / > 8 / > 64: {(n == 0).mean():.3f} / {(n > 8).mean():.3f} / {(n > 64).mean():.3f}")
    check_every_k(scene, boxes, member, f"{name}, {cell}")


def test_a_device_refit_that_changes_the_magnitude(pkg, gpu):
    """A resident S = 1 lobed_528 refit on a side stream to positions * 2^-40, queried, refit to positions * 2^50, queried, with
    no host synchronisation in between: each answer is the restatement's on the refit corners.  Then the boxes the DEVICE refit
    stored (group_boxmin / group_boxmax) equal refit_ref.node_boxes of the refit corners word for word, and the host path's
    counters equal overlap_ref.walk_counters over them (the scene's own tree, World.export_tree): at 2^50 as the stream left
    it, then after a device refit back to 2^-40 and after one to 2^-16, both on the side stream.

    What each magnitude pins.  A node's box is its corners -+ 1e-5 (box3d::add).  At 2^-40 the scene is 2.4e-12 across and the
    far boxes lie 5e-10 away, so the pad is four million times the scene: every walked box enters every node and tests every
    triangle (asserted on the restatement), and the counters there can only tell that nothing is culled.  At 2^50 the pad is
    absorbed by rounding and the boxes are the bare min / max.  2^-16 is the added step where the pad and the scene are of one
    size (4.0e-5 across, 37 % of the pairs of a walked box and a triangle tested; 5 % at 2^50): there a box that is stale,
    unpadded or padded otherwise moves the counters."""
    import torch
    world = pkg.World(OC.scene_path("lobed_528"))
    desc = world.export_tree()
    tree = R.TreeArrays.of(desc)
    vd = np.ctypeslib.as_array(desc.vertex_data, shape=(desc.vertex_count * 9,)).reshape(-1, 9).copy()
    scene = pkg.Scene(world.flatten())
    try:
        corners1 = np.ascontiguousarray(vd[tree.triangle_vertices][:, :, :3])
        assert np.array_equal(corners1.reshape(-1).view(np.uint32), np.asarray(world.arrays()["vertex_positions"], F).view(np.uint32))
        base = OC.make_boxes({"vertex_positions": corners1.reshape(-1)}, 2400, seed=17)
        forms = [(8, True, False), (8, False, False), (64, False, False), (0, True, False), (0, True, True)]
        steps = []
        for s_exp in (-40, 50):
            moved = vd.copy()
            moved[:, :3] = vd[:, :3] * F(2.0 ** s_exp)
            boxes = SC.scaled_boxes(base, s_exp)
            steps.append({"k": s_exp, "vd": moved, "boxes": boxes, "d_vd": torch.from_numpy(moved).cuda(), "d_boxes": device_boxes(boxes),
                          "out": [torch.full((len(boxes), max(k, 1)), -7, dtype=torch.int32, device="cuda") for k, _, _ in forms],
                          "cnt": [torch.full((len(boxes),), -7, dtype=torch.int32, device="cuda") for _ in forms]})
        d_tv = torch.from_numpy(tree.triangle_vertices.copy()).cuda()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for st in steps:
                scene.refit(st["d_vd"], d_tv, normal_offset=6, stream_ptr=side.cuda_stream)
                for (k, counts, any_only), out, cnt in zip(forms, st["out"], st["cnt"]):
                    scene.triangles_in_boxes_into(st["d_boxes"].data_ptr(), len(st["boxes"]), out.data_ptr() if k else 0, cnt.data_ptr() if counts else 0,
                                                  max_triangles=k, any_only=any_only, stream_ptr=side.cuda_stream)
        side.synchronize()
        sets = {}
        for st in steps:
            corners = np.ascontiguousarray(st["vd"][tree.triangle_vertices][:, :, :3])
            member = OR.overlaps(corners.reshape(-1), st["boxes"])
            sets[st["k"]] = (corners, member)
            want64, want_n = OR.from_set(member, 64)
            assert (want_n > 8).mean() > 0.2 and (want_n == 0).mean() > 0.05
            for (k, counts, any_only), out, cnt in zip(forms, st["out"], st["cnt"]):
                what = f"after the device refit to 2^{st['k']}, K = {k}, counts = {counts}, any = {any_only}"
                if k:
                    assert_same(out.cpu().numpy(), want64[:, :k], what)
                else:
                    assert bool((out == -7).all())
                if counts:
                    assert_same(cnt.cpu().numpy(), (want_n > 0).astype(np.int32) if any_only else want_n, what)
                else:
                    assert bool((cnt == -7).all())
        assert (sets[-40][1] != sets[50][1]).any()       # (both are outside the range: overlap_scale_cases.TABLE)
        now = scene.geometry()["vertex_positions"]
        assert np.array_equal(now.view(np.uint32), sets[50][0].reshape(-1).view(np.uint32))
        walked = OR.walked(base)
        moved = vd.copy()
        moved[:, :3] = vd[:, :3] * F(2.0 ** -16)
        steps.append({"k": -16, "vd": moved, "boxes": SC.scaled_boxes(base, -16), "d_vd": torch.from_numpy(moved).cuda()})
        corners = np.ascontiguousarray(moved[tree.triangle_vertices][:, :, :3])
        sets[-16] = (corners, OR.overlaps(corners.reshape(-1), steps[-1]["boxes"]))
        for st in (steps[1], steps[0], steps[2]):        # 2^50 as the stream left it, then device refits to 2^-40 and 2^-16
            s_exp = st["k"]
            corners, member = sets[s_exp]
            if s_exp != 50:
                with torch.cuda.stream(side):
                    scene.refit(st["d_vd"], d_tv, normal_offset=6, stream_ptr=side.cuda_stream)
                side.synchronize()
            if s_exp == -16:
                check_every_k(scene, st["boxes"], member, "after the device refit to 2^-16")
            assert np.array_equal(OR.walked(st["boxes"]), walked)
            node_boxes = R.node_boxes(tree, corners)
            bmin, bmax = R.flat_boxes(tree, node_boxes)
            g = scene.geometry()
            assert np.array_equal(g["vertex_positions"].view(np.uint32), corners.reshape(-1).view(np.uint32)), s_exp
            assert np.array_equal(g["group_boxmin"].view(np.uint32), bmin.view(np.uint32)) and np.array_equal(g["group_boxmax"].view(np.uint32), bmax.view(np.uint32)), s_exp
            for any_only, k in ((False, 0), (False, 8), (True, 0)):
                want = OR.walk_counters(tree, node_boxes, corners, st["boxes"], any_only=any_only, member=member)
                if not any_only and k == 0:              # does the cull reject anything at this magnitude?
                    everything = len(corners) * int(walked.sum())
                    tests = int(want["triangle_tests"].sum())
                    print(f"refit to 2^{s_exp}: the counting walk tests {tests} of {everything} pairs of a walked box and a triangle")
                    assert tests == everything if s_exp == -40 else tests < everything // 2, (s_exp, tests, everything)
                for rows in (np.arange(64), np.arange(len(st["boxes"]))):
                    _, _, c = scene.triangles_in_boxes(st["boxes"][rows], max_triangles=k, counters=True, any_only=any_only)
                    got = {key: c[key] for key in OR.COUNTERS}
                    assert got == {key: int(want[key][rows].sum()) for key in OR.COUNTERS}, (s_exp, any_only, k, len(rows))
                print(f"refit to 2^{s_exp}, {'ANY' if any_only else f'K = {k}'}: {got}")
    finally:
        scene.close()
        world.close()


@pytest.mark.parametrize("s_exp", [-64, 50])
def test_device_world_under_geometry_scale(pkg, gpu, worlds, s_exp):
    """the device-built scene of the same file at the same scale: the restatement on its own triangle order, and the host-built
    scene's counts (a count does not depend on the order)"""
    name = "lobed_528"
    before = os.environ.get("GEOMETRY_SCALE")
    os.environ["GEOMETRY_SCALE"] = X.scale_string(s_exp)
    try:
        dw = pkg.tracer.DeviceWorld(OC.scene_path(name))
    finally:
        if before is None:
            del os.environ["GEOMETRY_SCALE"]
        else:
            os.environ["GEOMETRY_SCALE"] = before
    try:
        positions = np.asarray(dw.flat_arrays()["vertex_positions"], F)
        assert np.array_equal(X.triangle_rows(positions), scaled_rows(pkg, name, s_exp))
        boxes = SC.boxes(pkg, name, s_exp)
        member = OR.overlaps(positions, boxes)
        check_every_k(dw, boxes, member, f"DeviceWorld at 2^{s_exp}")
        _, scene = worlds(name, s_exp)
        assert_same(dw.box_counts(boxes), scene.box_counts(boxes), f"DeviceWorld and the host-built scene at 2^{s_exp}")
        assert np.array_equal(member.sum(1), (SC.codes(pkg, name, s_exp) == OR.OVERLAP).sum(1))
    finally:
        dw.close()


def test_a_count_split_over_launches_at_a_scaled_cell(pkg, gpu, worlds):
    """test_gpu_overlap's test_a_count_split_over_launches on small_trisrc at 2^50: 2^24 + 3000 boxes at K = 1 with counts; the
    filler is a far, walked box that touches nothing on the restatement"""
    import torch
    s_exp = 50
    positions, scene = worlds("small_trisrc", s_exp)
    n = (1 << 24) + 3000
    real = SC.scaled_boxes(OC.make_boxes(SC.as_dict(X.base_arrays(pkg, "small_trisrc")), 3000 + 4096, seed=33), s_exp)
    tail, spread = real[:3000], real[3000:]
    far = SC.scaled_boxes(OR.make_boxes([(1e6, -2e6, 3e6)], [(1.5e6, -1e6, 4e6)]), s_exp)
    assert OR.walked(far).all() and not OR.overlaps(positions, far).any()
    d_boxes = device_boxes(far).repeat(n, 1)
    d_boxes[n - 3000:] = device_boxes(tail)
    sample = torch.from_numpy(np.random.default_rng(1).choice(n - 3000, 4096, replace=False)).cuda()
    d_boxes[sample] = device_boxes(spread)
    d_out = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    d_cnt = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    scene.triangles_in_boxes_into(d_boxes.data_ptr(), n, d_out.data_ptr(), d_cnt.data_ptr(), max_triangles=1,
                                  stream_ptr=torch.cuda.current_stream().cuda_stream)
    torch.cuda.current_stream().synchronize()
    want, want_n = OR.overlap(positions, tail, 1)
    assert (want_n > 0).mean() > 0.3
    assert_same(d_out[n - 3000:].cpu().numpy().reshape(-1, 1), want, "the last launch's boxes")
    assert_same(d_cnt[n - 3000:].cpu().numpy(), want_n, "the last launch's counts")
    want, want_n = OR.overlap(positions, spread, 1)
    assert_same(d_out[sample].cpu().numpy().reshape(-1, 1), want, "boxes of the first launch")
    assert_same(d_cnt[sample].cpu().numpy(), want_n, "counts of the first launch")
    rest = torch.ones(n - 3000, dtype=torch.bool, device="cuda")
    rest[sample] = False
    assert bool((d_out[: n - 3000][rest] == -1).all())
    assert bool((d_cnt[: n - 3000][rest] == 0).all())
