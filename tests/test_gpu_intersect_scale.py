"""Triangle-intersection queries on the GPU on scenes scaled by 2^-80 to 2^64 (tests/intersect_scale_cases.py) against the
restatement (tests/intersect_ref.py): every index and every count of every cell and of both special classes through
test_gpu_intersect's check_forms -- the underflow end, where normals and projections are subnormal and then 0, queries stop being
walked and scene triangles turn degenerate through the kernel's own cross product, and the overflow end, where projections are
infinite and NaN and nothing may separate; the self form at scaled cells; a device refit that changes a resident scene's
magnitude, with the walk's counters against intersect_ref.walk_counters over the refit boxes; DeviceWorld under GEOMETRY_SCALE;
a count split over two launches at a scaled cell with K = 1; and the flat lattice's queries with every zero negated.  At S = 1
a kernel that contracts, flushes subnormals or drops NaNs in min3 / max3 gives the right sets on these scenes
(tests/test_intersect_scale_reference.py): the cells away from 1 are where it does not.  No tolerance anywhere."""
import os

import numpy as np
import pytest

import intersect_cases as IC
import intersect_ref as IR
import intersect_scale_cases as SC
import ray_scale_cases as X
import refit_ref as R
from overlap_scale_cases import row_order
from test_gpu_intersect import assert_same, check_forms, device_triangles, flat_codes, flat_scene, item_run, self_run

pytestmark = pytest.mark.gpu

F = np.float32
CELLS = [(name, k) for name in SC.SCENES for k in SC.S_EXPONENTS + tuple(SC.SPECIAL_CELLS)]
SKIP_SHARED_AT = (-72, -40, 0, 30, 64)
SELF_AT = (-72, -33, 30, 50)


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
    _, queries = SC.inputs(pkg, name, cell)
    member = IR.intersects(queries, positions)             # on the world's own triangle order
    n = member.sum(1)
    # the same sets as the CPU's `positions * S`, triangle for triangle
    cpu = SC.codes(pkg, name, cell) == IR.INTERSECT
    assert np.array_equal(member[:, row_order(positions)], cpu[:, row_order(SC.scaled_positions(pkg, name, s_exp))]), (name, cell)
    base = SC.codes(pkg, name, 0) == IR.INTERSECT
    print(f"{name}, {cell}: {int(IR.walked(queries).sum())} queries walked, " +
          (f"{int((cpu != base).any(1).sum())} differ from S = 1, " if cell not in SC.SPECIAL_CELLS else "") +
          f"n = 0 / > 8 / > 64: {(n == 0).mean():.3f} / {(n > 8).mean():.3f} / {(n > 64).mean():.3f}")
    assert int(IR.walked(queries).sum()) == SC.walked_count(name, cell)
    check_forms(item_run(scene, queries), member, f"{name}, {cell}")
    if cell in SKIP_SHARED_AT:
        skipped = IR.intersects(queries, positions, True)
        assert not (skipped & ~member).any() and (cell == -72 or skipped.sum() < member.sum())
        check_forms(item_run(scene, queries, True), skipped, f"{name}, {cell}, SKIP_SHARED", ks=(0, 3, 8, 64))


@pytest.mark.parametrize("s_exp", SELF_AT)
@pytest.mark.parametrize("name", SC.SCENES)
def test_the_self_form_at_a_scaled_cell(pkg, gpu, worlds, name, s_exp):
    """The self form reads its nine floats from the scene's positions, not from an item array: the same arithmetic must follow.
    Every triangle of the scaled scene against the scene, with and without SKIP_SHARED."""
    positions, scene = worlds(name, s_exp)
    tris = positions.reshape(-1, 3, 3)
    pairs = []
    for skip in (False, True):
        own = IR.intersects(tris, positions, skip)
        pairs.append(int(own.sum()))
        print(f"{name}, 2^{s_exp}, self, SKIP_SHARED {skip}: {int(IR.walked(tris).sum())} of {len(tris)} walked, {pairs[-1]} pairs")
        check_forms(self_run(scene, 0, len(tris), skip), own, f"{name}, 2^{s_exp}, self, SKIP_SHARED {skip}", ks=(0, 8) if skip else (0, 1, 5, 8, 9, 64))
    assert pairs[0] > 0 and pairs[1] < pairs[0], (name, s_exp, pairs)   # (every cell of SELF_AT still has valid triangles)


def test_a_device_refit_that_changes_the_magnitude(pkg, gpu):
    """A resident S = 1 lobed_528 refit on a side stream to positions * 2^-40, queried with the item form (five forms) and the
    self form, refit to positions * 2^50, queried again, with no host synchronisation in between: each answer is the
    restatement's on the refit corners.  Then the host path's counters equal intersect_ref.walk_counters over
    refit_ref.node_boxes of the refit corners (the scene's own tree, World.export_tree): at 2^50 as the stream left it, then
    after a device refit back to 2^-40 and after one to 2^-16, both on the side stream.

    What each magnitude pins.  A node's box is its corners -+ 1e-5.  At 2^-40 the scene and every query are some 1e-12 across,
    so the pad is millions of times the scene: every walked query enters every node and tests every triangle (asserted on the
    restatement), and the counters there can only tell that nothing is culled.  At 2^50 the pad is absorbed by rounding and the
    boxes are the bare min / max.  2^-16 is the step where the pad and the scene are of one size: there a box that is stale,
    unpadded or padded otherwise moves the counters."""
    import torch
    world = pkg.World(IC.scene_path("lobed_528"))
    desc = world.export_tree()
    tree = R.TreeArrays.of(desc)
    vd = np.ctypeslib.as_array(desc.vertex_data, shape=(desc.vertex_count * 9,)).reshape(-1, 9).copy()
    scene = pkg.Scene(world.flatten())
    try:
        corners1 = np.ascontiguousarray(vd[tree.triangle_vertices][:, :, :3])
        assert np.array_equal(corners1.reshape(-1).view(np.uint32), np.asarray(world.arrays()["vertex_positions"], F).view(np.uint32))
        T = len(corners1)
        base = IC.make_queries({"vertex_positions": corners1.reshape(-1)}, 1200, seed=17)
        forms = [(8, True, False), (3, False, False), (64, True, False), (0, True, False), (0, True, True)]
        steps = []
        for s_exp in (-40, 50):
            moved = vd.copy()
            moved[:, :3] = vd[:, :3] * F(2.0 ** s_exp)
            queries = SC.scaled_queries(base, s_exp)
            steps.append({"k": s_exp, "vd": moved, "queries": queries, "d_vd": torch.from_numpy(moved).cuda(), "d_queries": device_triangles(queries),
                          "out": [torch.full((len(queries), max(k, 1)), -7, dtype=torch.int32, device="cuda") for k, _, _ in forms],
                          "cnt": [torch.full((len(queries),), -7, dtype=torch.int32, device="cuda") for _ in forms],
                          "self_out": torch.full((T, 8), -7, dtype=torch.int32, device="cuda"),
                          "self_cnt": torch.full((T,), -7, dtype=torch.int32, device="cuda")})
        d_tv = torch.from_numpy(tree.triangle_vertices.copy()).cuda()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for st in steps:
                scene.refit(st["d_vd"], d_tv, normal_offset=6, stream_ptr=side.cuda_stream)
                for (k, counts, any_only), out, cnt in zip(forms, st["out"], st["cnt"]):
                    scene.intersecting_triangles_into(st["d_queries"].data_ptr(), len(st["queries"]), out.data_ptr() if k else 0,
                                                      cnt.data_ptr() if counts else 0, max_triangles=k, any_only=any_only, stream_ptr=side.cuda_stream)
                scene.self_intersections_into(0, T, st["self_out"].data_ptr(), st["self_cnt"].data_ptr(), max_triangles=8, skip_shared=False,
                                              stream_ptr=side.cuda_stream)
        side.synchronize()
        sets = {}
        for st in steps:
            corners = np.ascontiguousarray(st["vd"][tree.triangle_vertices][:, :, :3])
            member = IR.intersects(st["queries"], corners.reshape(-1))
            sets[st["k"]] = (corners, member)
            want64, want_n = IR.from_set(member, 64)
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
            own64, own_n = IR.from_set(IR.intersects(corners, corners.reshape(-1)), 8)
            assert_same(st["self_out"].cpu().numpy(), own64, f"after the device refit to 2^{st['k']}, self")
            assert_same(st["self_cnt"].cpu().numpy(), own_n, f"after the device refit to 2^{st['k']}, self")
        assert (sets[-40][1] != sets[50][1]).any()       # (both are outside the range: intersect_scale_cases.TABLE)
        now = scene.geometry()["vertex_positions"]
        assert np.array_equal(now.view(np.uint32), sets[50][0].reshape(-1).view(np.uint32))
        walked = IR.walked(base)
        moved = vd.copy()
        moved[:, :3] = vd[:, :3] * F(2.0 ** -16)
        steps.append({"k": -16, "vd": moved, "queries": SC.scaled_queries(base, -16), "d_vd": torch.from_numpy(moved).cuda()})
        corners = np.ascontiguousarray(moved[tree.triangle_vertices][:, :, :3])
        sets[-16] = (corners, IR.intersects(steps[-1]["queries"], corners.reshape(-1)))
        for st in (steps[1], steps[0], steps[2]):        # 2^50 as the stream left it, then device refits to 2^-40 and 2^-16
            s_exp = st["k"]
            corners, member = sets[s_exp]
            if s_exp != 50:
                with torch.cuda.stream(side):
                    scene.refit(st["d_vd"], d_tv, normal_offset=6, stream_ptr=side.cuda_stream)
                side.synchronize()
            if s_exp == -16:
                check_forms(item_run(scene, st["queries"]), member, "after the device refit to 2^-16")
            assert np.array_equal(IR.walked(st["queries"]), walked)
            node_boxes = R.node_boxes(tree, corners)
            bmin, bmax = R.flat_boxes(tree, node_boxes)
            g = scene.geometry()
            assert np.array_equal(g["vertex_positions"].view(np.uint32), corners.reshape(-1).view(np.uint32)), s_exp
            assert np.array_equal(g["group_boxmin"].view(np.uint32), bmin.view(np.uint32)) and np.array_equal(g["group_boxmax"].view(np.uint32), bmax.view(np.uint32)), s_exp
            for any_only, k in ((False, 0), (False, 8), (True, 0)):
                want = IR.walk_counters(tree, node_boxes, corners, st["queries"], any_only=any_only, member=member)
                if not any_only and k == 0:              # does the cull reject anything at this magnitude?
                    everything = T * int(walked.sum())
                    tests = int(want["triangle_tests"].sum())
                    print(f"refit to 2^{s_exp}: the counting walk tests {tests} of {everything} pairs of a walked query and a triangle")
                    assert tests == everything if s_exp == -40 else tests < everything, (s_exp, tests, everything)
                for rows in (np.arange(64), np.arange(len(st["queries"]))):
                    _, _, c = scene.intersecting_triangles(st["queries"][rows], max_triangles=k, counters=True, any_only=any_only)
                    got = {key: c[key] for key in IR.COUNTERS}
                    assert got == {key: int(want[key][rows].sum()) for key in IR.COUNTERS}, (s_exp, any_only, k, len(rows))
                print(f"refit to 2^{s_exp}, {'ANY' if any_only else f'K = {k}'}: {got}")
    finally:
        scene.close()
        world.close()


@pytest.mark.parametrize("s_exp", [-64, 50])
def test_device_world_under_geometry_scale(pkg, gpu, worlds, s_exp):
    """the device-built scene of the same file at the same scale, through world.scene: the restatement on its own triangle order,
    and the host-built scene's counts (a count does not depend on the order)"""
    name = "lobed_528"
    before = os.environ.get("GEOMETRY_SCALE")
    os.environ["GEOMETRY_SCALE"] = X.scale_string(s_exp)
    try:
        dw = pkg.tracer.DeviceWorld(IC.scene_path(name))
    finally:
        if before is None:
            del os.environ["GEOMETRY_SCALE"]
        else:
            os.environ["GEOMETRY_SCALE"] = before
    try:
        positions = np.asarray(dw.flat_arrays()["vertex_positions"], F)
        assert np.array_equal(X.triangle_rows(positions), scaled_rows(pkg, name, s_exp))
        queries = SC.queries(pkg, name, s_exp)
        member = IR.intersects(queries, positions)
        check_forms(item_run(dw.scene, queries), member, f"DeviceWorld at 2^{s_exp}")
        _, scene = worlds(name, s_exp)
        assert_same(dw.scene.intersection_counts(queries), scene.intersection_counts(queries), f"DeviceWorld and the host-built scene at 2^{s_exp}")
        assert np.array_equal(member.sum(1), (SC.codes(pkg, name, s_exp) == IR.INTERSECT).sum(1))
    finally:
        dw.close()


def test_a_count_split_over_launches_at_a_scaled_cell(pkg, gpu, worlds):
    """test_gpu_intersect's test_a_count_split_over_launches on small_trisrc at 2^40 with K = 1 and counts, so that the indices'
    `out + index * k` carries an index past the first launch's 2^24; the filler is a far, walked triangle that meets nothing on
    the restatement"""
    import torch
    s_exp = 40
    positions, scene = worlds("small_trisrc", s_exp)
    n = (1 << 24) + 3000
    real = SC.scaled_queries(IC.make_queries(SC.as_dict(X.base_arrays(pkg, "small_trisrc")), 3000 + 4096, seed=33), s_exp)
    tail, spread = real[:3000], real[3000:]
    far = SC.scaled_queries(np.asarray([[(1e6, -2e6, 3e6), (1.5e6, -2e6, 3e6), (1e6, -1e6, 4e6)]], F), s_exp)
    assert IR.walked(far).all() and not IR.intersects(far, positions).any()
    d = device_triangles(far).repeat(n, 1)
    d[n - 3000:] = device_triangles(tail)
    sample = torch.from_numpy(np.random.default_rng(1).choice(n - 3000, 4096, replace=False)).cuda()
    d[sample] = device_triangles(spread)
    d_out = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    d_cnt = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    scene.intersecting_triangles_into(d.data_ptr(), n, d_out.data_ptr(), d_cnt.data_ptr(), max_triangles=1,
                                      stream_ptr=torch.cuda.current_stream().cuda_stream)
    torch.cuda.current_stream().synchronize()
    want, want_n = IR.intersect(real, positions, 1)
    assert (want_n[:3000] > 0).mean() > 0.3
    assert_same(d_out[n - 3000:].cpu().numpy().reshape(-1, 1), want[:3000], "the last launch's indices")
    assert_same(d_cnt[n - 3000:].cpu().numpy(), want_n[:3000], "the last launch's counts")
    assert_same(d_out[sample].cpu().numpy().reshape(-1, 1), want[3000:], "indices of the first launch")
    assert_same(d_cnt[sample].cpu().numpy(), want_n[3000:], "counts of the first launch")
    rest = torch.ones(n - 3000, dtype=torch.bool, device="cuda")
    rest[sample] = False
    assert bool((d_out[: n - 3000][rest] == -1).all())
    assert bool((d_cnt[: n - 3000][rest] == 0).all())


def test_minus_zero_queries_on_the_flat_lattice(pkg, gpu, tmp_path_factory):
    """the flat lattice's integer queries with the sign of every zero coordinate flipped to -0: the sets of the +0 queries (the
    header's == makes -0 equal +0), with and without SKIP_SHARED"""
    pos, scene = flat_scene(pkg, tmp_path_factory)
    queries, code, code_skip = flat_codes(pos)
    flipped = SC.minus_zero(queries)
    assert np.signbit(flipped[queries == 0]).all() and (queries == 0).mean() > 0.2
    assert np.array_equal(IR.first_axis(flipped, pos), code) and np.array_equal(IR.first_axis(flipped, pos, True), code_skip)
    check_forms(item_run(scene, flipped), code == IR.INTERSECT, "flat lattice, -0")
    check_forms(item_run(scene, flipped, True), code_skip == IR.INTERSECT, "flat lattice, -0, SKIP_SHARED", ks=(0, 4, 9))
