"""The CPU restatement of the refit (tests/refit_ref.py) pinned to the trees the package builds and to the reference's own
dumps: with the vertices unmoved, the restated boxes are World.export_tree()'s node boxes and the reference's group_boxmin /
group_boxmax bit for bit.  Also: libshray_refit.so exports what include/shader_ray_refit.h declares, and the ctypes mirror of
its structures has the header's layout."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import helpers
import refit_ref as R
from refdump import bits_sha256

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SCENES = {"lobed_528": "lobed_528.trisrc", "quads_mixed": "quads_mixed.obj", "quads_nonormals": "quads_nonormals.obj"}


def scene_path(name):
    return helpers.bunny_trisrc() if name == "bunny" else os.path.join(GOLDEN, SCENES[name])


def tree_and_corners(pkg, path):
    world = pkg.World(path)
    desc = world.export_tree()
    tree = R.TreeArrays.of(desc)
    vd = np.ctypeslib.as_array(desc.vertex_data, shape=(desc.vertex_count * 9,)).reshape(-1, 9).copy()
    return world, tree, vd, vd[tree.triangle_vertices][:, :, :3]


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.mark.parametrize("name", list(SCENES) + ["bunny"])
def test_restated_boxes_are_the_built_trees(pkg, name):
    world, tree, _, corners = tree_and_corners(pkg, scene_path(name))
    boxes = R.node_boxes(tree, corners)
    assert np.array_equal(bits(boxes), bits(tree.box)), f"{name}: {int((bits(boxes) != bits(tree.box)).sum())} words differ"
    flat = world.arrays()
    bmin, bmax = R.flat_boxes(tree, boxes)
    assert np.array_equal(bits(bmin), bits(flat["group_boxmin"])) and np.array_equal(bits(bmax), bits(flat["group_boxmax"]))
    assert R.exact_div_ok(boxes)
    assert R.sah_cost(tree, boxes) > 0
    world.close()


@pytest.mark.parametrize("name", ["lobed_528", "quads_mixed", "quads_nonormals", "bunny"])
def test_restated_boxes_are_the_reference_dumps(pkg, name):
    path = scene_path(name)
    world, tree, _, corners = tree_and_corners(pkg, path)
    bmin, bmax = R.flat_boxes(tree, R.node_boxes(tree, corners))
    ref = dict(np.load(os.path.join(GOLDEN, "bunny_class_132x264.ref.npz" if name == "bunny" else os.path.splitext(SCENES[name])[0] + ".ref.npz")))
    for key, mine in (("group_boxmin", bmin), ("group_boxmax", bmax)):
        if key + ".sha256" in ref:        # the bunny-class fixture keeps the digest of the array's bits
            assert bits_sha256(mine) == str(ref[key + ".sha256"]), key
        else:
            assert np.array_equal(bits(mine), bits(ref[key])), key
    world.close()


def test_sah_cost_by_hand():
    """a root over two leaves of 1 and 3 triangles: 1 + 4 (area(a) + 3 area(b)) / area(root)"""
    tree = R.TreeArrays(np.array([-1, 0, 0], np.int32), np.array([1, -1, -1], np.int32), np.array([2, -1, -1], np.int32),
                        None, np.zeros((3, 3), F), np.array([0, 0, 1], np.int32), np.array([4, 1, 3], np.int32), np.zeros((4, 3), np.int32))
    boxes = np.array([[0, 0, 0, 2, 1, 1], [0, 0, 0, 1, 1, 1], [1, 0, 0, 2, 1, 0.5]], F)
    area = [2 * (2 + 2 + 1), 6, 2 * (1 + 0.5 + 0.5)]
    assert R.sah_cost(tree, boxes) == pytest.approx(1 + 4 * (area[1] + 3 * area[2]) / area[0], rel=1e-15)
    flat = boxes.copy()
    flat[:, 3:] = flat[:, :3]                # zero-length diagonals
    assert R.sah_cost(tree, flat) == 0.0
    empty = np.array([[R.FLT_MAX] * 3 + [-R.FLT_MAX] * 3], F)
    assert R.box_area(empty)[0] == 0.0       # box3d::dim clamps an inverted box at 0


def test_exact_div_flag_by_hand():
    assert R.exact_div_ok(np.array([[0, -1e-20, 1, 2.0 ** 59, 3, 4]], F))
    assert not R.exact_div_ok(np.array([[0, 0, 0, 2.0 ** 60, 1, 1]], F))
    assert not R.exact_div_ok(np.array([[1e-30, 0, 0, 1, 1, 1]], F))


def test_a_moved_leaf_moves_its_ancestors_only(pkg):
    _, tree, _, corners = tree_and_corners(pkg, scene_path("lobed_528"))
    moved = corners.copy()
    leaf = int(np.nonzero(tree.negative < 0)[0][3])
    s, c = int(tree.start[leaf]), int(tree.triangles[leaf])
    moved[s:s + c] += F(0.25)
    before, after = R.node_boxes(tree, corners), R.node_boxes(tree, moved)
    changed = set(np.nonzero(np.any(bits(before) != bits(after), axis=1))[0].tolist())
    ancestors = {leaf}
    k = leaf
    while tree.parent[k] >= 0:
        k = int(tree.parent[k])
        ancestors.add(k)
    assert leaf in changed and changed <= ancestors


def declared_functions(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(shray_\w+)\s*\(", text)))


def test_refit_library_exports_every_declared_symbol(pkg):
    lib = pkg._native.load_refit()
    names = declared_functions("shader_ray_refit.h")
    assert len(names) == 4
    for name in names:
        assert hasattr(lib, name), f"libshray_refit.so does not export {name}"
    assert sorted(n for n, _, _ in pkg._native.REFIT_SYMBOLS) == names


def test_refit_struct_layouts_match_the_header(pkg, tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "shader_ray_refit.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(shray_refit_input), offsetof(shray_refit_input, normal_offset_floats),
         offsetof(shray_refit_input, vertex_data), offsetof(shray_refit_input, triangle_vertices), sizeof(shray_refit_stats),
         offsetof(shray_refit_stats, sah_cost), offsetof(shray_refit_stats, exact_div_ok), offsetof(shray_refit_stats, reserved));
  return 0; }''')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    N = pkg._native
    assert out == [C.sizeof(N.RefitInput), N.RefitInput.normal_offset_floats.offset, N.RefitInput.vertex_data.offset,
                   N.RefitInput.triangle_vertices.offset, C.sizeof(N.RefitStats), N.RefitStats.sah_cost.offset,
                   N.RefitStats.exact_div_ok.offset, N.RefitStats.reserved.offset]


def test_without_a_gpu_the_refit_fails_loudly_not_fatally(pkg):
    """argument errors come back as codes before any device work (a NULL scene, a NULL input)"""
    N = pkg._native
    lib = N.load_refit()
    inp = N.RefitInput()
    inp.struct_size = C.sizeof(N.RefitInput)
    assert lib.shray_scene_refit(None, C.byref(inp), None) != 0
    assert lib.shray_scene_refit_device(None, None, None, None) != 0
    assert lib.shray_scene_geometry_download(None, None, None, None, None) != 0
