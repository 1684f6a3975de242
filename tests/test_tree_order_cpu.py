"""CPU test of csrc/tree_order.h, the packed tree's topology in height order that the refit, the winding-number derivation and
the one-lane walks share: tests/native_tree_order.cpp builds DeviceNode arrays by hand in both octant conventions (copy 0: a'
names the positive child; copy 7: the negative) and checks the result against a plain recursive height computation -- order is
a permutation along which heights ascend, every branch sits one above its taller child, height_start brackets each height,
both conventions give the same Topo, tail_height and the bottom-up schedule follow the widths -- on a single leaf, three
nodes, one-sided chains 130 edges deep, a complete tree of 4096 leaves (tail_height 2) and seeded random trees; and that each
kind of malformed tree is refused."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "shader-ray_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("tree_order") / "native_tree_order")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", CSRC, "-o", path, os.path.join(HERE, "native_tree_order.cpp")],
                   check=True)
    return path


def run(exe, *args):
    out = subprocess.run([exe, *args], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout[-4000:] + out.stderr[-2000:]


def test_the_named_shapes(exe):
    run(exe, "shapes")


def test_the_shapes_at_the_schedules_edges(exe):
    """tests/tree_shapes.py's one_branch, tail_full, wide_by_one, two_wide, lopsided and mixed_spine, built by the program itself:
    leaves, tallest, tail_height and exactly the wide and tail calls for_each_level makes for a tail of 1024 threads"""
    run(exe, "edges")


@pytest.mark.parametrize("seed", [1, 77, 2024])
def test_seeded_random_trees(exe, seed):
    run(exe, "random", str(seed), "120")


def test_malformed_trees_are_refused(exe):
    run(exe, "refusals")
