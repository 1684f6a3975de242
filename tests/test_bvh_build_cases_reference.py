"""The inputs of tests/bvh_build_cases.py on the CPU: the host builder (host/bvh.cpp), which tests/test_gpu_bvh_build_edges.py
holds the device builder to, equals the REFERENCE's make_bvh on every one of them -- against committed digests of the compiled
reference's dumps (tests/golden/bvh_build_cases.ref.npz, written by tests/golden/make_golden.py) and, where oracle/_ref/ref_host
is built, against a dump made now, which must equal the committed one.  The build parameters are read once per process by
both builders, so each option set gets a process of its own.  And every case is checked to be what it claims to be: a later
change to a generator must not empty a test without anyone noticing."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bvh_build_cases as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


@pytest.fixture(scope="module")
def cases(pkg, tmp_path_factory):
    return B.CaseSet(pkg, tmp_path_factory.mktemp("bvh_build_cases"))


@pytest.fixture(scope="module")
def fixture():
    return B.load_fixture()


@pytest.fixture(scope="module")
def trees(pkg, cases):
    """name -> HostTree of the host build under the default parameters, built once"""
    made = {}

    def get(name):
        if name not in made:
            world = pkg.World(cases.path(name))
            made[name] = B.HostTree(world)
            world.close()
        return made[name]
    return get


def assert_same_summary(got, want, what):
    assert got["scalars"] == want["scalars"], (what, dict(zip(B.FLAT_SCALARS, zip(got["scalars"], want["scalars"]))))
    assert got["sizes"] == want["sizes"], (what, got["sizes"], want["sizes"])
    differing = [k for k, a, b in zip(B.FLAT_ARRAYS, got["sha256"], want["sha256"]) if a != b]
    assert not differing, f"{what}: the bits of {differing} differ"


@pytest.mark.parametrize("name", B.NAMES)
def test_host_build_equals_the_reference(pkg, cases, fixture, name):
    path = cases.path(name)
    committed = fixture[("", name)]
    assert B.file_sha256(path) == committed["input_sha256"], f"{name} is not the file the committed dump was made from: run tests/golden/make_golden.py"
    world = pkg.World(path)
    mine = B.summary(world.arrays(), world.info.triangle_count)
    world.close()
    assert_same_summary(mine, committed, f"{name}: host build against the committed reference dump")
    if os.path.exists(B.REF_HOST):
        live = B.reference_summary(path)
        assert_same_summary(live, committed, f"{name}: the reference's dump made now against the committed one")
        assert_same_summary(mine, live, f"{name}: host build against the reference's dump made now")


CHILD = r'''
import json, sys
sys.path[:0] = [%r, %r]
from __graft_entry__ import load_package
import bvh_build_cases as B
pkg = load_package()
cases = B.CaseSet(pkg, %r)
out = {}
for name in B.OPTION_INPUTS:
    world = pkg.World(cases.path(name))
    tree = B.HostTree(world)
    out[name] = {"summary": B.summary(world.arrays(), world.info.triangle_count), "large_leaves": int(world.info.large_leaves),
                 "max_level": int(world.info.max_level), "node_count": int(world.info.node_count),
                 "leaves": [[int(c), int(l)] for c, l in zip(tree.triangles[tree.is_leaf], tree.level[tree.is_leaf])]}
    world.close()
print(json.dumps(out))
'''


@pytest.mark.parametrize("options", list(B.OPTION_SETS))
def test_host_build_equals_the_reference_under_each_option_set(cases, fixture, options):
    paths = {name: cases.path(name) for name in B.OPTION_INPUTS}
    env = {k: v for k, v in os.environ.items() if k not in ("BVH_MAX_DEPTH", "BVH_LEAF_MAX", "SAH_CTRAV", "SAH_CISEC")}
    env.update(B.option_environment(options))
    run = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests"), cases.directory)], env=env, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-3000:]
    host = json.loads(run.stdout.strip().splitlines()[-1])
    max_depth, leaf_max, _, _ = B.option_values(options)
    for name in B.OPTION_INPUTS:
        committed = fixture[(options, name)]
        assert_same_summary(host[name]["summary"], committed, f"{options}, {name}: host build against the committed reference dump")
        if os.path.exists(B.REF_HOST):
            live = B.reference_summary(paths[name], B.option_environment(options))
            assert_same_summary(live, committed, f"{options}, {name}: the reference's dump made now against the committed one")
        # what the set is there for
        leaves, triangles = host[name]["leaves"], committed["scalars"][B.FLAT_SCALARS.index("triangle_count")]
        assert sum(c for c, _ in leaves) == triangles and host[name]["max_level"] <= max_depth
        if options in ("max_depth_0", "leaf_max_m1"):
            assert leaves == [[triangles, 0]], (options, name)                      # the root is the only node,
            assert host[name]["large_leaves"] == 0                                   # and only "no split pays" counts as large
        # (sah_ctrav = 1e6 is on both sides of `cost < leaf cost`: it does not stop the splitting, it rounds both costs to
        # multiples of 1/16 and so makes ties between neighbouring planes, which the first bin wins)
        if options == "max_depth_1":
            assert host[name]["node_count"] == 3 and [l for _, l in leaves] == [1, 1]
        if options in ("leaf_max_0", "leaf_max_1"):
            # below the depth cap a leaf above leaf_max is one that no split beat; with leaf_max 0 that is every leaf
            assert host[name]["node_count"] > 1 and host[name]["max_level"] < max_depth
            assert host[name]["large_leaves"] == sum(1 for c, _ in leaves if c > leaf_max)
            assert options != "leaf_max_0" or host[name]["large_leaves"] == len(leaves)
    if options == "max_depth_4":
        # the depth cap makes leaves above leaf_max that are NOT large leaves: nothing asked whether a split would pay
        leaves = host["chain_x"]["leaves"]
        assert any(c > 10 and l == 4 for c, l in leaves), leaves
        assert host["chain_x"]["large_leaves"] == sum(1 for c, l in leaves if c > 10 and l < 4)


# ---- the cases are what they claim to be

def test_the_ladder_contains_both_transitions(trees):
    """On the small side the 1e-5 bump swamps the geometry, on the large side the root's area overflows: in both places the root
    stops splitting, and the ladder has two adjacent rungs on either side of each place (not hard-coded which)."""
    for family, exponents in (("cube", B.LADDER_EXPONENTS), ("slab", B.SLAB_EXPONENTS)):
        splits = [trees(f"ladder_{family}_{B._tag(e)}").root_split() is not None for e in exponents]
        steps = [(a, b) for a, b in zip(splits, splits[1:])]
        assert (True, False) in steps, (family, "no rung where the root stops splitting towards the large end", splits)
        if family == "cube":
            assert (False, True) in steps, (family, "no rung where the root starts splitting from the small end", splits)
            assert splits[exponents.index(0)]
    # the slab's root still splits where the cube's no longer does
    cube_last = max(e for e in B.LADDER_EXPONENTS if trees(f"ladder_cube_{B._tag(e)}").root_split() is not None)
    slab_last = max(e for e in B.SLAB_EXPONENTS if trees(f"ladder_slab_{B._tag(e)}").root_split() is not None)
    assert slab_last > cube_last


def test_the_poles_overflow_their_barycentres(cases, trees):
    """ladder_poles_inf: some barycentres are +inf while the root's hi - lo is finite: (b - lo) * bins / (hi - lo) is +inf for them;
    ladder_poles_nan: hi - lo overflows too, and the expression is NaN for every triangle (inf / inf).  Both roots stay leaves."""
    with np.errstate(over="ignore", invalid="ignore"):
        for name, finite in (("ladder_poles_inf", True), ("ladder_poles_nan", False)):
            tree, b = trees(name), B.barycentres(cases.corners(name))[:, 0]
            lo, hi = F(tree.box[0, 0]), F(tree.box[0, 3])
            scaled = (b - lo) * F(40) / (hi - lo)
            assert np.isfinite(cases.corners(name)).all() and np.isinf(b).any() and np.isfinite(b).any()
            assert tree.root_split() is None and tree.info.large_leaves == 1 and np.isfinite(hi - lo) == finite
            if finite:
                assert np.isposinf(scaled).any() and not np.isnan(scaled).any() and (scaled[np.isfinite(scaled)] < 1).all()
            else:
                assert np.isnan(scaled).all()


@pytest.mark.parametrize("name,tied", [("16x16x4", (0, 1)), ("8x8x8", (0, 1, 2)), ("4x16x16", (1, 2))])
def test_the_lattices_tie_the_axis_choice(cases, trees, name, tied):
    for order in B.ORDERS:
        b = B.barycentres(cases.corners(f"ties_{name}_{order}"))
        lo, hi = (b - F(1e-5)).min(axis=0), (b + F(1e-5)).max(axis=0)           # box3d::add(point)
        spread = np.maximum(F(0), hi - lo)
        assert spread.dtype == F and len({spread[k].tobytes() for k in tied}) == 1, (name, order, spread)
        assert all(spread[k] < spread[tied[0]] for k in range(3) if k not in tied)
        # x before y before z, and only a STRICTLY longer axis wins: x = y (or all three) tied gives... not x
        want = 1 if tied == (0, 1) else 2
        assert trees(f"ties_{name}_{order}").root_split()[0] == want, (name, order)


def test_the_bin_boundary_row_lies_on_bin_boundaries(cases, trees):
    tree = trees("ties_bin_boundary_row")
    b = B.barycentres(cases.corners("ties_bin_boundary_row"))[:, 0]
    lo, hi = F(tree.box[0, 0]), F(tree.box[0, 3])
    bins = min(40, 2 * len(b))
    scaled = (b - lo) * F(bins) / (hi - lo)                                      # bvh.cpp:153-170, in float32
    assert scaled.dtype == F and bins == 40 and np.array_equal(scaled, np.floor(scaled)) and len(set(scaled.tolist())) == len(b)
    # and the root's plane, lo + i * (hi - lo) / bins, is the barycentre of the first triangle that did not go below it
    axis, below = tree.root_split()
    planes = lo + np.arange(bins).astype(F) * (hi - lo) / F(bins)
    assert axis == 0 and np.sort(b)[below] in planes


def test_the_chains_are_deep(trees):
    for axis in "xyz":
        tree = trees(f"chain_{axis}")
        assert tree.info.max_level >= 16 and tree.root_split()[0] == "xyz".index(axis)


@pytest.mark.parametrize("name", B.FAMILIES["blocks"])
def test_the_blocks_retire_as_one_large_leaf(trees, name):
    tree = trees(name)
    d = int(name.split("block_")[1].split("_")[0])
    level = 2 if "inside" in name else 1
    at = np.nonzero(tree.is_leaf & (tree.triangles == d) & (tree.level == level))[0]
    assert len(at) == 1 and tree.info.large_leaves == 1, (name, at)
    # where the retired positions lie: in front when the block is on the -x side, behind when on the +x side
    start = int(tree.start[at[0]])
    total = len(tree.triangle_vertices)
    assert start == (0 if "_before_row" in name else 128 if "inside" in name else total - d), (name, start)


@pytest.mark.parametrize("base", B.PARTITION_BASES)
def test_the_partition_cases_misplace_what_they_say(cases, trees, base):
    total = len(cases.corners(base))
    for order in B.PARTITION_ORDERS:
        tree = trees(f"partition_{base}_{order}")
        assert tree.root_split() == trees(base).root_split()                    # the root's split does not depend on the order
        flags, mid = B.misplaced_at_root(tree)
        left, right = int((~flags[:mid]).sum()), int(flags[mid:].sum())         # belong right but lie left; belong left but lie right
        assert left == right
        pairs = min(mid, total - mid)
        if order == "ascending":
            assert left == 0
        elif order == "descending":
            assert left == pairs                                                  # every exchange there can be
        elif order == "two_ends":
            assert left == 1 and not flags[0] and flags[-1]
        else:
            assert not flags[0:2 * pairs:2].any() and flags[1:2 * pairs:2].all() and pairs // 2 <= left <= pairs


def test_the_duplicates_make_leaves_of_their_size(trees):
    for name, counts in [(f"duplicates_{n}", (n,)) for n in B.DUPLICATES] + [("duplicates_11_40_41", B.DUPLICATES)]:
        tree = trees(name)
        sizes = sorted(int(c) for c in tree.triangles[tree.is_leaf] if c > 10)
        assert sizes == sorted(counts) and tree.info.large_leaves == len(counts), (name, sizes)


def test_the_zeros_hold_zeros_of_both_signs(cases, trees):
    plain, scaled, shifted, planes = (cases.corners(n) for n in ("zeros", "zeros_scaled", "zeros_shifted", "zeros_on_planes"))
    for c in (plain, scaled):
        zero = c == 0
        assert zero.any() and np.signbit(c[zero]).any() and not np.signbit(c[zero]).all()
        assert all(zero[..., k].any() for k in range(3))
    # both signs survive the file's %.9g and the loader (which merges -0 with +0 only between otherwise equal vertices)
    for name in ("zeros", "zeros_scaled", "zeros_on_planes"):
        loaded = trees(name).vertex_data[:, :3]
        signs = np.signbit(loaded[loaded == 0])
        assert signs.any() and not signs.all(), name
    # corners at exactly +-1e-5f: c - 1e-5f and c + 1e-5f are zeros there, and +0 (x - x in round-to-nearest), on triangle boxes
    for c in (plain, planes):
        low, high = c - F(1e-5), c + F(1e-5)
        assert (low == 0).any() and (high == 0).any() and not np.signbit(low[low == 0]).any() and not np.signbit(high[high == 0]).any()
    # and on node boxes: with x >= 1e-5f and y <= -1e-5f the low x plane and the high y plane of the root, and of nodes below it,
    # are +0 -- the only zero a box plane can hold (the header of csrc/bvh_build.hip says why)
    assert planes[..., 0].min() == F(1e-5) and planes[..., 1].max() == F(-1e-5)
    tree = trees("zeros_on_planes")
    for column in (0, 4):                                      # min x, max y
        plane = tree.box[:, column]
        assert plane[0] == 0 and int((plane == 0).sum()) > 1 and len(plane) > 1 and not np.signbit(plane[plane == 0]).any()
    for name in ("zeros", "zeros_scaled", "zeros_shifted", "zeros_on_planes"):
        box = trees(name).box
        assert not np.signbit(box[box == 0]).any(), name
    # where the bump is absorbed
    for c in (scaled[scaled != 0], shifted):
        assert np.abs(c).min() >= 512 and np.array_equal(c - F(1e-5), c) and np.array_equal(c + F(1e-5), c)


def test_the_case_lists_are_complete():
    assert len(set(B.NAMES)) == len(B.NAMES) and set(B.PIPELINE_NAMES) <= set(B.NAMES) and set(B.FRAME_NAMES) <= set(B.PIPELINE_NAMES)
    assert set(B.OPTION_INPUTS) <= set(B.NAMES)
    assert len(B.FAMILIES["ladder"]) == 21 and len(B.FAMILIES["ties"]) == 10 and len(B.FAMILIES["rows"]) == 10
    assert len(B.FAMILIES["blocks"]) == 33 and len(B.FAMILIES["partition"]) == 8 and len(B.FAMILIES["chain"]) == 3 and len(B.FAMILIES["zeros"]) == 4
    assert sorted(B.fixture_keys()) == sorted(B.load_fixture())
