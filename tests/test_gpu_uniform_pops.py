"""The uniform tails of the scheduled node stage (csrc/visit_asm.h, SHRAY_VISIT_POPS): a turn whose walking lanes are all at one
record and that no lane enters is the pop alone; one that every lane enters at a leaf's record is the park alone; and, in the
-DSHRAY_VISIT_POPS=2 build, the pop directly after a uniform run's push takes the pushed word from a scalar register (the mirror)
instead of the lanes' stacks.  The scenes are shaped for all three; which of them a library has is its build's choice.

Hand-built trees whose shape dictates the walk: every frame is compared bit for bit with the CPU oracle AND with kernel 1 (the
literal threaded kernel), through the three timed forms of kernel 0 -- one, two and four frames per launch -- and its counting
twin, whose tallies must be the oracle's (test_gpu_uniform_leaf.check_every_form).  Each case also renders one traversal per
pixel (material 0, one bounce) and asserts that the oracle's node_visits / leaf_visits are what the tree's shape dictates for
the rays inside the root box, so the scene provably walks the intended path.

The trees.  `chain` branches split on z enclose the node under test: a ray's D.z is negative in every view here, so each
branch's first child is its POSITIVE child (thread_tree) -- the next node of the chain --, and every lane of every wave enters
it: uniform every-lane-enters turns, a run, the push of the negative child (an empty leaf far outside the view, missed when it
is popped at the end).  The node under test is a branch split on x with one child outside the view and one that fills it; which
of them is visited first depends on the sign of D.x alone, and the views are rotated about y by +-30 degrees around a 40 degree
field of view, so that D.x has ONE sign over the whole frame: the same scene is walked "missed child first" (push, then the
mirrored pop of what was pushed) from one side and "filling child first" from the other.  The statement makes four turns per
evaluation of its exit tests: chains of 0 to 5 put the push on each of the four turns, and with 3 the mirrored pop would lie
across the exit tests (it goes through LDS there)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import HandScene, default_params
from test_gpu_uniform_leaf import bits, check_every_form, stacked

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = {value: os.path.join(ROOT, "shader-ray_amd", "_variants", f"libshray_hip_pops{value}.so") for value in (0, 1, 2)}

FILLS = ([-40, -40, -2], [40, 40, 1])             # a box every ray of every view here crosses
OFF = {+1: ([10, -40, -2], [20, 40, 1]),          # boxes no ray of any view here meets (the views see |x| < 5 between z = -2 and 1)
       -1: ([-20, -40, -2], [-10, 40, 1])}
FAR_OFF = ([-40, 60, -2], [40, 70, 1])
MATERIALS = ((0, 1), (6, 2))


class Tree:
    """Nodes added one by one; leaves hold triangle ranges of one shared list."""

    def __init__(self):
        self.neg, self.pos, self.axis, self.lo, self.hi, self.objects, self.tris = [], [], [], [], [], [], []

    def node(self, box, axis=0, tris=None):
        self.neg.append(-1)
        self.pos.append(-1)
        self.axis.append(axis)
        self.lo.append(box[0])
        self.hi.append(box[1])
        self.objects.append([len(self.tris), len(tris)] if tris else [0, 0])
        self.tris += list(tris or [])
        return len(self.neg) - 1

    def branch(self, box, axis, neg, pos):
        g = self.node(box, axis)
        self.neg[g], self.pos[g] = neg, pos
        return g

    def scene(self, root):
        import test_oracle_kat as kat
        tris = self.tris or [[[100, 100, 100], [101, 100, 100], [100, 101, 100]]]
        pts = np.asarray(tris, dtype=np.float32).reshape(-1, 3)
        normals = np.tile(np.asarray([0, 0, 1], np.float32), (len(pts), 1))
        hm = kat.thread_tree(self.neg, self.pos, self.axis, root)
        return HandScene(pts, normals, self.lo, self.hi, hm, self.objects, root)


def under_a_chain(tree, node, chain):
    """`node` under `chain` all-enter branches split on z: node = the positive (first-visited) child of the innermost."""
    for _ in range(chain):
        node = tree.branch(FILLS, 2, tree.node(FAR_OFF), node)
    return node


def missed_and_filling(chain, missed_side, missed="leaf", filling="leaf", filling_tris=3):
    """The node under test: a branch split on x whose child on `missed_side` (+1: the positive child) lies outside the view --
    an empty leaf, or a branch of two such leaves -- and whose other child fills the view: a leaf of `filling_tris` triangles, or
    `filling` = "missed": a second box outside the view.  Returns (scene, node visits per ray, leaf visits per ray)."""
    t = Tree()
    if missed == "leaf":
        out = t.node(OFF[missed_side])
    else:
        out = t.branch(OFF[missed_side], 1, t.node(OFF[missed_side]), t.node(OFF[missed_side]))
    other = t.node(FILLS, tris=stacked(filling_tris)) if filling == "leaf" else t.node(OFF[-missed_side])
    test = t.branch(FILLS, 0, *((other, out) if missed_side > 0 else (out, other)))
    root = under_a_chain(t, test, chain)
    # the chain's branches and their far children; the node under test, its two children (a missed branch's children are never visited)
    return t.scene(root), 2 * chain + 3, chain + 1 + (missed == "leaf")


def rotated(pkg, W, H, turn, material=0, degrees=30.0, zoom=4.0):
    """default_params' camera turned about y around the origin: it looks along (-sin, 0, -cos), so for turn = +1 every ray's D.x
    is negative (|eye.x| <= tan 20 < tan 30) and a branch split on x visits its POSITIVE child first; turn = -1: the negative one."""
    p = default_params(pkg, W, H, zoom=zoom, material=material)
    a = np.float32(np.radians(degrees) * turn)
    c, s = float(np.cos(a)), float(np.sin(a))
    for m in (p.camera_matrix, p.camera_normal_matrix):
        m[0], m[2], m[8], m[10] = c, -s, s, c
    p.camera_matrix[12], p.camera_matrix[14] = zoom * s, zoom * c
    right, up = p.right[0], p.up[1]
    p.right[0], p.right[2] = right * c, -right * s
    p.up[1] = up
    return p


def one_traversal(params):
    params.bounce_count = 1
    return params


def check(pkg, oracle_mod, hand, env, make_params, W, H, what, visits=None, leaves=None, inside=None):
    """Both materials through every form; then one traversal per pixel, whose tallies the tree's shape dictates."""
    for material, spp in MATERIALS:
        check_every_form(pkg, oracle_mod, hand, env, make_params(material), W, H, spp, f"{what}, material {material}")
    _, cpu = check_every_form(pkg, oracle_mod, hand, env, one_traversal(make_params(0)), W, H, 1, f"{what}, one traversal")
    assert cpu["traversals"] == W * H, (what, cpu)
    if visits is not None:
        inside = W * H if inside is None else inside
        assert cpu["node_visits"] == (W * H - inside) + visits * inside, (what, cpu)
        assert cpu["leaf_visits"] == leaves * inside, (what, cpu)
    return cpu


def first_child_is_the_missed_one(pkg, oracle_mod, hand, env, params, W, H, chain):
    """With the cap at the visit of the node under test's first child, a ray tests triangles only if that child is the filling
    leaf: the order of the two children, which no tally of an uncapped frame shows."""
    p = one_traversal(params)
    p.max_bvh_iterations = chain + 2
    _, cpu = oracle_mod.render(hand.desc, env, p, W, H, 1)
    return cpu["triangle_tests"] == 0


@pytest.fixture(scope="module")
def env(pkg):
    return pkg.scenes.environment_constant((0.5, 0.25, 2.0))


@pytest.mark.parametrize("missed_side", [+1, -1])
def test_first_child_missed_second_a_leaf(pkg, gpu, oracle_mod, env, missed_side):
    """Root split on x: the push of the filling leaf, the first child missed by every lane -- the mirrored pop --, then every lane
    enters the leaf.  From the other side the same scene is the leaf first and the missed child popped from LDS.  Either child
    word is the pushed one (missed_side)."""
    W, H = 64, 32
    hand, visits, leaves = missed_and_filling(0, missed_side)
    for turn in (+1, -1):
        first = first_child_is_the_missed_one(pkg, oracle_mod, hand, env, rotated(pkg, W, H, turn), W, H, 0)
        assert first == (turn == missed_side), (missed_side, turn)       # D.x < 0 (turn +1): the positive child first
        check(pkg, oracle_mod, hand, env, lambda m: rotated(pkg, W, H, turn, m), W, H, f"side {missed_side} turn {turn}", visits, leaves)


@pytest.mark.parametrize("chain", [1, 2, 3, 4, 5])
def test_under_chains_of_all_enter_branches(pkg, gpu, oracle_mod, env, chain):
    """The same under 1 to 5 enclosing all-enter branches: the push lands on turn chain % 4 of the four unrolled turns; with 3 the
    pop after it is the first turn after the exit tests.  The missed child once a leaf, once a branch (its record's second word
    has no leaf flag).  After the leaf stage the chain's far children come off the stacks through LDS, one after the other."""
    W, H = 64, 32
    for missed in ("leaf", "branch"):
        hand, visits, leaves = missed_and_filling(chain, +1, missed=missed)
        assert first_child_is_the_missed_one(pkg, oracle_mod, hand, env, rotated(pkg, W, H, +1), W, H, chain)
        check(pkg, oracle_mod, hand, env, lambda m: rotated(pkg, W, H, +1, m), W, H, f"chain {chain}, missed {missed}", visits, leaves)
    hand, visits, leaves = missed_and_filling(chain, -1)
    assert not first_child_is_the_missed_one(pkg, oracle_mod, hand, env, rotated(pkg, W, H, +1), W, H, chain)
    check(pkg, oracle_mod, hand, env, lambda m: rotated(pkg, W, H, +1, m), W, H, f"chain {chain}, the leaf first", visits, leaves)


def test_the_popped_sibling_is_missed_too(pkg, gpu, oracle_mod, env):
    """Both children outside the view: the mirrored pop, then a second pop.  With nothing below, the stacks are empty and every lane
    ends; under one enclosing branch the second pop reads LDS and must find that branch's other child -- here a leaf that fills
    the view, so the frame shows that it was reached."""
    W, H = 64, 32
    hand, visits, leaves = missed_and_filling(0, +1, filling="missed")
    cpu = check(pkg, oracle_mod, hand, env, lambda m: rotated(pkg, W, H, +1, m), W, H, "both missed, stack empty", visits, 2)
    assert cpu["triangle_tests"] == 0
    t = Tree()
    test = t.branch(FILLS, 0, t.node(OFF[-1]), t.node(OFF[+1]))
    below = t.node(FILLS, tris=stacked(3))
    root = t.branch(FILLS, 2, below, test)
    for turn in (+1, -1):
        cpu = check(pkg, oracle_mod, t.scene(root), env, lambda m: rotated(pkg, W, H, turn, m), W, H, f"both missed, turn {turn}", 5, 3)
        assert cpu["triangle_tests"] >= 3 * W * H


def mixed_scene():
    """A root whose silhouette cuts through 8 x 8 wave tiles (lanes that never walk), split on z: first an all-enter branch with
    the root's box -- a run's push after a mixed turn --, split on x into two leaves whose boxes' edges cut through tiles as well:
    waves in which no lane, some lanes and every lane enter the first child, side by side."""
    t = Tree()
    box = ([-1.1, -0.5, -1.0], [0.9, 0.45, 0.0])
    left = [[[-1.2, -0.6, z], [0.4, -0.6, z], [-0.4, 0.6, z]] for z in (-0.5, -0.2, -0.8)]
    right = [[[-0.5, -0.6, z], [1.0, -0.6, z], [0.3, 0.6, z]] for z in (-0.3, -0.6, -0.1, -0.9)]
    neg = t.node(([-1.1, -0.5, -1.0], [0.3, 0.45, 0.0]), tris=left)
    pos = t.node(([-0.4, -0.5, -1.0], [0.9, 0.45, 0.0]), tris=right)
    inner = t.branch(box, 0, neg, pos)
    root = t.branch(box, 2, t.node(FAR_OFF), inner)
    return t.scene(root)


@pytest.mark.parametrize("size", [(64, 32), (63, 31)])
def test_mixed_waves(pkg, gpu, oracle_mod, env, size):
    """Axis-aligned views: D.x changes sign at the frame's centre, so the first child is the positive leaf in the left half and
    the negative one in the right half.  At 63 x 31 the centre column and row have a direction component that is exactly zero: those
    lanes divide, and every turn of their waves -- the one after a run's push too -- is made by the compiler's visit; on return
    neither the run nor the mirror may survive.  A ray inside the root box visits root, inner branch, both leaves and the far leaf."""
    W, H = size
    hand = mixed_scene()
    for zoom in (4.0, 3.1):
        cpu = check(pkg, oracle_mod, hand, env, lambda m: default_params(pkg, W, H, zoom=zoom, material=m), W, H, f"mixed {size} {zoom}")
        inside, rest = divmod(cpu["node_visits"] - W * H, 4)
        assert rest == 0 and 0 < inside < W * H and cpu["leaf_visits"] == 3 * inside, (size, zoom, cpu)


def test_zero_direction_component_in_a_run(pkg, gpu, oracle_mod, env):
    """The chain scenes in an axis-aligned 63 x 31 view: the left half walks missed child first, the right half leaf first, and the
    waves of the centre column and row leave the statement at every turn."""
    W, H = 63, 31
    for chain in (0, 2, 3):
        hand, visits, leaves = missed_and_filling(chain, +1)
        check(pkg, oracle_mod, hand, env, lambda m: default_params(pkg, W, H, material=m), W, H, f"axis-aligned, chain {chain}", visits, leaves)


@pytest.mark.parametrize("chain", [1, 3])
def test_iteration_cap_around_the_mirrored_pop(pkg, gpu, oracle_mod, env, chain):
    """max_bvh_iterations at the visit whose tail is the mirrored pop (the missed first child: visit chain + 2), one less and one
    more: the marker colour and the tallies are the oracle's (check_every_form asserts both, the counting twin's included)."""
    W, H = 64, 32
    hand, visits, _ = missed_and_filling(chain, +1)
    for cap in (chain + 1, chain + 2, chain + 3, visits - 1, visits):
        for material, spp in MATERIALS:
            params = rotated(pkg, W, H, +1, material)
            params.max_bvh_iterations = cap
            want, cpu = check_every_form(pkg, oracle_mod, hand, env, params, W, H, spp, f"chain {chain}, cap {cap}, material {material}")
            if material == 0 and cap < visits:
                assert np.array_equal(bits(want), bits(np.broadcast_to(want[0, 0], want.shape))), (chain, cap)    # the marker, everywhere


@pytest.mark.parametrize("count", [0, 1, 10])
def test_every_lane_enters_one_leaf_from_inside_a_run(pkg, gpu, oracle_mod, env, count):
    """One leaf that fills the view under two all-enter branches: the park alone, from inside a run.  A leaf without triangles is
    handed to the compiler's visit."""
    W, H = 48, 32
    t = Tree()
    root = under_a_chain(t, t.node(FILLS, tris=stacked(count)), 2)
    for turn in (0, +1):
        make = (lambda m: default_params(pkg, W, H, material=m)) if turn == 0 else (lambda m: rotated(pkg, W, H, turn, m))
        cpu = check(pkg, oracle_mod, t.scene(root), env, make, W, H, f"{count} triangles, turn {turn}", 5, 3)
        assert cpu["triangle_tests"] == count * W * H


CHILD = r"""
import sys, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from __graft_entry__ import load_package
import bench
pkg = load_package()
world = pkg.World(pkg.scenes.bunny_trisrc())
scene = pkg.Scene(world.flatten(), pkg.scenes.environment_hdr_sky(2048), device=0)
scene.set_kernel(0)
orbit = bench.orbit_params(pkg, world, 256, 144)[:4]
out = torch.zeros(4, 144, 256, 4, dtype=torch.float32, device="cuda")
scene.render_batch_into(orbit, 256, 144, 1, out.data_ptr(), 144 * 256 * 16, torch.cuda.current_stream().cuda_stream)
torch.cuda.synchronize()
torch.save(out.cpu(), sys.argv[2])
scene.close()
print("views written")
"""


def test_the_headline_scene_against_the_builds_without(pkg, gpu, tmp_path):
    """The headline scene at 256 x 144, four frames per launch: this library against the -DSHRAY_VISIT_POPS=0, =1 and =2 builds
    (make -C shader-ray_amd variant VARIANT=pops0 HIP_EXTRA=-DSHRAY_VISIT_POPS=0, likewise pops1 and pops2), where they have been
    built: one of them is the default's own code, the others are the A/B builds."""
    built = {value: path for value, path in VARIANTS.items() if os.path.exists(path)}
    if not built:
        pytest.skip("no SHRAY_VISIT_POPS variant is built")
    import torch
    import bench
    world = pkg.World(pkg.scenes.bunny_trisrc())
    scene = pkg.Scene(world.flatten(), pkg.scenes.environment_hdr_sky(2048), device=0)
    try:
        scene.set_kernel(0)
        orbit = bench.orbit_params(pkg, world, 256, 144)[:4]
        out = torch.zeros(4, 144, 256, 4, dtype=torch.float32, device="cuda")
        scene.render_batch_into(orbit, 256, 144, 1, out.data_ptr(), 144 * 256 * 16, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        ours = out.cpu()
    finally:
        scene.close()
    assert float(ours[..., :3].std()) > 0.01         # (a picture, not a constant)
    for value, path in built.items():
        views = os.path.join(str(tmp_path), f"views_{value}.pt")
        run = subprocess.run([sys.executable, "-c", CHILD, ROOT, views], env=dict(os.environ, SHRAY_HIP_LIB=path),
                             capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert run.returncode == 0 and "views written" in run.stdout, (run.stdout + run.stderr)[-3000:]
        theirs = torch.load(views)
        os.remove(views)
        assert torch.equal(ours.view(torch.int32), theirs.view(torch.int32)), f"SHRAY_VISIT_POPS={value}: frames differ"
