"""The CPU restatement of scene creation's derived arrays (tests/scene_ref.py) pinned to the reference's own dumps: every octant
copy decodes back to the reference's boxes and leaf ranges, and the child each copy names first is the hit link of the reference's
threaded table for that direction code.  The GPU suite compares the restatement with what both creation paths derive
(tests/test_gpu_scene_device.py)."""
import os

import numpy as np
import pytest

import refit_ref as R
import scene_ref as S

F, U32 = np.float32, np.uint32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SCENES = {"lobed_528": "lobed_528.trisrc", "quads_mixed": "quads_mixed.obj", "quads_nonormals": "quads_nonormals.obj"}


def bits(a):
    return np.ascontiguousarray(a, F).view(U32)


@pytest.mark.parametrize("name", list(SCENES))
def test_restated_records_decode_to_the_reference_dumps(pkg, name):
    world = pkg.World(os.path.join(GOLDEN, SCENES[name]))
    tree = R.TreeArrays.of(world.export_tree())
    mine = S.derived_arrays(tree, world.arrays())
    ref = dict(np.load(os.path.join(GOLDEN, name + ".ref.npz")))
    index = R.in_order_index(tree)                     # pre-order -> the reference's numbering
    n = tree.node_count
    assert n == int(ref["group_count"][0])
    leaf = tree.negative < 0
    bmin, bmax = ref["group_boxmin"].reshape(-1, 3)[index], ref["group_boxmax"].reshape(-1, 3)[index]
    objects = ref["group_objects"].reshape(-1, 2)[index]
    assert mine["packed_nodes"].shape == (8, n, 8)
    for o in range(8):
        copy = mine["packed_nodes"][o]
        enters_low = np.array([(o >> k) & 1 for k in range(3)], bool)
        entry, leave = copy[:, [0, 1, 4]].view(F), copy[:, [2, 3, 5]].view(F)
        assert np.array_equal(bits(np.where(enters_low, entry, leave)), bits(bmin)), (name, o)
        assert np.array_equal(bits(np.where(enters_low, leave, entry)), bits(bmax)), (name, o)
        assert np.array_equal(copy[leaf, 6], objects[leaf, 0].astype(U32)), (name, o)
        assert np.array_equal(copy[leaf, 7], S.LEAF_FLAG | objects[leaf, 1].astype(U32)), (name, o)
        # a branch names the child a ray of this octant visits first, then the other (name = pre-order index * 4)
        first, other = (copy[~leaf, 6] & 0x1fffffff) >> 2, copy[~leaf, 7] >> 2
        hit = ref[f"group_hitmiss_{o}"].reshape(-1, 2)[index[~leaf], 0]
        assert np.array_equal(index[first].astype(F), hit), (name, o)
        assert np.array_equal(np.sort([first, other], axis=0), np.sort([tree.negative[~leaf], tree.positive[~leaf]], axis=0))
        assert np.all(copy[~leaf, 6] >> 29 == 1 << S.split_axis(tree)[~leaf]), (name, o)   # the axis-hot bit
    # the pair records: each branch's children's boxes and links
    pairs, b = mine["pair_nodes"], np.nonzero(~leaf)[0]
    assert pairs.shape == (n, 16) and not pairs[leaf].any()
    for first, child in ((0, tree.negative[b]), (8, tree.positive[b])):
        assert np.array_equal(pairs[b, first:first + 3], bits(bmin[child])) and np.array_equal(pairs[b, first + 4:first + 7], bits(bmax[child]))
        assert np.array_equal(pairs[b, first + 3] & S.PAIR_INDEX_MASK, child)
        assert np.array_equal(pairs[b, first + 3] >> 31, leaf[child].astype(U32))
    # the packed triangles: v0 is the reference's first corner, and one spare record of zeros follows
    corners = ref["vertex_positions"].reshape(-1, 3, 3)
    tris = mine["packed_tris"]
    assert tris.shape == (len(corners) + 1, 9) and not tris[-1].any()
    assert np.array_equal(tris[:-1, 0:3], bits(corners[:, 0]))
    assert np.array_equal(tris[:-1, 3:6], bits(corners[:, 1] - corners[:, 0]))
    assert np.array_equal(mine["normals16"], S.half_bits(ref["vertex_normals"]))
    assert mine["stack_levels"] >= 3
    world.close()


def test_half_bits_round_to_nearest_even():
    """every non-NaN binary32 converts as numpy's correctly rounded float16 does; a NaN becomes the quiet 0x7e00 with its sign"""
    rng = np.random.default_rng(7)
    u = np.concatenate([rng.integers(0, 1 << 32, 1 << 20, dtype=np.uint64).astype(U32),
                        np.arange(0x33000000, 0x33800000, 97, dtype=U32),          # around the smallest half
                        np.arange(0x38000000, 0x39000000, 89, dtype=U32),          # subnormal -> normal halves
                        np.arange(0x477fe000, 0x47800100, 1, dtype=U32)])           # the overflow edge
    u = np.concatenate([u, u | 0x80000000])
    f = u.view(F)
    ok = ~np.isnan(f)
    with np.errstate(over="ignore"):
        assert np.array_equal(S.half_bits(f[ok]), f[ok].astype(np.float16).view(np.uint16))
    nan = np.array([0x7f800001, 0x7fc00000, 0xffffffff, 0xff812345], U32).view(F)
    assert S.half_bits(nan).tolist() == [0x7e00, 0x7e00, 0xfe00, 0xfe00]


def test_deepest_stack_by_hand():
    """a root split along x over a leaf (negative) and a branch split along y over two leaves (positive): a ray with D.x <= 0
    (code bit 0 clear) visits the root's positive child first and keeps the leaf pending, so at the branch it holds two far
    children"""
    deep = R.TreeArrays(np.array([-1, 0, 0, 2, 2], np.int32), np.array([1, -1, 3, -1, -1], np.int32), np.array([2, -1, 4, -1, -1], np.int32),
                        None, np.array([[1, 0, 0], [0, 0, 0], [0, 1, 0], [0, 0, 0], [0, 0, 0]], F), np.array([0, 0, 0, 1, 2], np.int32),
                        np.array([0, 1, 0, 1, 1], np.int32), np.zeros((3, 3), np.int32))
    assert S.deepest_stack(deep) == 2
    one_leaf = R.TreeArrays(np.array([-1], np.int32), np.array([-1], np.int32), np.array([-1], np.int32), None, np.zeros((1, 3), F),
                            np.array([0], np.int32), np.array([3], np.int32), np.zeros((3, 3), np.int32))
    assert S.deepest_stack(one_leaf) == 0
    assert S.derived_arrays(one_leaf, {"group_boxmin": np.zeros(3, F), "group_boxmax": np.ones(3, F),
                                       "vertex_positions": np.zeros(27, F), "vertex_normals": np.zeros(27, F)})["stack_levels"] == 3
