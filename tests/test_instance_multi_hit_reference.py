"""The CPU restatement of the instanced all-hits ray query (tests/instance_multi_hit_ref.py) pinned to analytic answers: two
copies of a stack of squares interleave by t with their instances, an exact duplicate gives pairs of equal t with the lower
instance first (an odd K cuts a pair), tmax between and exactly at a layer, a tmax that is not positive, and a one-instance
identity set is the all-hits restatement itself."""
import numpy as np
import pytest

import instance_multi_hit_ref as IM
import multi_hit_ref as M
import ray_query_ref as R
from test_gpu_ray_query import random_rays

F = np.float32
MISS = R.HIT_MISS
EYE = np.eye(3, 4, dtype=F)


def shifted(dz):
    m = EYE.copy()
    m[2, 3] = -dz          # world to object: the copy sits dz higher in the world
    return m


@pytest.fixture(scope="module")
def stack(pkg, tmp_path_factory):
    world = pkg.World(M.write_mesh(pkg, str(tmp_path_factory.mktemp("instance_multihit") / "stack.trisrc"), "stack_of_squares"))
    arrays = R.SceneArrays(world.arrays())
    world.close()
    return arrays


def one_ray(scenes, W, origin, direction, tmax=1e7, **kw):
    hits, inst, counts, _ = IM.all_hits(scenes, W, [origin], [direction], [tmax], **kw)
    return hits[0], inst[0], int(counts[0])


def test_two_copies_interleave_by_t(stack):
    # the second copy half a layer up: squares at z = 0, 0.5, 1, 1.5, ... seen from z = -2, off the diagonal (one triangle each)
    W = np.stack([EYE, shifted(0.5)])
    h, i, n = one_ray([stack, stack], W, (0.25, -0.5, -2.0), (0.0, 0.0, 1.0), max_hits=12)
    assert n == 10
    assert h["t"][:10].tolist() == [2.0, 2.5, 3.0, 3.5, 4.0, 4.5, 5.0, 5.5, 6.0, 6.5]
    assert i.tolist() == [0, 1] * 5 + [-1, -1]
    assert h["triangle"][:10].tolist() == [0, 0, 2, 2, 4, 4, 6, 6, 8, 8]
    assert (h["triangle"][10:] == MISS).all() and (h["t"][10:] == F(1e7)).all() and (h["u"][10:] == 0).all() and (h["v"][10:] == 0).all()
    # the order of the instances in the set is the order of their indices only: swapped maps, swapped indices
    h2, i2, n2 = one_ray([stack, stack], W[::-1], (0.25, -0.5, -2.0), (0.0, 0.0, 1.0), max_hits=12)
    assert n2 == 10 and np.array_equal(h2, h) and i2.tolist() == [1, 0] * 5 + [-1, -1]
    # from above, the other side of the diagonal
    h, i, n = one_ray([stack, stack], W, (-0.5, 0.25, 5.0), (0.0, 0.0, -1.0), max_hits=3)
    assert n == 10 and h["t"].tolist() == [0.5, 1.0, 1.5] and i.tolist() == [1, 0, 1] and h["triangle"].tolist() == [9, 9, 7]


def test_an_exact_duplicate_gives_pairs_with_the_lower_instance_first(stack):
    W = np.stack([EYE, EYE])
    h, i, n = one_ray([stack, stack], W, (0.25, -0.5, -2.0), (0.0, 0.0, 1.0), max_hits=10)
    assert n == 10
    assert h["t"].tolist() == [2.0, 2.0, 3.0, 3.0, 4.0, 4.0, 5.0, 5.0, 6.0, 6.0]
    assert i.tolist() == [0, 1] * 5 and h["triangle"].tolist() == [0, 0, 2, 2, 4, 4, 6, 6, 8, 8]
    assert np.array_equal(h[0::2], h[1::2])                    # the same record twice
    # an odd K cuts a pair: the lower instance stays
    h, i, n = one_ray([stack, stack], W, (0.25, -0.5, -2.0), (0.0, 0.0, 1.0), max_hits=3)
    assert n == 10 and h["t"].tolist() == [2.0, 2.0, 3.0] and i.tolist() == [0, 1, 0]
    h, i, n = one_ray([stack, stack], W, (0.25, -0.5, -2.0), (0.0, 0.0, 1.0), max_hits=1)
    assert n == 10 and i.tolist() == [0] and h["triangle"].tolist() == [0]
    # on the diagonal x = y both triangles of a square are crossed: the instance sorts before the triangle
    h, i, n = one_ray([stack, stack], W, (0.25, 0.25, -2.0), (0.0, 0.0, 1.0), max_hits=4)
    assert n == 20 and h["t"].tolist() == [2.0] * 4 and i.tolist() == [0, 0, 1, 1] and h["triangle"].tolist() == [0, 1, 0, 1]


def test_tmax_cuts_the_union_and_excludes_a_hit_at_tmax(stack):
    W = np.stack([EYE, shifted(0.5)])
    h, i, n = one_ray([stack, stack], W, (0.25, -0.5, -2.0), (0.0, 0.0, 1.0), tmax=3.25, max_hits=4)   # between layers
    assert n == 3 and h["t"].tolist() == [2.0, 2.5, 3.0, 3.25] and i.tolist() == [0, 1, 0, -1] and h["triangle"][3] == MISS
    h, i, n = one_ray([stack, stack], W, (0.25, -0.5, -2.0), (0.0, 0.0, 1.0), tmax=3.5, max_hits=4)    # exactly at one
    assert n == 3 and h["t"].tolist() == [2.0, 2.5, 3.0, 3.5] and i.tolist() == [0, 1, 0, -1]
    h, i, n = one_ray([stack, stack], W, (0.25, -0.5, -2.0), (0.0, 0.0, 1.0), tmax=np.inf, max_hits=11)
    assert n == 10 and h["t"][10] == F(np.inf) and i[10] == -1


@pytest.mark.parametrize("tmax", [0.0, -0.0, -1.5, np.nan, -np.inf])
def test_tmax_not_positive_is_no_walk(stack, tmax):
    hits, inst, counts, counters = IM.all_hits([stack, stack], np.stack([EYE, shifted(0.5)]), [(0.25, -0.5, -2.0)], [(0.0, 0.0, 1.0)],
                                               [tmax], max_hits=3)
    assert counts[0] == 0 and (hits["triangle"] == MISS).all() and (hits["u"] == 0).all() and (hits["v"] == 0).all() and (inst == -1).all()
    assert np.array_equal(hits["t"][0].view(np.uint32), np.full(3, F(tmax)).view(np.uint32))
    assert counters == {"node_visits": 0, "leaf_visits": 0, "triangle_tests": 0, "traversals": 0, "bad_hits": 0}


def test_one_identity_instance_is_the_all_hits_restatement(stack):
    o, d, tmax = random_rays(stack, 3000, seed=3)
    want, want_counts, want_counters, want_nan = M.all_hits(stack, o, d, tmax, max_hits=6, details=True)
    hits, inst, counts, counters, nan, per = IM.all_hits([stack], EYE[None], o, d, tmax, max_hits=6, details=True)
    assert np.array_equal(hits.view(np.uint32), want.view(np.uint32)) and np.array_equal(counts, want_counts)
    assert counters == want_counters and np.array_equal(nan, want_nan) and np.array_equal(per[0], want_counts)
    assert np.array_equal(inst, np.where(want["triangle"] >= 0, 0, -1))
    assert (counts > 0).sum() > 100
    # the merge of per-instance answers cut at K' is the same answer (what the GPU composition test relies on)
    merged, minst, mcounts = IM.merge([want], [want_counts], tmax, 4)
    assert np.array_equal(merged.view(np.uint32), hits[:, :4].view(np.uint32)) and np.array_equal(minst, inst[:, :4])
    assert np.array_equal(mcounts, counts)
