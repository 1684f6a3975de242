"""The device update's level-by-level build from three presorted lists (tests/instance_build_ref.py: presorted_build) gives the
host update's recursive object-median build (median_build) node for node: sizes 1, 2, 3 and 2^k +- 1, many equal centres,
-0 and +0 centres, and collinear and coplanar placements."""
import numpy as np
import pytest

import instance_build_ref as B


def check(centres):
    want = B.median_build(centres)
    got = B.presorted_build(centres)
    assert len(got) == 2 * len(centres) - 1
    assert got == want


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 33, 63, 64, 65, 127, 129, 255, 257])
def test_random_centres(n):
    rng = np.random.default_rng(n)
    check(rng.normal(size=(n, 3)) * rng.uniform(0.1, 10, 3))


@pytest.mark.parametrize("n", [2, 3, 17, 100, 257])
def test_many_equal_centres(n):
    rng = np.random.default_rng(1000 + n)
    check(rng.integers(-2, 3, (n, 3)).astype(np.float64))            # few distinct values on every axis
    check(np.ones((n, 3)))                                            # all the same: ties by id everywhere


@pytest.mark.parametrize("n", [2, 5, 33, 200])
def test_signed_zeros(n):
    rng = np.random.default_rng(2000 + n)
    c = rng.integers(-1, 2, (n, 3)).astype(np.float64)
    c[c == 0] = np.where(rng.random((c == 0).sum()) < 0.5, -0.0, 0.0)
    c[0, 0], c[1, 0] = -0.0, 0.0
    assert np.signbit(c[c == 0]).any() and (~np.signbit(c[c == 0])).any()
    check(c)


@pytest.mark.parametrize("n", [3, 31, 129])
def test_collinear_and_coplanar(n):
    rng = np.random.default_rng(3000 + n)
    t = rng.normal(size=n)
    check(np.stack([t, 2 * t, np.zeros(n)], 1))                       # on a line through the origin
    check(np.stack([np.zeros(n), np.zeros(n), np.sort(t)], 1))        # on the z axis, sorted
    check(np.stack([rng.normal(size=n), rng.normal(size=n), np.full(n, 3.0)], 1))   # in a plane
    g = np.arange(n) % 4
    check(np.stack([g * 1.0, g * 1.0, g * 1.0], 1))                   # equal extents on every axis: axis 0 wins


def test_a_duplicate_heavy_large_set():
    rng = np.random.default_rng(7)
    c = rng.normal(size=(600, 3))
    c[::3] = c[0]
    check(c)
