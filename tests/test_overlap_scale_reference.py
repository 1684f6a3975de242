"""The cases of tests/overlap_scale_cases.py pinned on the CPU, with the restatement (tests/overlap_ref.py) alone: the TABLE of
kept and changed cells; at every cell the header's invariants (the set lies in stage 0's, K is a prefix of 64, the count is
the set's size); that the cells' boxes exercise the query; and that the cells tell wrong kernels apart: four mutants of the
header's arithmetic, restated here, each change some box's set in a cell named in CATCHES."""
import numpy as np
import pytest

import overlap_cases as OC
import overlap_ref as OR
import overlap_scale_cases as SC

F = np.float32
CELLS = [(name, k) for name in SC.SCENES for k in SC.S_EXPONENTS]
TINY = np.finfo(F).tiny


@pytest.mark.parametrize("name", SC.SCENES)
def test_the_table_is_the_restatements(pkg, name):
    base = SC.codes(pkg, name, 0) == OR.OVERLAP
    row = ""
    for k in SC.S_EXPONENTS:
        member = SC.codes(pkg, name, k) == OR.OVERLAP
        differ = int((member != base).any(1).sum())
        print(f"{name}, k = {k}: {differ} boxes differ from S = 1, {int((member & ~base).sum())} pairs added, {int((~member & base).sum())} lost")
        row += "k" if differ == 0 else "c"
        if differ and k not in (-28, 45):
            assert differ >= 50, (name, k, differ)
    assert row == SC.TABLE[name], (name, row)
    assert SC.flag(name, 0) == SC.flag(name, -27) == SC.flag(name, 44) == SC.KEPT    # the header's range


@pytest.mark.parametrize("name, k", CELLS + [(name, which) for name in SC.SCENES for which in SC.SPECIAL_CELLS])
def test_invariants_and_inputs_of_a_cell(pkg, name, k):
    code = SC.codes(pkg, name, k)
    pos, boxes = SC.inputs(pkg, name, k)
    member = code == OR.OVERLAP
    # the set lies in stage 0's: no member is a pair that a box axis separates (first_axis gives the first axis, and the stages'
    # order does not change the set), and an unwalked box has none
    lo, hi = OR.lo_hi(boxes)
    passes0 = ~OR._stage0(pos.reshape(-1, 3, 3), lo, hi).any(2) & OR.walked(boxes)[:, None]
    assert not (member & ~passes0).any(), (name, k)
    want64, n = OR.from_set(member, 64)
    assert np.array_equal(n, member.sum(1))
    for kk in (0, 1, 2, 3, 4, 8, 9):
        got, nk = OR.from_set(member, kk)
        assert np.array_equal(got, want64[:, :kk]) and np.array_equal(nk, n), (name, k, kk)
    c = OC.coverage(code, f"{name}, k = {k}")
    walked = OR.walked(boxes)
    print(f"{name}, k = {k}: {int(walked.sum())} boxes walked")
    if k in SC.SPECIAL_CELLS:
        assert walked.all() and (n > 0).sum() >= 100, (name, int((n > 0).sum()))
        assert (boxes["lo"][0] == -SC.FLT_MAX).all() and (boxes["hi"][0] == SC.FLT_MAX).all() and n[0] == member.shape[1]
        return
    assert c["n == 0"] > 0.05 and c["n > 8"] > 0.20 and c["n > 64"] > 0.10, (name, k, c)
    assert np.array_equal(walked, OR.walked(SC.base_boxes(pkg, name))), (name, k)
    if k == 0:
        OC.assert_interesting(code, name)
    if k == -90:
        assert np.array_equal(member, passes0), (name, "at 2^-90 no later axis separates: the set is stage 0's")


# the header's arithmetic with its operations as parameters -----------------------------------------------------------------------

class Arith:
    """mn, mx: the two-operand min and max; rnd: applied to every product and sum; fused: a*b - c*d as one fused
    multiply-subtract, fma(a, b, -(c*d)) with c*d rounded to float32 first (fused_sub: one rounding); translated: stage 0 on the
    translated corners against -+h"""

    def __init__(self, mn=OR._min, mx=OR._max, rnd=lambda x: x, fused=False, translated=False):
        self.mn, self.mx, self.rnd, self.fused, self.translated = mn, mx, rnd, fused, translated

    def mul(self, a, b):
        return self.rnd(a * b)

    def add(self, a, b):
        return self.rnd(a + b)

    def sub(self, a, b):
        return self.rnd(a - b)

    def det(self, a, b, c, d):
        if self.fused:
            return self.rnd(fused_sub(a, b, self.mul(c, d)))
        return self.sub(self.mul(a, b), self.mul(c, d))

    def min3(self, x, y, z):
        return self.mn(self.mn(x, y), z)

    def max3(self, x, y, z):
        return self.mx(self.mx(x, y), z)


def fused_sub(a, b, q):
    """fma(a, b, -q) of float32 arrays with ONE rounding.  In float64 the product p = a*b is exact (48 bits) and so is q; their
    difference s = p - q is rounded once to 53 bits, and TwoSum gives its error.  Rounding s to float32 as it stands would
    round twice, so where s is inexact it is first replaced by the odd one of the two float64 that bracket the exact difference
    (rounding to odd): 53 bits are more than 24 + 2, so the cast to float32 then rounds the exact difference correctly, ties
    and subnormal results included.  A non-finite s is left alone."""
    p, q = a.astype(np.float64) * b.astype(np.float64), -q.astype(np.float64)
    s = p + q
    bb = s - p
    err = (p - (s - bb)) + (q - bb)
    inexact = np.isfinite(s) & np.isfinite(err) & (err != 0) & ((s.view(np.int64) & 1) == 0)
    towards = np.where(err > 0, np.inf, -np.inf)
    return np.where(inexact, np.nextafter(s, towards), s).astype(F)


def flush(x):
    return np.where(np.abs(x) < TINY, np.copysign(F(0), x), x)


MUTANTS = {
    "fmin_fmax": Arith(mn=np.fmin, mx=np.fmax),
    "flushed_subnormals": Arith(rnd=flush),
    "fused_multiply_subtract": Arith(fused=True),
    "stage0_translated": Arith(translated=True),
}


def restate(positions, boxes, A, block=256):
    """(member bool [B, T], nonfinite bool [B, T]) by the header's text with A's operations: nonfinite marks the pairs that
    reach stage 1 with some value of stage 1 or 2 (d, r, a projection p, an edge axis' r) NaN or infinite"""
    tris = np.ascontiguousarray(positions, F).reshape(-1, 3, 3)
    lo_all, hi_all = (np.ascontiguousarray(x, F) for x in OR.lo_hi(boxes))
    member = np.zeros((len(lo_all), len(tris)), bool)
    nonfinite = np.zeros_like(member)
    half = F(0.5)
    X, Y, Z = 0, 1, 2
    with np.errstate(all="ignore"):
        for s in range(0, len(lo_all), block):
            lo_b, hi_b = lo_all[s:s + block], hi_all[s:s + block]
            if A.translated:
                m = A.add(A.mul(half, lo_b), A.mul(half, hi_b))[:, None, :]
                h = A.sub(A.mul(half, hi_b), A.mul(half, lo_b))[:, None, :]
                v = [A.sub(tris[None, :, c, :], m) for c in range(3)]
                sep0 = (A.min3(*v) > h) | (A.max3(*v) < -h)
            else:
                a, b, c = (tris[:, k, :] for k in range(3))
                sep0 = (A.min3(a, b, c)[None] > hi_b[:, None, :]) | (A.max3(a, b, c)[None] < lo_b[:, None, :])
            bi, ti = np.nonzero(~sep0.any(2))
            tri, lo, hi = tris[ti], lo_b[bi], hi_b[bi]
            m = A.add(A.mul(half, lo), A.mul(half, hi))
            h = A.sub(A.mul(half, hi), A.mul(half, lo))
            v0, v1, v2 = (A.sub(tri[:, c], m) for c in range(3))
            e0, e1, e2 = A.sub(v1, v0), A.sub(v2, v1), A.sub(v0, v2)
            nx = A.det(e0[:, Y], e1[:, Z], e0[:, Z], e1[:, Y])
            ny = A.det(e0[:, Z], e1[:, X], e0[:, X], e1[:, Z])
            nz = A.det(e0[:, X], e1[:, Y], e0[:, Y], e1[:, X])
            d = A.add(A.add(A.mul(nx, v0[:, X]), A.mul(ny, v0[:, Y])), A.mul(nz, v0[:, Z]))
            r = A.add(A.add(A.mul(h[:, X], np.abs(nx)), A.mul(h[:, Y], np.abs(ny))), A.mul(h[:, Z], np.abs(nz)))
            sep = (d > r) | (d < -r)
            odd = ~np.isfinite(d) | ~np.isfinite(r)
            for e in (e0, e1, e2):
                for u, w in ((Y, Z), (Z, X), (X, Y)):
                    p = [A.det(e[:, u], vv[:, w], e[:, w], vv[:, u]) for vv in (v0, v1, v2)]
                    r = A.add(A.mul(h[:, u], np.abs(e[:, w])), A.mul(h[:, w], np.abs(e[:, u])))
                    sep |= (A.min3(*p) > r) | (A.max3(*p) < -r)
                    odd |= ~np.isfinite(r) | ~np.isfinite(p[0]) | ~np.isfinite(p[1]) | ~np.isfinite(p[2])
            member[s + bi, ti] = ~sep
            nonfinite[s + bi, ti] = odd
    go = OR.walked(boxes)
    member[~go] = False
    nonfinite[~go] = False
    return member, nonfinite


# mutant -> the cells (scene, k) that tell it from the header's arithmetic; the test asserts each one and prints how many boxes
# change.  Measured here (boxes whose set changes, lobed_528 / small_trisrc where both are named):
#   fmin_fmax                 k = 67: 461 / 83 (0 at every other cell: overlap_scale_cases.ADDED_FOR_NAN)
#   flushed_subnormals        k = -64: 1405 / 1433, k = -70: 1338 / 1190, k = -40: 459 / 111 (0 from k = -27 up and at k = -90, where
#                             every later product is 0 either way)
#   fused_multiply_subtract   k = 0: 56 / 74, k = 45: 50 / 74, special: 51 / 54, special64: 34 / 45 (0 at k <= -64 and k >= 50)
#   stage0_translated         k = 0: 25 / 19, special: 1540 / 1521, special64: 895 / 902 (19 to 50 at every k)
CATCHES = {
    "fmin_fmax": [(name, 67) for name in SC.SCENES],
    "flushed_subnormals": [(name, k) for name in SC.SCENES for k in (-70, -64, -40)],
    "fused_multiply_subtract": [(name, k) for name in SC.SCENES for k in (0, 45, "special", "special64")],
    "stage0_translated": [(name, k) for name in SC.SCENES for k in (0, "special", "special64")],
}
_plain = {}


def plain(pkg, name, k):
    if (name, k) not in _plain:
        _plain[(name, k)] = restate(*SC.inputs(pkg, name, k), Arith())
    return _plain[(name, k)]


@pytest.mark.parametrize("name, k", sorted({cell for cells in CATCHES.values() for cell in cells}, key=str))
def test_the_parametrised_restatement_is_the_restatement(pkg, name, k):
    """with the header's own operations it gives overlap_ref's set, in every cell the mutants are judged in"""
    member, _ = plain(pkg, name, k)
    assert np.array_equal(member, SC.codes(pkg, name, k) == OR.OVERLAP), (name, k)


@pytest.mark.parametrize("name", SC.SCENES)
def test_the_special_class_meets_non_finite_projections(pkg, name):
    """none at S = 1, where no product can overflow (overlap_scale_cases.MEASURED: a translated corner is huge only beside a huge
    box coordinate, the edges are the mesh's own, below 1, and stage 0 lets no pair through whose product would pass FLT_MAX),
    so the boxes that do it are the half at 2^64: at least 20 of them"""
    boxes_with = {}
    for which in SC.SPECIAL_CELLS:
        member, nonfinite = plain(pkg, name, which)
        boxes_with[which] = int(nonfinite.any(1).sum())
        print(f"{name}, {which}: {boxes_with[which]} boxes hold a pair with a NaN or infinite stage 1 or 2 value "
              f"({int(nonfinite.sum())} pairs, {int((nonfinite & member).sum())} of them overlapping)")
    assert boxes_with["special"] == 0, (name, boxes_with)
    assert boxes_with["special64"] >= 20, (name, boxes_with)


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_a_mutant_is_told_apart(pkg, mutant):
    for name, k in CATCHES[mutant]:
        want, _ = plain(pkg, name, k)
        got, _ = restate(*SC.inputs(pkg, name, k), MUTANTS[mutant])
        changed = int((got != want).any(1).sum())
        print(f"{mutant}: {name}, k = {k}: {changed} boxes' sets change ({int((got & ~want).sum())} pairs added, {int((want & ~got).sum())} lost)")
        assert changed >= 1, (mutant, name, k)
