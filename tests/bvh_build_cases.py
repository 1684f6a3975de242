"""Inputs that take make_bvh to the places where a level-parallel rebuild of the sequential algorithm (csrc/bvh_build.hip) could
part from it (host/bvh.cpp, pinned to the reference): exact ties, node ranges on and one off the multiples of a wave (64) and a
workgroup (256), the partition's extreme exchange patterns, the ends of the float range, many thin levels, large leaves inside
a tree, zeros of both signs.  Deterministic and GPU-free; the largest case has 1,025 triangles.

A case is (positions float32 [3T, 3], triangles int [T, 3], normals float32 [3T, 3]); CaseSet writes it as a trisrc file.  The
normals are constants, never derived from the geometry (smooth normals are not finite at the extreme scales); every triangle
has a unit normal of its own, (cos, sin, 0) of an angle that encodes its place in the input, so that no two triangles share a
vertex (the loader merges equal vertices, +0 with -0) and the input triangle at every post-build position can be read back from
the built tree (`input_ids`).

Families (FAMILIES: family -> case names):
  ladder     one 300-triangle soup (centres uniform in [-1, 1]^3, corners normal(0, 0.1)) times 2^e, and a slab of it (z times
             2^-40) whose root area overflows later than the cube's; two inputs whose barycentres overflow, so that the bin
             index is computed from +inf and from NaN
  ties       the triangle (0,0,0) (.5,0,0) (0,.5,0) on integer lattices whose barycentre spreads tie (x = y largest; all three;
             y = z largest, with the triangle turned into the yz plane), in lattice order, reversed and shuffled; a row whose
             barycentres lie exactly on the boundaries of the root's 40 bins and on its split plane
  rows       m triangles 2.5 apart along x, m around the multiples of 64 and 256
  blocks     such a row with a block of d identical triangles far to one side of it (or inside it): the block retires as one
             large leaf, and its positions stay retired in whole waves and workgroups next to live ones
  partition  the 1025-row and a 1,000-triangle soup in input orders that leave the root's exchange partition nothing to move,
             everything, every other element, the two end elements; the root's split is taken from the host build's tree
  chain      64 tiny triangles at 3^k along one axis: a depth-18 tree of thin levels
  duplicates a 512-row with 11, 40 and 41 copies of one of its triangles in one place
  zeros      corners drawn from {+0, -0, +-1e-5f, +-2e-5f}; the same scaled and shifted to where the 1e-5 bump is absorbed; and
             with x >= 1e-5f and y <= -1e-5f, so that node boxes have planes that are exactly +0"""
from __future__ import annotations

import os

import numpy as np

F = np.float32
BASE = np.array([[0, 0, 0], [.5, 0, 0], [0, .5, 0]], np.float64)       # the lattice triangle
ONE = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float64)          # the row triangle
PITCH = 2.5

LADDER_EXPONENTS = (-140, -126, -40, -36, -24, -17, 0, 20, 56, 61, 62, 63, 100, 125, 126)
SLAB_EXPONENTS = (61, 62, 63, 64)
LATTICES = {"16x16x4": (16, 16, 4), "8x8x8": (8, 8, 8), "4x16x16": (4, 16, 16)}
ORDERS = ("lattice", "reversed", "shuffled")
ROWS = (63, 64, 65, 255, 256, 257, 511, 512, 513, 1025)
BLOCK_ROWS, BLOCK_SIZES = (64, 65, 256, 257), (64, 65, 256, 300)
PARTITION_BASES = ("row_1025", "soup_1000")
PARTITION_ORDERS = ("ascending", "descending", "alternating", "two_ends")
DUPLICATES = (11, 40, 41)


def _tag(e):
    return f"m{-e}" if e < 0 else f"p{e}"


def _soup(seed, count):
    rng = np.random.default_rng(seed)
    centres = rng.uniform(-1.0, 1.0, (count, 1, 3))
    return centres + rng.normal(0.0, 0.1, (count, 3, 3))          # float64 [T, 3, 3]


def _row(m, x0=0.0):
    return ONE[None] + np.array([PITCH, 0, 0])[None, None] * np.arange(m)[:, None, None] + np.array([x0, 0, 0])


def _block(d, x):
    return np.tile(ONE[None] + np.array([x, 0, 0]), (d, 1, 1))


def _lattice(dims, order):
    nx, ny, nz = dims
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")        # x runs fastest
    at = np.stack([i.ravel(), j.ravel(), k.ravel()], axis=1).astype(np.float64)
    if order == "reversed":
        at = at[::-1]
    elif order == "shuffled":
        at = at[np.random.default_rng(4100 + nx).permutation(len(at))]
    # 4x16x16 ties y with z: the triangle turned into the yz plane.  As it lies in the xy plane its barycentre is off the lattice
    # point by 1/6 in y and by 0 in z, and the two spreads then differ by one unit in the last place
    triangle = BASE[:, [2, 0, 1]] if dims == (4, 16, 16) else BASE
    return triangle[None] + at[:, None, :]


def _bin_boundary_row():
    """39 triangles whose corners' x are c - 8, c, c + 8 for c = 1032 + 8 k: the barycentre is c exactly, the 1e-5 bump is
    absorbed (|x| >= 512), the root's box is [1024, 1344] and (c - 1024) * 40 / 320 = k + 1 is an integer: every barycentre lies
    on a bin boundary, and whichever plane 1024 + 8 i the sweep picks is some triangle's barycentre."""
    c = 1032.0 + 8.0 * np.arange(39)
    t = np.zeros((39, 3, 3))
    t[:, 0, 0], t[:, 1, 0], t[:, 2, 0] = c - 8, c, c + 8
    t[:, 1, 1] = 0.5
    t[:, 2, 2] = 0.25
    return t


def _chain(axis):
    t = np.tile(0.25 * BASE[None], (64, 1, 1))
    t[:, :, axis] += np.array([float(3 ** k) for k in range(64)])[:, None]          # (exact integers, rounded once)
    return t


def _duplicates(counts):
    row = _row(512)
    places = {11: 100, 40: 250, 41: 400}
    extra = [np.tile(row[places[n]][None], (n - 1, 1, 1)) for n in counts]      # n equal triangles in one place, the row's own included
    return np.concatenate([row] + extra)


ZERO_VALUES = np.array([0.0, -0.0, 1e-5, -1e-5, 2e-5, -2e-5], F)


def _zeros(variant):
    rng = np.random.default_rng(6200)
    t = ZERO_VALUES[rng.integers(0, len(ZERO_VALUES), (200, 3, 3))]          # float32, the signs of the zeros kept
    if variant == "on_planes":       # x >= 1e-5f and y <= -1e-5f: every node's low x plane and high y plane is x - x = +0
        t[..., 0] = np.abs(t[..., 0]) + np.where(t[..., 0] == 0, F(1e-5), F(0))
        t[..., 1] = -np.abs(t[..., 1]) - np.where(t[..., 1] == 0, F(1e-5), F(0))
    if variant == "scaled":          # 1e-5 * 2^26 = 671: the nonzero corners lie where x +- 1e-5 == x; the zeros stay zeros
        t = t * F(2.0 ** 26)
    elif variant == "shifted":       # everything in [705, 3391]: every box plane is an exact corner coordinate
        t = t * F(2.0 ** 26) + F(2048.0)
    return t


def _poles(kind):
    """The soup, flat in y and z, in clusters along x so far apart that a barycentre's sum overflows:
      inf  half at -2^126 (finite barycentres), half at 1.5 * 2^126 (barycentres +inf): hi - lo is finite, `scaled` is +inf, which
           no int holds: those triangles, the rightmost, go to bin 0, where all the others are: the root cannot split.  A
           builder that sent them to the LAST bin would split it.
      nan  thirds at -1.5 * 2^127, 0 and +1.5 * 2^127: hi - lo overflows as well, and so does (b - lo) * bins even in the middle:
           `scaled` is NaN (inf / inf) for every triangle, everything goes to bin 0 and the root cannot split"""
    t = _soup(7300, 300) * np.array([2.0 ** 120, 2.0 ** -4, 2.0 ** -4])
    if kind == "inf":
        t[:150, :, 0] -= 2.0 ** 126
        t[150:, :, 0] += 1.5 * 2.0 ** 126
    else:
        t[:100, :, 0] -= 1.5 * 2.0 ** 127
        t[200:, :, 0] += 1.5 * 2.0 ** 127
    return t


def _generators():
    g = {}
    for e in LADDER_EXPONENTS:
        g[f"ladder_cube_{_tag(e)}"] = lambda e=e: _soup(7300, 300) * 2.0 ** e
    for e in SLAB_EXPONENTS:
        g[f"ladder_slab_{_tag(e)}"] = lambda e=e: _soup(7300, 300) * np.array([1.0, 1.0, 2.0 ** -40]) * 2.0 ** e
    g["ladder_poles_inf"] = lambda: _poles("inf")
    g["ladder_poles_nan"] = lambda: _poles("nan")
    for name, dims in LATTICES.items():
        for order in ORDERS:
            g[f"ties_{name}_{order}"] = lambda dims=dims, order=order: _lattice(dims, order)
    g["ties_bin_boundary_row"] = _bin_boundary_row
    for m in ROWS:
        g[f"row_{m}"] = lambda m=m: _row(m)
    for m in BLOCK_ROWS:
        for d in BLOCK_SIZES:
            far = 10 * PITCH * m
            g[f"block_{d}_before_row_{m}"] = lambda m=m, d=d, far=far: np.concatenate([_block(d, -far), _row(m)])
            g[f"row_{m}_before_block_{d}"] = lambda m=m, d=d, far=far: np.concatenate([_row(m), _block(d, PITCH * m + far)])
    # the block in the middle, of the input and of space: row, a gap, the block, a gap, row
    g["block_256_inside_row_257"] = lambda: np.concatenate([_row(128, -8000.0), _block(256, 0.0), _row(129, 8000.0)])
    for axis, name in enumerate("xyz"):
        g[f"chain_{name}"] = lambda axis=axis: _chain(axis)
    for n in DUPLICATES:
        g[f"duplicates_{n}"] = lambda n=n: _duplicates((n,))
    g["duplicates_11_40_41"] = lambda: _duplicates(DUPLICATES)
    g["zeros"] = lambda: _zeros("plain")
    g["zeros_scaled"] = lambda: _zeros("scaled")
    g["zeros_shifted"] = lambda: _zeros("shifted")
    g["zeros_on_planes"] = lambda: _zeros("on_planes")
    g["soup_1000"] = lambda: _soup(7400, 1000)
    return g


GENERATORS = _generators()
PARTITION_NAMES = tuple(f"partition_{base}_{order}" for base in PARTITION_BASES for order in PARTITION_ORDERS)

FAMILIES = {
    "ladder": tuple(n for n in GENERATORS if n.startswith("ladder_")),
    "ties": tuple(n for n in GENERATORS if n.startswith("ties_")),
    "rows": tuple(f"row_{m}" for m in ROWS),
    "blocks": tuple(n for n in GENERATORS if "block_" in n),
    "partition": PARTITION_NAMES,
    "chain": tuple(n for n in GENERATORS if n.startswith("chain_")),
    "duplicates": tuple(n for n in GENERATORS if n.startswith("duplicates_")),
    "zeros": ("zeros", "zeros_scaled", "zeros_shifted", "zeros_on_planes"),
}
NAMES = tuple(n for family in FAMILIES.values() for n in family)          # (soup_1000 itself is only the partition cases' base)

# the device-resident pipeline's subset (scene creation on these): everything but the extreme rungs and the zeros
PIPELINE_NAMES = tuple(f"ladder_cube_{_tag(e)}" for e in (-17, 0, 20)) + tuple(n for n in FAMILIES["ties"] if "bin_boundary" not in n) \
    + FAMILIES["rows"] + FAMILIES["blocks"] + FAMILIES["partition"] + FAMILIES["chain"] + FAMILIES["duplicates"]
FRAME_NAMES = ("ties_8x8x8_shuffled", "block_65_before_row_257", "chain_y")

# the option sets (BVH_MAX_DEPTH, BVH_LEAF_MAX, SAH_CTRAV, SAH_CISEC; None = the default) and the inputs each is built on
OPTION_SETS = {
    "max_depth_0": (0, None, None, None), "max_depth_1": (1, None, None, None), "max_depth_4": (4, None, None, None),
    "leaf_max_0": (None, 0, None, None), "leaf_max_1": (None, 1, None, None), "leaf_max_m1": (None, -1, None, None),
    "sah_cisec_0": (None, None, None, "0"), "sah_ctrav_1e6": (None, None, "1e6", None),
}
OPTION_INPUTS = ("chain_x", "ties_16x16x4_shuffled", "row_513", "ladder_cube_p0")
DEFAULTS = (30, 10, 1.0, 4.0)


def option_environment(name) -> dict:
    """the environment variables of an option set, as both the host builder and the reference read them"""
    keys = ("BVH_MAX_DEPTH", "BVH_LEAF_MAX", "SAH_CTRAV", "SAH_CISEC")
    return {k: str(v) for k, v in zip(keys, OPTION_SETS[name]) if v is not None}


def option_values(name) -> tuple:
    """(max_depth, leaf_max, sah_ctrav, sah_cisec) of an option set, defaults filled in"""
    given = OPTION_SETS[name]
    return tuple(type(d)(g) if g is not None else d for g, d in zip(given, DEFAULTS))


def id_normals(count) -> np.ndarray:
    """float32 [count, 3]: the unit normal that encodes a triangle's place in the input"""
    angle = 2.0 * np.pi * np.arange(count) / 2048.0
    return np.stack([np.cos(angle), np.sin(angle), np.zeros(count)], axis=1).astype(F)


def barycentres(corners) -> np.ndarray:
    """indexed_triangle's barycentre, ((a + b) + c) / 3 in float32 (geometry.h:79-90), of float32 corners [T, 3, 3]"""
    c = np.asarray(corners, F)
    return ((c[:, 0] + c[:, 1]) + c[:, 2]) / F(3.0)


class HostTree:
    """The host build's tree of a World, as numpy arrays in pre-order, with each node's level and the input triangle at
    every post-build position."""

    def __init__(self, world):
        tree = world.export_tree()
        n, t = tree.node_count, tree.triangle_count
        take = lambda ptr, count: np.ctypeslib.as_array(ptr, shape=(count,)).copy()   # noqa: E731
        self.parent, self.negative, self.positive = take(tree.node_parent, n), take(tree.node_negative, n), take(tree.node_positive, n)
        self.box = take(tree.node_box, 6 * n).reshape(n, 6)
        self.direction = take(tree.node_direction, 3 * n).reshape(n, 3)
        self.start, self.triangles = take(tree.node_start, n), take(tree.node_triangles, n)
        self.triangle_vertices = take(tree.triangle_vertices, 3 * t).reshape(t, 3)
        self.vertex_data = take(tree.vertex_data, 9 * tree.vertex_count).reshape(-1, 9)      # position, colour, normal
        self.level = np.zeros(n, np.int64)
        for k in range(1, n):                        # pre-order: a parent comes before its children
            self.level[k] = self.level[self.parent[k]] + 1
        self.is_leaf = self.negative < 0
        self.info = world.info

    def input_ids(self) -> np.ndarray:
        """which input triangle sits at each post-build position: read from the normal of its first corner"""
        first = self.vertex_data[self.triangle_vertices[:, 0], 6:8].astype(np.float64)
        turns = np.arctan2(first[:, 1], first[:, 0]) % (2.0 * np.pi) * 2048.0 / (2.0 * np.pi)
        ids = np.rint(turns).astype(np.int64)
        assert np.abs(turns - ids).max() < 0.01 and np.array_equal(np.sort(ids), np.arange(len(ids))), "the normals no longer name the triangles"
        return ids

    def root_split(self):
        """(axis, how many triangles went below the plane) of the root; None if the root is a leaf"""
        if self.is_leaf[0]:
            return None
        # the negative subtree is nodes [negative[0], positive[0]) of the pre-order; branches hold no triangles
        below = int(self.triangles[self.negative[0]:self.positive[0]].sum())
        return int(np.argmax(self.direction[0])), below


def misplaced_at_root(tree: HostTree) -> tuple:
    """For a case's own host tree: (flags, mid) where flags[p] says whether the input's p-th triangle belongs below the root's
    plane and mid is how many do.  Position p is misplaced when p < mid and not flags[p], or p >= mid and flags[p]."""
    _, mid = tree.root_split()
    flags = np.zeros(len(tree.triangle_vertices), bool)
    flags[tree.input_ids()[:mid]] = True
    return flags, mid


def reorder_for_partition(corners, tree: HostTree, order) -> np.ndarray:
    """`corners` (the base case, whose host tree is `tree`) in the input order that gives the root's partition the stated work.
    The root's split does not depend on the input order (bounds and bins are sets), so the base's split is the reordered case's."""
    axis, mid = tree.root_split()
    flags, _ = misplaced_at_root(tree)
    key = barycentres(corners.astype(F))[:, axis]
    ascending = np.argsort(key, kind="stable")
    assert flags[ascending[:mid]].all() and not flags[ascending[mid:]].any()       # below the plane <=> among the mid smallest
    below, above = ascending[:mid], ascending[mid:]
    if order == "ascending":
        perm = ascending
    elif order == "descending":
        perm = ascending[::-1]
    elif order == "two_ends":
        perm = ascending.copy()
        perm[0], perm[-1] = ascending[-1], ascending[0]
    elif order == "alternating":
        pairs = min(len(below), len(above))
        perm = np.empty(2 * pairs, ascending.dtype)
        perm[0::2], perm[1::2] = above[:pairs], below[:pairs]
        perm = np.concatenate([perm, below[pairs:], above[pairs:]])
    else:
        raise ValueError(order)
    return corners[perm]


class CaseSet:
    """Writes the cases as trisrc files into `directory`, once each.  The partition cases need the host builder (`pkg`)."""

    def __init__(self, pkg, directory):
        self.pkg, self.directory = pkg, str(directory)
        self._corners = {}

    def corners(self, name) -> np.ndarray:
        """float32 [T, 3, 3]"""
        if name not in self._corners:
            if name.startswith("partition_"):
                base = next(b for b in PARTITION_BASES if name.startswith(f"partition_{b}_"))
                order = name[len(f"partition_{base}_"):]
                world = self.pkg.World(self.path(base))
                made = reorder_for_partition(self.corners(base), HostTree(world), order)
                world.close()
            else:
                made = GENERATORS[name]()
            self._corners[name] = np.ascontiguousarray(made, F)
        return self._corners[name]

    def arrays(self, name):
        """(positions float32 [3T, 3], triangles [T, 3], normals float32 [3T, 3])"""
        c = self.corners(name)
        t = len(c)
        return c.reshape(-1, 3), np.arange(3 * t).reshape(t, 3), np.repeat(id_normals(t), 3, axis=0)

    def path(self, name) -> str:
        path = os.path.join(self.directory, name + ".trisrc")
        if not os.path.exists(path):
            pos, tri, normals = self.arrays(name)
            self.pkg.scenes.write_trisrc(path + ".part", pos, tri, normals=normals)
            os.replace(path + ".part", path)
        return path


# ---- what is compared with the reference: the flattened arrays (scene_shader_data, world.h:68-93) and the counts

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bvh_build_cases.ref.npz")
REF_HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref", "ref_host")
FLAT_ARRAYS = ("vertex_positions", "vertex_normals", "vertex_colors", "group_boxmin", "group_boxmax", "group_children", "group_objects",
               "group_directions") + tuple(f"group_hitmiss_{c}" for c in range(8))
FLAT_SCALARS = ("vertex_count", "vertex_data_rows", "group_count", "group_data_rows", "tree_root", "triangle_count")


def fixture_keys():
    """the rows of the committed fixture: every case under the defaults, then the option sets' inputs under each set"""
    return [("", name) for name in NAMES] + [(options, name) for options in OPTION_SETS for name in OPTION_INPUTS]


def summary(flat: dict, triangle_count=None) -> dict:
    """{"sha256": the digest of each flattened array's bits, "sizes": their lengths, "scalars": the counts} of a World's arrays()
    or of a dump by ref_host (refdump.read_dump): what the fixture holds per case"""
    from refdump import bits_sha256
    one = lambda v: int(np.asarray(v).reshape(-1)[0])   # noqa: E731
    # (World.arrays() has no triangle_count: only that one may come from the argument; any other missing key raises)
    scalars = [int(triangle_count) if k == "triangle_count" and k not in flat else one(flat[k]) for k in FLAT_SCALARS]
    return {"sha256": [bits_sha256(flat[k]) for k in FLAT_ARRAYS], "sizes": [int(np.asarray(flat[k]).size) for k in FLAT_ARRAYS],
            "scalars": scalars}


def reference_summary(path, environment=None, scratch=None) -> dict:
    """summary() of the compiled reference's own dump of the file, made now"""
    import subprocess
    from refdump import read_dump
    dump = (scratch or path) + ".ref.bin"
    env = dict(os.environ)
    for k in ("BVH_MAX_DEPTH", "BVH_LEAF_MAX", "SAH_CTRAV", "SAH_CISEC"):
        env.pop(k, None)
    env.update(environment or {})
    subprocess.run([REF_HOST, path, dump, "96", "64"], check=True, env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    made = summary(read_dump(dump))
    os.remove(dump)
    return made


def file_sha256(path) -> str:
    import hashlib
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def load_fixture() -> dict:
    """(option set or "", case) -> {"sha256", "sizes", "scalars", "input_sha256"}"""
    z = np.load(FIXTURE)
    assert [str(a) for a in z["arrays"]] == list(FLAT_ARRAYS) and [str(s) for s in z["scalar_names"]] == list(FLAT_SCALARS)
    out = {}
    for row, (options, name) in enumerate(zip(z["options"], z["names"])):
        out[(str(options), str(name))] = {"sha256": [d.decode() for d in z["sha256"][row]], "sizes": [int(s) for s in z["sizes"][row]],
                                          "scalars": [int(s) for s in z["scalars"][row]], "input_sha256": z["input_sha256"][row].decode()}
    return out


def write_fixture(cases: "CaseSet"):
    """tests/golden/make_golden.py: the reference's dumps of every row of fixture_keys(), as digests"""
    keys = fixture_keys()
    rows = [dict(reference_summary(cases.path(name), option_environment(options) if options else None), input_sha256=file_sha256(cases.path(name)))
            for options, name in keys]
    np.savez_compressed(FIXTURE, arrays=np.array(FLAT_ARRAYS), scalar_names=np.array(FLAT_SCALARS),
                        options=np.array([k[0] for k in keys]), names=np.array([k[1] for k in keys]),
                        sha256=np.array([r["sha256"] for r in rows], dtype="S64"), sizes=np.array([r["sizes"] for r in rows], np.int64),
                        scalars=np.array([r["scalars"] for r in rows], np.int64), input_sha256=np.array([r["input_sha256"] for r in rows], dtype="S64"))
