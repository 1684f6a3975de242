"""The workload generators that more than one profiles/*_bench.py script uses: points, rays and instance maps, all seeded.
Their outputs are the workloads the recorded results were measured on, so every seed, every dtype and every order of
operations here is fixed (tests/test_bench_harness.py compares each against values recorded in tests/golden/)."""
import numpy as np

F = np.float32


def rotation(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def grid_transforms(dims, spacing, rng, scale=(0.6, 1.0)):
    cells = np.stack(np.meshgrid(*[np.arange(k) for k in dims], indexing="ij"), -1).reshape(-1, len(dims))
    M = np.zeros((len(cells), 3, 4))
    for i, c in enumerate(cells):
        M[i, :, :3] = rotation(rng) * rng.uniform(*scale)
        M[i, :len(c), 3] = c * spacing
    return M.astype(F)


def down_rays(lo, hi, n, rng):
    """rays from above the region's top, aimed at random points of its floor (a camera looking down at the grid)"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    size = hi - lo
    o = lo + size * rng.random((n, 3))
    o[:, 2] = hi[2] + size.max()
    aim = lo + size * rng.random((n, 3))
    aim[:, 2] = lo[2]
    d = aim - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o.astype(F), d.astype(F)


def through_rays(positions, n, seed):
    """origins on a sphere of 1.5 box diagonals around the box centre, aimed at uniform points of the box; tmax 1e7"""
    rng = np.random.default_rng(seed)
    v = positions.reshape(-1, 3).astype(np.float64)
    lo, hi = v.min(0), v.max(0)
    centre, radius = (lo + hi) / 2, 1.5 * np.linalg.norm(hi - lo)
    s = rng.normal(size=(n, 3))
    o = centre + radius * s / np.linalg.norm(s, axis=1, keepdims=True)
    d = lo + (hi - lo) * rng.random((n, 3)) - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o.astype(F), d.astype(F), np.full(n, F(1e7))


def camera_rays(params, width, height, xform):
    """the 1-spp pixel-centre rays of trace_pixels in object space, float32 (row 0 = the bottom row)"""
    px, py = np.meshgrid(np.arange(width, dtype=F), np.arange(height, dtype=F))
    u = (px.reshape(-1) + F(0.5)) / F(width)
    v = (py.reshape(-1) + F(0.5)) / F(height)
    ipw, aspect = F(params.image_plane_width), F(params.aspect)
    eye = np.stack([ipw * (u - F(0.5)), ipw * (v - F(0.5)) * aspect, np.full_like(u, F(-1))], axis=1)
    eye = eye / np.sqrt((eye * eye).sum(1, dtype=F), dtype=F)[:, None]
    origin = xform(params.camera_matrix, np.zeros((1, 3), F), 1.0)
    d = xform(params.camera_normal_matrix, eye, 0.0)
    d = d / np.sqrt((d * d).sum(1, dtype=F), dtype=F)[:, None]
    return np.repeat(xform(params.object_matrix, origin, 1.0), len(d), axis=0), xform(params.object_normal_matrix, d, 0.0)


def ao_rays(positions, n, seed):
    """points on the surface (uniform over triangles' area), cosine-distributed directions about the geometric normal
    (its side chosen at random), the origin lifted off the surface by 1e-4 of the scene's extent"""
    rng = np.random.default_rng(seed)
    tri = positions.reshape(-1, 3, 3).astype(np.float64)
    cross = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    area = np.linalg.norm(cross, axis=1)
    k = rng.choice(len(tri), n, p=area / area.sum())
    b = rng.random((n, 2))
    b = np.where(b.sum(1, keepdims=True) > 1, 1 - b, b)
    p = tri[k, 0] + b[:, :1] * (tri[k, 1] - tri[k, 0]) + b[:, 1:] * (tri[k, 2] - tri[k, 0])
    nrm = cross[k] / np.maximum(area[k], 1e-30)[:, None]
    nrm *= np.where(rng.random(n) < 0.5, -1.0, 1.0)[:, None]
    # a cosine-weighted direction in the normal's frame
    r1, r2 = rng.random(n), rng.random(n)
    phi, s = 2 * np.pi * r1, np.sqrt(r2)
    t1 = np.cross(nrm, np.where(np.abs(nrm[:, :1]) < 0.9, [[1.0, 0, 0]], [[0, 1.0, 0]]))
    t1 /= np.linalg.norm(t1, axis=1, keepdims=True)
    t2 = np.cross(nrm, t1)
    d = t1 * (s * np.cos(phi))[:, None] + t2 * (s * np.sin(phi))[:, None] + nrm * np.sqrt(1 - r2)[:, None]
    extent = float(np.linalg.norm(tri.reshape(-1, 3).max(0) - tri.reshape(-1, 3).min(0)))
    return (p + nrm * 1e-4 * extent).astype(F), d.astype(F), F(extent / 10)


def near_points(positions, n, seed):
    """points on the surface (uniform over the triangles' area) moved along the normal by up to extent/100 either way"""
    rng = np.random.default_rng(seed)
    tri = positions.reshape(-1, 3, 3).astype(np.float64)
    cross = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    area = np.linalg.norm(cross, axis=1)
    k = rng.choice(len(tri), n, p=area / area.sum())
    b = rng.random((n, 2))
    b = np.where(b.sum(1, keepdims=True) > 1, 1 - b, b)
    p = tri[k, 0] + b[:, :1] * (tri[k, 1] - tri[k, 0]) + b[:, 1:] * (tri[k, 2] - tri[k, 0])
    nrm = cross[k] / np.maximum(area[k], 1e-30)[:, None]
    extent = float(np.linalg.norm(tri.reshape(-1, 3).max(0) - tri.reshape(-1, 3).min(0)))
    return (p + nrm * ((rng.random(n) * 2 - 1) * extent / 100)[:, None]).astype(F)


def morton_order(p):
    """the permutation that sorts points by the 30-bit Morton code of their position in their bounding box"""
    lo, hi = p.min(0), p.max(0)
    q = np.clip(((p - lo) / np.maximum(hi - lo, 1e-30) * 1023).astype(np.int64), 0, 1023)
    code = np.zeros(len(p), np.int64)
    for bit in range(10):
        for axis in range(3):
            code |= ((q[:, axis] >> bit) & 1) << (3 * bit + axis)
    return np.argsort(code, kind="stable")


def near_surface_points(positions, maps, n, rng):
    """world points [n, 4] float32 (max_dist2 = +inf) near the surfaces of the placed copies of `positions`"""
    tris = positions.reshape(-1, 3, 3).astype(np.float64)
    extent = float(np.ptp(tris.reshape(-1, 3), axis=0).max())
    i, t = rng.integers(0, len(maps), n), rng.integers(0, len(tris), n)
    on = tris[t].mean(1) + rng.normal(size=(n, 3)) * extent / 100
    A = maps.astype(np.float64)
    out = np.full((n, 4), np.inf, F)
    out[:, :3] = np.einsum("nrc,nc->nr", A[i, :, :3], on) + A[i, :, 3]
    return out
