"""Instanced box-overlap query throughput (include/shader_ray_instance_overlap.h), one JSON line on stdout.

Rows, each on the device path with 2^18 boxes:
  a_identity     the bunny-class scene under one identity instance against Scene.triangles_in_boxes on the same boxes: the cost
                 of the layer (and whether the two wrote the same indices and counts)
  b_bunny_8x8    profiles/instance_bench.py's 64 rotated and scaled bunny-class copies on an 8 x 8 grid
Both on cells of a 128^3 grid over the world box (a contiguous run of its middle slabs, in grid order) and on
profiles/overlap_bench.py's "5 % boxes" (cubes of 5 % of the unscaled scene's diagonal about points of the placed surfaces), in
three forms each: counts only (K = 0), K = 8 with counts, and SHRAY_OVERLAP_ANY.

Every time is the median of --trials launches after --warmup launches, bracketed by HIP events on the current torch stream,
with the fastest and the slowest launch.  The walk counters per box (image-box tests, leaf visits, triangle tests, instance
walks begun) come from one blocking counting run over 2^12 of the same boxes, and with them the mean count.

Usage: python profiles/instance_overlap_bench.py [--trials 15] [--warmup 5] [--boxes 262144] [--out FILE]"""
import sys

import numpy as np

import bench_harness as H
from bench_workloads import grid_transforms

F = np.float32
SAMPLE = 1 << 12
GRID = 128
FORMS = (("counts_only", 0, False), ("K8_counts", 8, False), ("any", 0, True))


def main():
    ap = H.parser()
    ap.add_argument("--boxes", type=int, default=1 << 18)
    args = ap.parse_args()
    import torch
    import instance_point_ref as IP

    pkg = H.load_package()
    stream = torch.cuda.current_stream()
    n = args.boxes
    median_ms = H.median_timer(args, slow_ms=1000.0)

    def time_cell(fn):
        return H.entry(median_ms(fn), "Mboxes_s", n)

    def cells(s, plain, d_boxes, what):
        """per form: the set's time and, with `plain` (a Scene), Scene.triangles_in_boxes' on the same boxes"""
        cell = {}
        sample = d_boxes[torch.from_numpy(np.random.default_rng(5).permutation(len(d_boxes))[:SAMPLE]).cuda()].cpu().numpy()
        for name, any_only in (("counting", False), ("any", True)):
            _, _, cnt, c = s.triangles_in_boxes(sample, max_triangles=0, counters=True, any_only=any_only)
            cell[f"per_box_{name}"] = {key: round(c[key] / len(sample), 2) for key in ("node_visits", "leaf_visits", "triangle_tests", "traversals")}
            if not any_only:
                cell["n_mean"], cell["n_max"], cell["touched"] = round(float(cnt.mean()), 2), int(cnt.max()), round(float((cnt > 0).mean()), 4)
        d_out = torch.empty((n, 8), dtype=torch.int32, device="cuda")
        d_inst = torch.empty((n, 8), dtype=torch.int32, device="cuda")
        d_cnt = torch.empty(n, dtype=torch.int32, device="cuda")
        for name, k, any_only in FORMS:
            r = time_cell(lambda: s.triangles_in_boxes_into(d_boxes.data_ptr(), n, d_out.data_ptr() if k else 0, d_inst.data_ptr() if k else 0,
                                                            d_cnt.data_ptr(), k, any_only, stream.cuda_stream))
            if plain is not None:
                d_plain = torch.empty((n, 8), dtype=torch.int32, device="cuda")
                d_plain_cnt = torch.empty(n, dtype=torch.int32, device="cuda")
                p = time_cell(lambda: plain.triangles_in_boxes_into(d_boxes.data_ptr(), n, d_plain.data_ptr() if k else 0, d_plain_cnt.data_ptr(),
                                                                    k, any_only, stream.cuda_stream))
                r = {"instance": r, "scene": p, "instance_over_scene": round(r["ms"] / p["ms"], 3),
                     "same_answer": bool(torch.equal(d_cnt, d_plain_cnt)) and (k == 0 or bool(torch.equal(d_out, d_plain)))}
                del d_plain, d_plain_cnt
            cell[name] = r
            print(f"  {what}, {name}: {r}", file=sys.stderr, flush=True)
        return cell

    def boxes_of(positions, maps, extent, rng):
        """(grid cells, 5 % boxes) as [n, 8] tensors, for the scene's positions placed by `maps`"""
        lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
        for M in maps:
            w = IP.map_corners(M, positions)
            lo, hi = np.minimum(lo, w.min(0)), np.maximum(hi, w.max(0))
        lo, hi = lo.astype(F), hi.astype(F)
        cell = ((hi - lo) / F(GRID)).astype(F)
        slabs = n // (GRID * GRID)                                      # a contiguous run of the grid: its middle slabs
        first = (GRID - slabs) // 2
        origin = (lo + F(first) * cell * np.array([1, 0, 0], F)).astype(F)
        d_grid = pkg.tracer.voxel_boxes(origin, cell, (slabs, GRID, GRID), device="cuda")
        assert len(d_grid) == n
        tris = positions.reshape(-1, 3, 3)
        t, i = rng.integers(0, len(tris), n), rng.integers(0, len(maps), n)
        w = rng.random((n, 3)).astype(F)
        w /= w.sum(1, keepdims=True)
        on = (tris[t] * w[:, :, None]).sum(1).astype(np.float64)
        A = np.asarray(maps, np.float64)[i]
        centre = np.einsum("nrc,nc->nr", A[:, :, :3], on) + A[:, :, 3]
        half = 0.025 * extent
        d_near = H.upload(pkg.tracer.make_boxes(centre - half, centre + half), 8)
        return d_grid, d_near

    out = {"trials": args.trials, "warmup": args.warmup, "boxes": n, "device": torch.cuda.get_device_name(0)}
    rng = np.random.default_rng(2026)
    with H.bunny_scene(pkg) as (world, bunny, positions):
        verts = positions.reshape(-1, 3).astype(np.float64)
        extent = float(np.linalg.norm(verts.max(0) - verts.min(0)))
        out["triangles"] = len(positions) // 9

        eye = np.eye(3, 4, dtype=F)[None]
        one = pkg.tracer.InstanceSet([bunny], eye)
        d_grid, d_near = boxes_of(positions, eye, extent, rng)
        out["a_identity"] = {f"grid{GRID}": cells(one, bunny, d_grid, "one identity instance, grid cells"),
                             "surface_5pct": cells(one, bunny, d_near, "one identity instance, 5 % boxes")}
        one.close()

        M = grid_transforms((8, 8), 1.5 * float(np.ptp(verts, axis=0).max()), np.random.default_rng(2026))
        grid = pkg.tracer.InstanceSet([bunny] * 64, M)
        d_grid, d_near = boxes_of(positions, M, extent, rng)
        out["b_bunny_8x8"] = {f"grid{GRID}": cells(grid, None, d_grid, "64 copies, grid cells"),
                              "surface_5pct": cells(grid, None, d_near, "64 copies, 5 % boxes")}
        grid.close()
    H.emit(out, args)


if __name__ == "__main__":
    main()
