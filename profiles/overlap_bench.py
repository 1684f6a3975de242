"""Box-overlap query throughput (include/shader_ray_overlap.h), one JSON line on stdout.

Scenes: the bunny-class scene and the 1M-triangle OBJ.  Boxes: 2^20 voxel cells of a 128^3 and of a 256^3 grid over the
scene's box (a contiguous 2^20 run of the grid from its middle slab, in grid order, and the same cells shuffled), and 2^20 boxes
of 5 % of the extent around surface points.  Forms: counts only (K = 0), K = 8 with counts, and SHRAY_OVERLAP_ANY.

Every time is the median of --trials launches after --warmup launches, bracketed by HIP events on the current torch stream.
The mean and maximum of n and the counters per box (node visits, i.e. box tests evaluated, leaf visits, triangle tests) come
from one blocking counting run of 2^12 of the boxes, for the counting form and for ANY.

  torch_vs_k8   K = 8 with counts on 2^12 of the 5 % boxes against the restatement's arithmetic in plain fp32 torch on the GPU
                (every box against every triangle: what a caller would write without this query)

Usage: python profiles/overlap_bench.py [--trials 15] [--warmup 5] [--no-million]"""
import ctypes as C
import sys

import numpy as np

import bench_harness as H

F = np.float32
COUNT = 1 << 20


def torch_overlap(pos, boxes, k):
    """the header's test in fp32 torch, every box against every triangle: (indices [n, k], counts [n])"""
    import torch
    tri = pos.reshape(-1, 3, 3)
    a, b, c = tri[None, :, 0], tri[None, :, 1], tri[None, :, 2]
    lo, hi = boxes[:, None, 0:3], boxes[:, None, 4:7]

    def mn(x, y):
        return torch.where(x < y, x, y)

    def mx(x, y):
        return torch.where(x > y, x, y)

    sep = ((mn(mn(a, b), c) > hi) | (mx(mx(a, b), c) < lo)).any(2)
    m, h = 0.5 * lo + 0.5 * hi, 0.5 * hi - 0.5 * lo
    v0, v1, v2 = a - m, b - m, c - m
    e0, e1, e2 = v1 - v0, v2 - v1, v0 - v2
    nx = e0[..., 1] * e1[..., 2] - e0[..., 2] * e1[..., 1]
    ny = e0[..., 2] * e1[..., 0] - e0[..., 0] * e1[..., 2]
    nz = e0[..., 0] * e1[..., 1] - e0[..., 1] * e1[..., 0]
    d = (nx * v0[..., 0] + ny * v0[..., 1]) + nz * v0[..., 2]
    r = (h[..., 0] * nx.abs() + h[..., 1] * ny.abs()) + h[..., 2] * nz.abs()
    sep |= (d > r) | (d < -r)
    for e in (e0, e1, e2):
        for u, w in ((1, 2), (2, 0), (0, 1)):
            p = [e[..., u] * v[..., w] - e[..., w] * v[..., u] for v in (v0, v1, v2)]
            r = h[..., u] * e[..., w].abs() + h[..., w] * e[..., u].abs()
            sep |= (mn(mn(p[0], p[1]), p[2]) > r) | (mx(mx(p[0], p[1]), p[2]) < -r)
    walked = torch.isfinite(boxes).all(1) & ~(boxes[:, 0:3] > boxes[:, 4:7]).any(1)
    member = ~sep & walked[:, None]
    index = torch.where(member, torch.arange(member.shape[1], device=member.device)[None], torch.iinfo(torch.int32).max)
    first = torch.sort(index, 1).values[:, :k]
    return torch.where(first == torch.iinfo(torch.int32).max, -1, first).int(), member.sum(1).int()


def main():
    ap = H.parser()
    ap.add_argument("--no-million", action="store_true")
    args = ap.parse_args()
    import torch

    pkg = H.load_package()
    N = pkg._native
    lib = N.load_overlap()
    stream = torch.cuda.current_stream()
    median_ms = H.median_timer(args, slow_ms=500.0)

    def entry(boxes, t):
        return H.entry(t, "Mboxes_s", boxes, boxes=boxes)

    def launcher(scene, d_boxes, k, any_only, d_out, d_cnt):
        op = pkg.tracer.overlap_params(k, any_only)

        def launch():
            N.check(lib.shray_overlap_triangles_device(scene._handle, C.byref(op), C.c_void_p(d_boxes.data_ptr()), len(d_boxes),
                                                       C.c_void_p(d_out.data_ptr() if k else None), C.c_void_p(d_cnt.data_ptr()),
                                                       C.c_void_p(stream.cuda_stream)))
        return launch

    def forms(scene, d_boxes):
        d_out = torch.empty((len(d_boxes), 8), dtype=torch.int32, device="cuda")
        d_cnt = torch.empty(len(d_boxes), dtype=torch.int32, device="cuda")
        sample = d_boxes[torch.from_numpy(np.random.default_rng(5).permutation(len(d_boxes))[:1 << 12]).cuda()].cpu().numpy()
        row = {}
        for name, any_only in (("counting", False), ("any", True)):
            _, cnt, c = scene.triangles_in_boxes(sample, max_triangles=0, counters=True, any_only=any_only)
            row[f"per_box_{name}"] = {k: round(c[k] / len(sample), 2) for k in ("node_visits", "leaf_visits", "triangle_tests")}
            if not any_only:
                row["n_mean"], row["n_max"], row["touched"] = round(float(cnt.mean()), 2), int(cnt.max()), round(float((cnt > 0).mean()), 4)
        row["counts_only"] = entry(len(d_boxes), median_ms(launcher(scene, d_boxes, 0, False, d_out, d_cnt)))
        row["K8_counts"] = entry(len(d_boxes), median_ms(launcher(scene, d_boxes, 8, False, d_out, d_cnt)))
        row["any"] = entry(len(d_boxes), median_ms(launcher(scene, d_boxes, 0, True, d_out, d_cnt)))
        row["any_over_counts_only"] = round(row["any"]["ms"] / row["counts_only"]["ms"], 4)
        print(f"  {row['counts_only']['ms']} / {row['K8_counts']['ms']} / {row['any']['ms']} ms", file=sys.stderr, flush=True)
        return row

    def scene_cases(scene, pos):
        verts = pos.reshape(-1, 3)
        lo, hi = verts.min(0), verts.max(0)
        extent = float(np.linalg.norm(hi - lo))
        res = {}
        for g in (128, 256):
            cell = ((hi - lo) / F(g)).astype(F)
            slabs = COUNT // (g * g)                                  # a contiguous run of the grid: its middle slabs
            first = (g - slabs) // 2
            origin = (lo + F(first) * cell * np.array([1, 0, 0], F)).astype(F)
            d_boxes = pkg.tracer.voxel_boxes(origin, cell, (slabs, g, g), device="cuda")
            assert len(d_boxes) == COUNT
            res[f"grid{g}_in_order"] = forms(scene, d_boxes)
            shuffled = d_boxes[torch.from_numpy(np.random.default_rng(9).permutation(COUNT)).cuda()].contiguous()
            res[f"grid{g}_shuffled"] = forms(scene, shuffled)
        rng = np.random.default_rng(3)
        tris = pos.reshape(-1, 3, 3)
        t = rng.integers(0, len(tris), COUNT)
        w = rng.random((COUNT, 3)).astype(F)
        w /= w.sum(1, keepdims=True)
        centre = (tris[t] * w[:, :, None]).sum(1)
        half = F(0.025 * extent)
        d_near = H.upload(pkg.tracer.make_boxes(centre - half, centre + half), 8)
        res["surface_5pct"] = forms(scene, d_near)
        return res, d_near

    out = {"trials": args.trials, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}
    with H.bunny_scene(pkg) as (world, scene, pos):
        out["bunny"], d_near = scene_cases(scene, pos)
        out["bunny"]["triangles"] = len(pos) // 9

        # what a caller would write today: every box against every triangle in torch, on 2^12 of the 5 % boxes
        few = d_near[: 1 << 12].contiguous()
        d_pos = torch.from_numpy(pos).cuda()
        want, want_n = torch_overlap(d_pos, few, 8)
        got, got_n = scene.triangles_in_boxes(few, max_triangles=8)
        assert bool((got == want).all()) and bool((got_n == want_n).all())
        d_out = torch.empty((len(few), 8), dtype=torch.int32, device="cuda")
        d_cnt = torch.empty(len(few), dtype=torch.int32, device="cuda")
        ours = entry(len(few), median_ms(launcher(scene, few, 8, False, d_out, d_cnt)))
        brute = entry(len(few), median_ms(lambda: torch_overlap(d_pos, few, 8)))
        out["torch_vs_k8"] = {"kernel": ours, "torch": brute, "torch_over_kernel": round(brute["ms"] / ours["ms"], 2)}

    if not args.no_million:
        dw = pkg.tracer.DeviceWorld(pkg.scenes.million_obj())
        pos = np.asarray(dw.flat_arrays()["vertex_positions"], F)
        out["million"], _ = scene_cases(dw.scene, pos)
        out["million"]["triangles"] = len(pos) // 9
        dw.close()
    H.emit(out, args)


if __name__ == "__main__":
    main()
