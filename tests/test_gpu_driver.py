"""GPU tests of the callers around the hot path: the headless animation /
benchmark-histogram driver (ray.cpp:91-98, :791-918, :1096-1131), the blocking and the pinned
readback forms of the C ABI (ray.cpp:760), and BASELINE config 4 at its full size."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import helpers
from helpers import assert_images_match

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
EXE = os.path.join(ROOT, "shader-ray_amd", "tools", "shray_render")


def test_animation_driver_frames_and_histogram(pkg, gpu, tmp_path):
    """`shray_render -n 30`: every frame of the trackball animation equals a batch render
    (shray_render_batch_device) of the same drag sequence replayed through the host C ABI, and
    the benchmark print-out is the reference's ten-bucket histogram over all 30 frames."""
    import torch
    if not os.path.exists(EXE):
        subprocess.run(["make", "-C", os.path.dirname(os.path.dirname(EXE)), "tools"], check=True, stdout=subprocess.DEVNULL)
    model = os.path.join(GOLDEN, "lobed_528.trisrc")
    W, H, frames = 96, 64, 30
    prefix = str(tmp_path / "frame")
    run = subprocess.run([EXE, model, "grid", "-o", str(tmp_path / "last.ppm"), "-w", str(W), "-h", str(H), "-n", str(frames),
                          "-f", prefix], check=True, capture_output=True, text=True)

    # the reference's print-out (ray.cpp:1116-1131): "N frames:" then ten "a to b ms, f fps : count" lines
    lines = run.stdout.strip().splitlines()
    assert lines[0] == f"{frames} frames:" and len(lines) == 11
    counts, edges = [], []
    for line in lines[1:]:
        m = re.fullmatch(r"([\d.]+) to ([\d.]+) ms, ([\d.]+) fps : (\d+)", line)
        assert m, line
        lo, hi, fps, count = float(m.group(1)), float(m.group(2)), float(m.group(3)), int(m.group(4))
        assert lo <= hi and fps > 0
        edges.append((lo, hi))
        counts.append(count)
    assert sum(counts) == frames and counts[0] >= 1 and counts[-1] >= 1
    assert all(abs(edges[k][1] - edges[k + 1][0]) < 0.011 for k in range(9))

    # replay the drag sequence of tools/shray_render.cpp: object for the first half, light for the second,
    # next material after frame 24
    world = pkg.World(model)
    scene = pkg.Scene(world.flatten(), pkg.load_background("grid"), device=0)
    view = world.default_view()
    params = []
    for frame in range(frames):
        target = view.object_rotation if frame < frames // 2 else view.light_rotation
        pkg.host.trackball_motion(target, 0.011, 0.004)
        if frame % 25 == 24:
            view.which_material = (view.which_material + 1) % 7
        params.append(world.frame_params(W, H, view))
    assert params[0].object_matrix[:] != params[1].object_matrix[:]
    assert params[-1].light_dir[:] != params[frames // 2 - 1].light_dir[:]
    assert params[-1].specular_color[:] != params[0].specular_color[:]
    out = torch.empty((frames, H, W, 4), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    for first in range(0, frames, 16):
        chunk = params[first:first + 16]
        scene.render_batch_into(chunk, W, H, 1, out[first].data_ptr(), H * W * 16, stream)
    torch.cuda.synchronize()
    want = out.cpu().numpy()
    for frame in range(frames):
        got = np.fromfile(f"{prefix}{frame:03d}.rgba", dtype=np.float32).reshape(H, W, 4)
        assert np.array_equal(got, want[frame]), f"animation frame {frame} differs from the batch render"
    # and the saved picture is the last frame, 8 bits, top row first
    blob = open(tmp_path / "last.ppm", "rb").read().split(b"\n", 1)[1]
    assert np.array_equal(np.frombuffer(blob, np.uint8).reshape(H, W, 3),
                          (np.clip(want[-1][::-1, :, :3], 0, 1) * 255.0 + 0.5).astype(np.uint8))
    scene.close()


def test_readback_forms_return_the_device_frame(pkg, gpu):
    """shray_render into pageable memory (fresh and reused buffers), into pinned memory (one DMA) and
    shray_render_host_async all deliver the frame shray_render_device leaves on the GPU; the
    scene's frame buffer is reused across sizes."""
    import torch
    from shader_ray_amd.tracer import PinnedFrame
    world = pkg.World(os.path.join(GOLDEN, "lobed_528.trisrc"))
    scene = pkg.Scene(world.flatten(), pkg.scenes.environment_hdr_sky(128), device=0)
    stream = torch.cuda.current_stream().cuda_stream
    for W, H, spp in ((333, 77, 1), (640, 360, 2), (64, 64, 1)):
        params = world.frame_params(W, H, material=6)
        dev = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
        scene.render_into(params, W, H, spp, dev.data_ptr(), stream)
        torch.cuda.synchronize()
        want = dev.cpu().numpy()
        assert np.array_equal(scene.render(params, W, H, spp), want)
        mine = np.full((H, W, 4), -1.0, dtype=np.float32)      # a frame loop's own buffer, filled in place
        assert scene.render(params, W, H, spp, out=mine) is mine and np.array_equal(mine, want)
        with pytest.raises(ValueError):
            scene.render(params, W, H, spp, out=np.empty((H, W, 3), dtype=np.float32))
        pinned = PinnedFrame(W, H)
        pinned.array[:] = -1.0
        got = scene.render_to_pinned(params, W, H, spp, pinned, stream, wait=True)
        assert np.array_equal(got, want)
        # blocking form straight into pinned memory
        pinned.array[:] = -1.0
        lib = pkg._native.load_hip()
        import ctypes as C
        pkg._native.check(lib.shray_render(scene._handle, C.byref(params), W, H, spp,
                                           C.cast(C.c_void_p(pinned.ptr), pkg._native.c_float_p)))
        assert np.array_equal(pinned.array, want)
        pinned.close()
    # pageable memory is refused by the asynchronous form, with a message
    import ctypes as C
    page = np.empty((64, 64, 4), np.float32)
    rc = pkg._native.load_hip().shray_render_host_async(scene._handle, C.byref(world.frame_params(64, 64)), 64, 64, 1,
                                                        C.c_void_p(page.ctypes.data), C.c_void_p(stream))
    assert rc == -1 and b"pinned" in pkg._native.load_hip().shray_last_error()
    scene.close()


def test_config4_full_size_million_triangles_4spp(pkg, gpu, oracle_mod):
    """BASELINE config 4 at its full size: 1M-triangle OBJ (obj-support.cpp:104-146 normals), deep BVH,
    1920x1080, 4 spp, against a full-frame oracle render (seconds on the GPU box's host cores): every
    float bit-identical, every work counter equal -- including the samples that hit the 400-iteration
    cap (raytracer.es.fs:381, :436-438) -- for the stack kernel, its plain twin and the literal kernel."""
    world = pkg.World(helpers.million_obj())
    desc = world.flatten()
    env = pkg.scenes.environment_hdr_sky(512)
    scene = pkg.Scene(desc, env, device=0)
    W, H, spp = 1920, 1080, 4
    params = world.frame_params(W, H, material=0)
    want, cpu = oracle_mod.render(desc, env, params, W, H, spp)
    assert cpu["samples"] == W * H * spp and cpu["traversals"] > cpu["samples"]
    # the cap is 'a little too few' for this tree: a few samples per 100,000 hit it
    fraction = cpu["bad_hits"] / cpu["samples"]
    assert 0 < fraction < 1e-3, fraction
    for kernel in (0, 1, 3, 4):  # 3: both children per turn (its counting twin reproduces the capped samples' tallies too); 4: wavefront form
        scene.set_kernel(kernel)
        got, counters = scene.render_counters(params, W, H, spp)
        assert_images_match(got, want, f"config 4 kernel {kernel}")
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"config 4 kernel {kernel}: not bit-identical"
        assert counters == cpu, f"config 4 kernel {kernel}: {counters} != {cpu}"
        if kernel != 1:
            assert np.array_equal(scene.render(params, W, H, spp), got)
    scene.set_kernel(0)
    assert np.all(want[..., 3] == 1.0) and not np.isnan(want).any()
    scene.close()


def test_uneven_rank_shares_on_one_gpu(pkg, gpu):
    """Rank 0 owns fewer tiles than its peers (shray_tile_set.tile_phase_count, shray_assemble_tiles_split_device):
    every rank's tile set rendered on this GPU, RGB on the wire, de-interleaved by the split kernel -- the frames
    equal full-frame renders bit for bit; so does BASELINE config 5's shape (8 ranks, balanced shares) at 960x540."""
    import ctypes as C
    import torch
    from shader_ray_amd import multigpu
    N = pkg._native
    world = pkg.World(os.path.join(GOLDEN, "lobed_528.trisrc"))
    scene = pkg.Scene(world.flatten(), pkg.scenes.environment_hdr_sky(128), device=0)
    stream = torch.cuda.current_stream().cuda_stream
    for (W, H, tile, ranks, shares, spp) in ((200, 136, 32, 3, (2, 3), 1), (333, 100, 16, 4, (3, 4), 2),
                                             (960, 540, 32, 8, multigpu.balanced_shares(8), 4), (96, 64, 32, 2, (1, 5), 1)):
        frames = [world.frame_params(W, H, material=m) for m in (0, 6)]
        want = [scene.render(p, W, H, spp) for p in frames]
        per = multigpu.max_tiles_per_rank(W, H, tile, tile, ranks, shares)
        pixels = per * tile * tile
        gathered = torch.zeros(ranks, 2, pixels * 3, dtype=torch.float32, device="cuda:0")
        rgba = torch.zeros(2, pixels * 4, dtype=torch.float32, device="cuda:0")
        for r in range(ranks):
            period, phase, count = multigpu.rank_phases(ranks, r, shares)
            tiles = N.TileSet(tile, tile, period, phase, count)
            assert pkg.tracer.tile_buffer_bytes(W, H, tiles) <= pixels * 16
            rgba.zero_()
            scene.render_batch_into(frames, W, H, spp, rgba.data_ptr(), pixels * 16, stream, tiles)
            gathered[r].view(2, pixels, 3).copy_(rgba.view(2, pixels, 4)[:, :, :3])
        out = torch.zeros(2, H, W, 4, dtype=torch.float32, device="cuda:0")
        N.check(N.load_hip().shray_assemble_tiles_split_device(
            C.c_void_p(gathered.data_ptr()), ranks, shares[0], shares[1], 2, 3, gathered.stride(0) * 4, gathered.stride(1) * 4,
            W, H, tile, tile, C.c_void_p(out.data_ptr()), C.c_void_p(stream)))
        torch.cuda.synchronize()
        for k in range(2):
            assert np.array_equal(out[k].cpu().numpy(), want[k]), (W, H, tile, ranks, shares, k)
    # the object the bench uses, one rank: shares collapse to (1, 1)
    one = multigpu.plan(multigpu.make_config(0, 1, 64, 64))
    assert (one.rank0_phases, one.other_phases) == (1, 1)
    with pytest.raises(N.ShrayError):
        scene.render_into(world.frame_params(64, 64), 64, 64, 1, out.data_ptr(), stream, N.TileSet(32, 32, 4, 3, 2))
    scene.close()


@pytest.mark.parametrize("material", [0, 6])
def test_shader_constants_as_parameters(pkg, gpu, oracle_mod, material):
    """The shader's compile-time constants are frame parameters here (raytracer.es.fs:550, :381, :382, :445): the
    convergent bounce loop and the dealt leaf stage follow them exactly like the oracle does -- no bounce at all,
    two bounces, a leaf cap of 3 and of 0, a tight iteration cap, no shadow rays -- frames and counters equal for
    every kernel."""
    world = pkg.World(os.path.join(GOLDEN, "lobed_528.trisrc"))
    desc = world.flatten()
    env = pkg.scenes.environment_hdr_sky(128)
    scene = pkg.Scene(desc, env, device=0)
    W, H = 120, 72
    variants = [dict(bounce_count=0), dict(bounce_count=2), dict(max_leaf_tests=3), dict(max_leaf_tests=0),
                dict(max_bvh_iterations=12), dict(cast_shadows=0, bounce_count=5), dict(tonemap=0)]
    for spp in (1, 2, 7):   # 2 and 7: sample lanes in pairs and in fours, the last round not full (uniform_driver.h)
        for overrides in variants:
            params = world.frame_params(W, H, material=material)
            for key, value in overrides.items():
                setattr(params, key, value)
            want, cpu = oracle_mod.render(desc, env, params, W, H, spp)
            for kernel in (0, 1, 2, 3, 4):
                scene.set_kernel(kernel)
                got, counters = scene.render_counters(params, W, H, spp)
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (overrides, spp, kernel)
                assert counters == cpu, (overrides, spp, kernel)
                assert np.array_equal(scene.render(params, W, H, spp), got), (overrides, spp, kernel)
    scene.set_kernel(0)
    scene.close()


def test_bench_line_carries_the_frozen_roofline_object(gpu):
    """`python bench.py --full` (N = 1) prints ONE line whose `roofline` has the round-5 definition: hbm / vmem / valu, each
    achieved over peak, the top-level pair = the largest of the three; its instruction and byte counts come from `rocprofv3 --pmc`
    passes the command runs on its own child processes in the same invocation, and agree with the committed counter file of the same
    device code to a fraction of a per cent (the counts of a deterministic kernel)."""
    import json
    bench = os.path.join(ROOT, "bench.py")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    run = subprocess.run([sys.executable, bench, "--full", "--steps", "20", "--warmup", "4", "--trials", "3", "--no-cpu-baseline"], env=env,
                         capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-3000:]
    lines = [ln for ln in run.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    line = json.loads(lines[0])
    roof = line["roofline"]
    assert line["value"] > 1000 and line["frames_mismatched"] == 0 and line["unit"] == "Mrays/s"
    fracs = {"hbm": roof["hbm"]["frac_measured"], "vmem": roof["vmem"]["frac"], "valu": roof["valu"]["frac"]}
    assert all(0.0 < f < 1.0 for f in fracs.values()), fracs
    assert roof["bound"] == max(fracs, key=fracs.get) and roof["frac"] == fracs[roof["bound"]]
    assert abs(roof["achieved"] / roof["peak"] - roof["frac"]) < 1e-3 and roof["traffic"] > 0
    assert roof["hbm"]["algorithmic_over_peak"] > 1.0 and roof["vmem"]["frac_scattered"] > roof["vmem"]["frac"] > roof["vmem"]["frac_at_one_record_peak"]
    assert roof["counter_source"].startswith("rocprofv3 --pmc passes of this invocation"), roof["counter_source"]
    agree = roof.get("archived_counters_agree")
    if agree:       # the committed counter file is of this build: the same counts
        assert all(abs(v - 1.0) < 0.01 for v in agree.values()), agree
    assert not any(key.endswith("_busy") for key in roof if key != "busy_profiled")


def test_plain_bench_line_and_its_dumped_outputs(pkg, gpu, tmp_path):
    """A plain `python bench.py` times exactly --steps steps once and carries only the headline fields; --dump-outputs writes
    the last timed frame, which is the one-frame render of that step's view of the orbit, bit for bit."""
    import json
    W, H, steps = 320, 180, 7
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    out = tmp_path / "dump"
    run = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "2",
                          "--width", str(W), "--height", str(H), "--dump-outputs", str(out)], env=env, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-3000:]
    lines = [ln for ln in run.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["unit"] == "Mrays/s" and line["higher_is_better"] is True and line["dtype"] == "f32" and line["value"] > 0
    assert line["steps"] == steps and line["trials"] == 1 and len(line["trial_ms"]) == 1
    assert abs(line["ms_per_step"] - line["trial_ms"][0] / steps) < 1e-3
    assert "roofline" not in line and "cpu_baseline" not in line and "latency" not in line
    assert sorted(os.listdir(out)) == ["frame.npy"]
    frame = np.load(out / "frame.npy")
    assert frame.dtype == np.float32 and frame.shape == (H, W, 4)
    # bench.py's orbit: the start-up view dragged (0.025, 0.010) further every frame; step k renders view k % 20
    world = pkg.World(pkg.scenes.bunny_trisrc())
    view = world.default_view()
    view.which_material = 0
    for _ in range(steps):
        pkg.host.trackball_motion(view.object_rotation, 0.025, 0.010)
    scene = pkg.Scene(world.flatten(), pkg.scenes.environment_hdr_sky(2048), device=0)
    assert np.array_equal(frame, scene.render(world.frame_params(W, H, view), W, H, 1))
    scene.close()
