"""The one-leaf sequential loop (csrc/leaf_asm.h, SHRAY_LEAF_UNIFORM): a crowded leaf stage -- more than 32 lanes of a wave parked --
whose parked lanes are all in ONE leaf fetches each triangle once, through the scalar cache, and tests it with the triangle's words as
scalar operands; the next round's triangle is asked for a round ahead.  Scenes built so that this loop is certainly taken and its
edges are met; every frame is compared bit for bit with the CPU oracle AND with kernel 1 (the literal threaded kernel, which has no
leaf stage at all), through the three timed forms of kernel 0 -- one frame per launch, two and four frames per launch (the
throughput form the benchmark times) -- and its counting twin, whose tallies must be the oracle's.

The look-ahead and the end of the triangle array: the LAST round of a leaf asks for nothing (the loader does not pad), so the loop
never reads past the last record.  In every single-leaf scene below the leaf's last triangle is the array's last record."""
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
from helpers import END, HandScene, default_params, single_leaf_scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOUNIFORM = os.path.join(ROOT, "shader-ray_amd", "_variants", "libshray_hip_nouniform.so")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check_every_form(pkg, oracle_mod, hand, env, params, W, H, spp, what):
    """Oracle == kernel 1 == kernel 0 (one, two and four frames per launch, and the counting twin), bit for bit."""
    import torch
    want, cpu = oracle_mod.render(hand.desc, env, params, W, H, spp)
    scene = pkg.Scene(hand.desc, env, device=0)
    try:
        scene.set_kernel(1)
        literal, literal_counters = scene.render_counters(params, W, H, spp)
        assert np.array_equal(bits(literal), bits(want)), f"{what}: kernel 1 against the oracle"
        assert literal_counters == cpu, (what, literal_counters, cpu)
        scene.set_kernel(0)
        got = scene.render(params, W, H, spp)
        assert np.array_equal(bits(got), bits(want)), f"{what}: one frame per launch against the oracle"
        assert np.array_equal(bits(got), bits(literal)), f"{what}: one frame per launch against kernel 1"
        stream = torch.cuda.current_stream().cuda_stream
        for count in (2, 4):
            out = torch.zeros(count, H, W, 4, dtype=torch.float32, device="cuda")
            scene.render_batch_into([params] * count, W, H, spp, out.data_ptr(), H * W * 16, stream)
            torch.cuda.synchronize()
            for k in range(count):
                frame = out[k].cpu().numpy()
                assert np.array_equal(bits(frame), bits(want)), f"{what}: frame {k} of {count} per launch against the oracle"
                assert np.array_equal(bits(frame), bits(literal)), f"{what}: frame {k} of {count} per launch against kernel 1"
        counted, counters = scene.render_counters(params, W, H, spp)
        assert np.array_equal(bits(counted), bits(want)) and counters == cpu, (what, counters, cpu)
    finally:
        scene.set_kernel(0)
        scene.close()
    return want, cpu


def stacked(count):
    """`count` triangles that fill the view, the nearest neither first nor last where there is room, one of them tilted (its
    barycentric tests fail over part of the frame) and one small (most lanes leave the round at the barycentrics)."""
    zs = [-0.25 * ((k * 7) % 11) for k in range(count)]
    tris = [[[-5, -5, z], [5, -5, z], [0, 5, z]] for z in zs]
    if count >= 2:
        tris[1] = [[-5, -5, 0.5], [5, -5, -0.5], [0, 5, 0.2]]
    if count >= 10:
        tris[7] = [[-0.3, -0.3, 0.9], [0.4, -0.3, 0.9], [0.0, 0.5, 0.9]]
    return tris


@pytest.mark.parametrize("count", [1, 2, 10, 11])
def test_a_view_filled_by_one_leaf(pkg, gpu, oracle_mod, count):
    """Every pixel's ray enters the scene's only leaf: every wave's primary stage has 64 lanes parked in one leaf.  Leaves of 1, 2,
    10 and 11 triangles under the shader's cap of 10 tests per leaf, and under a cap of 11 (the eleventh is then tested too):
    an odd and an even number of rounds, so the loop ends in either of its two register sets."""
    env = pkg.scenes.environment_constant((0.5, 0.25, 2.0))
    hand = single_leaf_scene(stacked(count))
    for material, spp in ((0, 1), (6, 2)):
        for cap in (10, 11):
            params = default_params(pkg, 48, 32, zoom=4.0, material=material)
            params.max_leaf_tests = cap
            _, cpu = check_every_form(pkg, oracle_mod, hand, env, params, 48, 32, spp, f"{count} triangles, cap {cap}, material {material}")
            assert cpu["triangle_tests"] >= min(count, cap) * 48 * 32 * spp     # (every primary ray tests the whole leaf)


def two_leaf_scene():
    """A branch split on x with a leaf on either side; the leaves' boxes overlap in a narrow band around x = 0, so the waves in the
    middle columns of the frame park lanes in BOTH leaves (the stage must take the per-lane loop) next to waves in one."""
    import test_oracle_kat as kat
    left = [[[-6, -5, z], [0.2, -5, z], [-3, 5, z]] for z in (-0.5, 0.25, -1.0)]
    right = [[[-0.2, -5, z], [6, -5, z], [3, 5, z]] for z in (0.0, -0.75, 0.5, -0.25, -1.5)]
    pts = np.asarray(left + right, dtype=np.float32).reshape(-1, 3)
    normals = np.tile(np.asarray([0, 0, 1], np.float32), (len(pts), 1))
    hm = kat.thread_tree([1, -1, -1], [2, -1, -1], [0, 0, 0], 0)
    lo = [[-6.5, -6, -2], [-6.5, -6, -2], [-0.25, -6, -2]]
    hi = [[6.5, 6, 1], [0.25, 6, 1], [6.5, 6, 1]]
    return HandScene(pts, normals, lo, hi, hm, [[0, 0], [0, len(left)], [len(left), len(right)]], 0)


def test_waves_in_two_leaves_beside_waves_in_one(pkg, gpu, oracle_mod):
    env = pkg.scenes.environment_constant((0.5, 0.25, 2.0))
    hand = two_leaf_scene()
    for material, spp in ((0, 1), (6, 2)):
        for zoom in (4.0, 6.0):
            params = default_params(pkg, 64, 32, zoom=zoom, material=material)
            _, cpu = check_every_form(pkg, oracle_mod, hand, env, params, 64, 32, spp, f"two leaves, zoom {zoom}, material {material}")
            assert cpu["leaf_visits"] > 64 * 32 * spp       # (both leaves are visited)


def test_slow_rounds_inside_a_one_leaf_stage(pkg, gpu, oracle_mod):
    """A triangle whose determinant is outside the reciprocal's domain (infinite: the huge triangle of test_oracle_kat) leaves the
    statement; its candidate is NaN in every field and is accepted by the compiler's round, and the loop goes back into the one-leaf
    loop at the next round -- with the right round number and the right address: the huge triangle first, last, in the middle,
    twice in a row and alone in its leaf.  The leaf's box fills the view, so every wave's stage is crowded and one-leaf."""
    import test_oracle_kat as kat
    env = pkg.scenes.environment_constant((0.5, 0.25, 2.0))
    for order in kat.NAN_ORDERS:
        hand = kat.nan_leaf_scene(order, half=3.0)
        for material, bounces in ((0, 1), (0, 3), (6, 3)):
            params = default_params(pkg, 32, 32, zoom=4.0, material=material)
            params.bounce_count = bounces
            want, cpu = check_every_form(pkg, oracle_mod, hand, env, params, 32, 32, 1, f"order {order}, material {material}, {bounces} bounce(s)")
            assert not np.isnan(want).any()
            assert cpu["triangle_tests"] >= len(order) * 32 * 32


def test_candidates_at_the_ends_of_the_parked_bounds(pkg, gpu, oracle_mod):
    """The construction of test_gpu_parity.py::test_triangles_at_the_ends_of_a_leaf_range (triangles a few 1e-7 in front of, on and
    behind the near and the far face of a hand-built leaf box), here with every lane of every wave parked in that one leaf: a
    candidate within 2^-19 of an end of the parked bounds leaves the one-leaf loop and the exact range decides."""
    env = pkg.scenes.environment_constant((0.5, 0.25, 2.0))

    def leaf(zs, box_z):
        tris = [[[-5, -5, z], [5, -5, z], [0, 5, z]] for z in zs]
        pts = np.asarray(tris, dtype=np.float32).reshape(-1, 3)
        normals = np.tile(np.asarray([0, 0, 1], np.float32), (len(pts), 1))
        hm = np.full((8, 1, 2), END, dtype=np.float32)
        return HandScene(pts, normals, [[-6, -6, box_z[0]]], [[6, 6, box_z[1]]], hm, [[0, len(zs)]], 0)

    near = leaf([1e-5, 3e-6, 1e-6, 3e-7, 1e-7, 0.0, -1e-7, -0.5], (-1.0, 0.0))
    far = leaf([-1.0 - 1e-6, -1.0 - 3e-7, -1.0 - 1e-7, -1.0, -1.0 + 1e-7], (-1.0, 0.0))
    last_only = leaf([-0.5, -0.25, 1e-7], (-1.0, 0.0))          # the slow round is the leaf's last
    first_only = leaf([1e-7, -0.25, -0.5], (-1.0, 0.0))         # ... and its first
    hit = {}
    for what, hand in (("near face", near), ("far face", far), ("last round", last_only), ("first round", first_only)):
        for material, spp in ((0, 1), (6, 2)):
            for zoom in (3.0, 2.9999998):
                params = default_params(pkg, 48, 32, zoom=zoom, material=material)
                want, _ = check_every_form(pkg, oracle_mod, hand, env, params, 48, 32, spp, f"{what} {material} {zoom}")
                hit[(what, material, zoom)] = float((np.abs(want[..., :3] - want[0, 0, :3]).max(axis=-1) > 1e-6).mean())
    assert min(v for k, v in hit.items() if k[1] == 0) > 0.5     # (not vacuous: the scenes are hit over most of the frame)


CHILD = r"""
import sys, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from __graft_entry__ import load_package
import bench
pkg = load_package()
world = pkg.World(pkg.scenes.bunny_trisrc())
scene = pkg.Scene(world.flatten(), pkg.scenes.environment_hdr_sky(2048), device=0)
scene.set_kernel(0)
orbit = bench.orbit_params(pkg, world, bench.WIDTH, bench.HEIGHT)
stream = torch.cuda.current_stream().cuda_stream
for first in range(0, bench.ORBIT, 4):
    out = torch.zeros(4, bench.HEIGHT, bench.WIDTH, 4, dtype=torch.float32, device="cuda")
    scene.render_batch_into(orbit[first:first + 4], bench.WIDTH, bench.HEIGHT, 1, out.data_ptr(), bench.HEIGHT * bench.WIDTH * 16, stream)
    torch.cuda.synchronize()
    torch.save(out.cpu(), sys.argv[2] + f"/views_{first}.pt")
scene.close()
print("views written")
"""


def test_the_orbit_against_the_build_without_the_loop(pkg, gpu, tmp_path):
    """The benchmark's 20 views at its size, four frames per launch: this library against the -DSHRAY_LEAF_UNIFORM=0 build
    (make -C shader-ray_amd variant VARIANT=nouniform HIP_EXTRA="-DSHRAY_LEAF_UNIFORM=0"), where that has been built."""
    if not os.path.exists(NOUNIFORM):
        pytest.skip("the SHRAY_LEAF_UNIFORM=0 variant is not built")
    import torch
    import bench
    run = subprocess.run([sys.executable, "-c", CHILD, ROOT, str(tmp_path)], env=dict(os.environ, SHRAY_HIP_LIB=NOUNIFORM),
                         capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert run.returncode == 0 and "views written" in run.stdout, (run.stdout + run.stderr)[-3000:]
    world = pkg.World(pkg.scenes.bunny_trisrc())
    scene = pkg.Scene(world.flatten(), pkg.scenes.environment_hdr_sky(2048), device=0)
    try:
        scene.set_kernel(0)
        orbit = bench.orbit_params(pkg, world, bench.WIDTH, bench.HEIGHT)
        stream = torch.cuda.current_stream().cuda_stream
        for first in range(0, bench.ORBIT, 4):
            out = torch.zeros(4, bench.HEIGHT, bench.WIDTH, 4, dtype=torch.float32, device="cuda")
            scene.render_batch_into(orbit[first:first + 4], bench.WIDTH, bench.HEIGHT, 1, out.data_ptr(),
                                    bench.HEIGHT * bench.WIDTH * 16, stream)
            torch.cuda.synchronize()
            path = os.path.join(str(tmp_path), f"views_{first}.pt")
            theirs = torch.load(path)
            os.remove(path)
            assert torch.equal(out.cpu().view(torch.int32), theirs.view(torch.int32)), f"views {first} .. {first + 3} differ"
            for k in range(4):
                lone = scene.render(orbit[first + k], bench.WIDTH, bench.HEIGHT, 1)
                assert np.array_equal(bits(lone), bits(theirs[k].numpy())), f"view {first + k}, one frame per launch"
    finally:
        scene.close()
