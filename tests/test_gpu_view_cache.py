"""The scene's view cache (include/shader_ray_hip.h: shray_scene_set_view_cache) leaves every frame as it is.

Every case renders the same launches twice -- with the cache off, then on -- and compares the frames bit for bit, every pixel;
where the suite has an oracle for the fixture the cached frames are compared with it too, and the statistics call proves that
the cached launches really read an entry.  Sizes are 64x48, and 70x37 for patches with lanes outside the frame."""
import ctypes as C
import os

import numpy as np
import pytest

import helpers
from helpers import default_params, single_leaf_scene

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SIZES = [(64, 48), (70, 37)]
STATS = ("entries_built", "launches_cached")

# one triangle in front of the start-up camera (at z = 4, looking down -z; a 64x48 frame sees about 2.9 x 2.2 at z = 0)
TRIANGLE = [[[-0.8, -0.6, 0.0], [0.9, -0.5, 0.1], [0.1, 0.7, -0.1]]]
FILLING = [[[-60.0, -50.0, 0.0], [60.0, -50.0, 0.0], [0.0, 80.0, 0.0]]]
OUT_OF_VIEW = [[[100.0, 100.0, 0.0], [101.0, 100.0, 0.0], [100.0, 101.0, 0.0]]]


@pytest.fixture(scope="module")
def env(pkg):
    return pkg.scenes.environment_hdr_sky(128)


@pytest.fixture(scope="module")
def other_env(pkg):
    return pkg.scenes.environment_grid(64)


def frame(pkg, W, H, turn=0.0, **changes):
    """The start-up camera's frame block with the object turned by `turn` about y (what a drag changes), then `changes`."""
    p = default_params(pkg, W, H)
    c, s = float(np.cos(turn)), float(np.sin(turn))
    for name in ("object_matrix", "object_inverse", "object_normal_matrix", "object_normal_inverse"):
        m = getattr(p, name)
        sign = 1.0 if name in ("object_matrix", "object_normal_matrix") else -1.0
        m[0], m[2], m[8], m[10] = c, -sign * s, sign * s, c
    for name, value in changes.items():
        if name == "zoom":
            p.camera_matrix[14] = value
        else:
            setattr(p, name, value)
    return p


def launch(frames, W=64, H=48, spp=1, stream=0, tiles=None, one_by_one=False):
    return {"frames": frames, "W": W, "H": H, "spp": spp, "stream": stream, "tiles": tiles, "one_by_one": one_by_one}


def run(pkg, scene, steps, streams):
    """Enqueues the steps -- launches, or callables run between two launches -- without waiting in between; returns every
    launch's frames as float32 arrays [frames, pixels * 4]."""
    import torch
    from shader_ray_amd.tracer import tile_buffer_bytes
    outs = []
    for step in steps:
        if callable(step):
            step()
            continue
        nbytes = tile_buffer_bytes(step["W"], step["H"], step["tiles"])
        out = torch.full((len(step["frames"]), nbytes // 4), -7.0, dtype=torch.float32, device="cuda")
        st = streams[step["stream"] % len(streams)]
        st.wait_stream(torch.cuda.current_stream())      # (the fill above)
        if step["one_by_one"]:
            for k, p in enumerate(step["frames"]):
                scene.render_into(p, step["W"], step["H"], step["spp"], out[k].data_ptr(), st.cuda_stream, step["tiles"])
        else:
            scene.render_batch_into(step["frames"], step["W"], step["H"], step["spp"], out.data_ptr(), nbytes, st.cuda_stream, step["tiles"])
        outs.append(out)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs]


def off_then_on(pkg, scene, steps, lanes=1):
    """The steps with the cache off and on: asserts bit-identical frames, returns (the cached frames, the statistics' growth)."""
    import torch
    streams = [torch.cuda.current_stream()] + [torch.cuda.Stream() for _ in range(lanes - 1)]
    scene.set_view_cache(False)
    assert scene.view_cache_stats()["bytes_held"] >= 0
    before_off = scene.view_cache_stats()
    plain = run(pkg, scene, steps, streams)
    assert {k: scene.view_cache_stats()[k] for k in STATS} == {k: before_off[k] for k in STATS}, "the cache is off and still worked"
    scene.set_view_cache(True)
    before = scene.view_cache_stats()
    cached = run(pkg, scene, steps, streams)
    after = scene.view_cache_stats()
    assert len(plain) == len(cached)
    for j, (a, b) in enumerate(zip(plain, cached)):
        differing = int((a.view(np.uint32) != b.view(np.uint32)).sum())
        assert differing == 0, f"launch {j}: {differing} floats differ between the cached and the uncached frames"
        assert not (a == -7.0).all(), f"launch {j} rendered nothing"
    return cached, {k: after[k] - before[k] for k in STATS}


def as_image(flat, W, H):
    return flat.reshape(H, W, 4)


def assert_oracle(oracle_mod, desc, environment, params, W, H, got, what):
    want, _ = oracle_mod.render(desc, environment, params, W, H, 1)
    differing = int((as_image(got, W, H).view(np.uint32) != want.view(np.uint32)).sum())
    assert differing == 0, f"{what}: {differing} floats of the cached frame are not bit-identical to the oracle"


@pytest.fixture(scope="module")
def triangle(pkg, gpu, env):
    hand = single_leaf_scene(TRIANGLE)
    scene = pkg.Scene(hand.desc, env, device=0)
    yield hand, scene
    scene.close()


@pytest.fixture(scope="module")
def lobed(pkg, gpu, env):
    world = pkg.World(os.path.join(GOLDEN, "lobed_528.trisrc"))
    desc = world.flatten()
    scene = pkg.Scene(desc, env, device=0)
    yield world, desc, scene
    scene.close()


def build_sequence(frames_per_launch, turns, make):
    """launch 1 (no entry), launch 2 (builds), launches 3 to 5 (cached): one camera, three object rotations"""
    return [[make(turns[(j + k) % 3]) for k in range(frames_per_launch)] for j in range(5)]


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("frames_per_launch", [1, 4])
def test_build_sequence_one_triangle(pkg, oracle_mod, triangle, env, W, H, frames_per_launch):
    hand, scene = triangle
    batches = build_sequence(frames_per_launch, [0.0, 0.4, -0.7], lambda t: frame(pkg, W, H, t))
    steps = [launch(b, W, H, one_by_one=frames_per_launch == 1) for b in batches]
    cached, grew = off_then_on(pkg, scene, steps)
    # launch 2 builds and reads, 3 to 5 read; launches of ONE frame never read the cache (a lone frame is latency-bound and was
    # measured slower with it): they are what they were
    assert grew == ({"entries_built": 1, "launches_cached": 4} if frames_per_launch > 1 else {"entries_built": 0, "launches_cached": 0})
    for j, b in enumerate(batches):
        assert_oracle(oracle_mod, hand.desc, env, b[0], W, H, cached[j][0], f"launch {j + 1}")
    assert scene.view_cache_stats()["bytes_held"] >= (W * H * 28 if frames_per_launch > 1 else 0)


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("frames_per_launch", [1, 4])
def test_build_sequence_over_four_streams(pkg, lobed, W, H, frames_per_launch):
    """The same with the launches alternating over four streams: a launch on another stream than the prepass's reads the entry only
    once it is complete, and until then renders as ever -- how many do is a matter of timing, the frames are not."""
    import torch
    world, desc, scene = lobed
    view = world.default_view()
    batches = []
    for j in range(6):
        batch = []
        for k in range(frames_per_launch):
            pkg.host.trackball_motion(view.object_rotation, 0.05, 0.02)
            batch.append(world.frame_params(W, H, view))
        batches.append(batch)
    steps = [launch(b, W, H, stream=j, one_by_one=frames_per_launch == 1) for j, b in enumerate(batches[:5])]
    # the device is idle before the sixth launch: whichever stream it is on, it reads the entry
    steps += [torch.cuda.synchronize, launch(batches[5], W, H, stream=3, one_by_one=frames_per_launch == 1)]
    cached, grew = off_then_on(pkg, scene, steps, lanes=4)
    if frames_per_launch == 1:
        assert grew == {"entries_built": 0, "launches_cached": 0}       # one-frame launches never read the cache
    else:
        assert grew["entries_built"] == 1 and 2 <= grew["launches_cached"] <= 5


def test_golden_scene_cached_frames_match_the_oracle(pkg, oracle_mod, lobed, env):
    world, desc, scene = lobed
    for W, H in SIZES:
        for material in (0, 6):
            params = world.frame_params(W, H, material=material)
            cached, grew = off_then_on(pkg, scene, [launch([params] * 2, W, H) for _ in range(3)])
            assert grew == {"entries_built": 1, "launches_cached": 2}
            assert_oracle(oracle_mod, desc, env, params, W, H, cached[2][1], f"lobed {W}x{H} material {material}")


def tiny_comb(triangle, branches):
    """test_oracle_kat.comb_scene's binary tree -- every ray that enters visits all 2 * branches + 1 nodes -- with every box tight
    around one small triangle in the last leaf: only the rays of a pixel or two enter it."""
    import test_oracle_kat as kat
    n = 2 * branches + 1
    neg, pos, axis = [-1] * n, [-1] * n, [2] * n
    for i in range(branches):
        neg[2 * i] = 2 * i + 1
        pos[2 * i] = 2 * i + 2
    points = np.asarray(triangle, np.float32).reshape(-1, 3)
    lo = np.tile(points.min(0) - [1e-4, 1e-4, 0.5], (n, 1))
    hi = np.tile(points.max(0) + [1e-4, 1e-4, 0.5], (n, 1))
    objects = np.zeros((n, 2), np.float32)
    objects[n - 1] = (0, 1)
    return helpers.HandScene(points, [[0, 0, 1]] * 3, lo, hi, kat.thread_tree(neg, pos, axis, 0), objects, 0)


def hit_pixels(a, b):
    return int((a.reshape(-1, 4).view(np.uint32) != b.reshape(-1, 4).view(np.uint32)).any(axis=1).sum())


@pytest.mark.parametrize("W,H", SIZES)
def test_object_placement(pkg, oracle_mod, gpu, env, W, H):
    """Out of view: every wave copies its pixels.  Filling the frame: none does.  One pixel: exactly one hit lane in one wave.  A
    capped lane in an otherwise empty wave: the marker colour survives."""
    frames = {}
    zoom, ipw = 4.0, default_params(pkg, W, H).image_plane_width
    px, py = 20, 13                       # the pixel whose centre the tiny triangle covers: half a pixel is 0.022 at z = 0
    cx = zoom * ipw * ((px + 0.5) / W - 0.5)
    cy = zoom * ipw * ((py + 0.5) / H - 0.5) * (H / W)
    tiny = [[[cx - 0.012, cy - 0.008, 0.0], [cx + 0.012, cy - 0.008, 0.0], [cx, cy + 0.014, 0.0]]]
    for name, triangles, cap in (("out of view", OUT_OF_VIEW, 400), ("filling", FILLING, 400), ("one pixel", tiny, 400), ("capped", tiny, 5)):
        # capped: the tiny triangle behind eleven nodes, and five visits allowed: the rays that enter its box end as markers, none hits
        hand = tiny_comb(tiny, 5) if name == "capped" else single_leaf_scene(triangles)
        scene = pkg.Scene(hand.desc, env, device=0)
        params = frame(pkg, W, H, max_bvh_iterations=cap)
        if name == "capped":
            _, cpu = oracle_mod.render(hand.desc, env, params, W, H, 1)
            assert cpu["bad_hits"] >= 1 and cpu["shaded_hits"] == 0, cpu
        cached, grew = off_then_on(pkg, scene, [launch([params] * 2, W, H) for _ in range(3)] + [launch([params] * 3, W, H)])
        assert grew == {"entries_built": 1, "launches_cached": 3}, name
        assert_oracle(oracle_mod, hand.desc, env, params, W, H, cached[3][2], name)
        frames[name] = cached[3][2]
        scene.close()
    sky = frames["out of view"]
    assert hit_pixels(frames["filling"], sky) > W * H * 0.9
    assert hit_pixels(frames["one pixel"], sky) == 1
    marker = as_image(frames["capped"], W, H)[py, px]
    assert hit_pixels(frames["capped"], sky) >= 1 and marker[0] > 0.5 and marker[1] == 0.0 and marker[2] == 0.0, marker


def test_key_changes_between_launches(pkg, triangle):
    """Each change of the key alone: the frames behind it must come from the new camera's own entry, never from the old one's."""
    hand, scene = triangle
    W, H = 64, 48
    base = dict(zoom=4.0)
    for what, change in (("zoom", dict(zoom=5.5)), ("image_plane_width", dict(image_plane_width=0.5)), ("aspect", dict(aspect=0.6)),
                         ("tonemap", dict(tonemap=0))):
        a = [frame(pkg, W, H, t, **base) for t in (0.0, 0.3)]
        b = [frame(pkg, W, H, t, **{**base, **change}) for t in (0.0, 0.3)]
        steps = [launch(a), launch(a), launch(b), launch(b), launch(a), launch(b)]
        cached, grew = off_then_on(pkg, scene, steps)
        assert grew == {"entries_built": 2, "launches_cached": 4}, what
        assert hit_pixels(cached[1][0], cached[3][0]) > 0, f"{what} changes the frame"


def test_frame_size_change(pkg, triangle):
    hand, scene = triangle
    wide, tall = [frame(pkg, 64, 48, 0.2)] * 2, [frame(pkg, 48, 64, 0.2)] * 2
    steps = [launch(wide, 64, 48), launch(wide, 64, 48), launch(tall, 48, 64), launch(tall, 48, 64), launch(wide, 64, 48)]
    cached, grew = off_then_on(pkg, scene, steps)
    assert grew == {"entries_built": 2, "launches_cached": 3}


def test_set_environment_between_launches(pkg, oracle_mod, triangle, env, other_env):
    hand, scene = triangle
    W, H = 70, 37
    p = frame(pkg, W, H, 0.1)
    steps = [lambda: scene.set_environment(env), launch([p] * 2, W, H), launch([p] * 2, W, H), lambda: scene.set_environment(other_env),
             launch([p] * 2, W, H), launch([p] * 2, W, H), launch([p] * 2, W, H)]
    try:
        cached, grew = off_then_on(pkg, scene, steps)
        assert grew == {"entries_built": 2, "launches_cached": 3}
        assert_oracle(oracle_mod, hand.desc, env, p, W, H, cached[1][1], "first environment")
        for j in (2, 3, 4):
            assert_oracle(oracle_mod, hand.desc, other_env, p, W, H, cached[j][1], f"second environment, launch {j + 1}")
    finally:
        scene.set_environment(env)


def test_two_cameras_and_a_third(pkg, triangle):
    """A, A, B, B, A keeps two entries; C evicts the least recently used one while launches that read it are still queued (nothing
    waits between the launches, which alternate over four streams), and A comes back afterwards."""
    hand, scene = triangle
    W, H = 70, 37
    cam = {name: [frame(pkg, W, H, t, zoom=z) for t in (0.0, 0.5, -0.5, 0.9)] for name, z in (("A", 4.0), ("B", 4.7), ("C", 6.0))}
    order = "AABBA"
    cached, grew = off_then_on(pkg, scene, [launch(cam[c], W, H) for c in order])
    assert grew == {"entries_built": 2, "launches_cached": 3}
    # a camera that alternates between two positions is cached from its second round on; one that cycles through three is not
    cached, grew = off_then_on(pkg, scene, [launch(cam[c], W, H) for c in "ABABAB"])
    assert grew == {"entries_built": 2, "launches_cached": 4}
    cached, grew = off_then_on(pkg, scene, [launch(cam[c], W, H) for c in "ABCABCA"])
    assert grew == {"entries_built": 0, "launches_cached": 0}
    order = "AABBACCBBAAC"
    cached, grew = off_then_on(pkg, scene, [launch(cam[c], W, H, stream=j) for j, c in enumerate(order)], lanes=4)
    assert grew["entries_built"] == 5                       # A, B, C (evicts B), B (evicts A), A (evicts C)
    cached, grew = off_then_on(pkg, scene, [launch(cam[c], W, H) for c in order])
    assert grew == {"entries_built": 5, "launches_cached": 6}


def test_batch_with_different_cameras(pkg, triangle):
    hand, scene = triangle
    W, H = 64, 48
    a, b, c = (frame(pkg, W, H, 0.2 * k, zoom=z) for k, z in enumerate((4.0, 5.0, 6.5)))
    cached, grew = off_then_on(pkg, scene, [launch([a, b, a, b], W, H) for _ in range(3)])
    assert grew == {"entries_built": 2, "launches_cached": 2}
    # three cameras in every launch: two entries serve two of them, the third renders as ever
    cached, grew = off_then_on(pkg, scene, [launch([a, b, c, a], W, H) for _ in range(3)])
    assert grew == {"entries_built": 2, "launches_cached": 2}


def test_never_cached(pkg, triangle, monkeypatch):
    hand, scene = triangle
    N = pkg._native
    W, H = 64, 48
    p = frame(pkg, W, H, 0.3)
    for what, step in (("spp 4", launch([p] * 2, W, H, spp=4)), ("which 2", launch([frame(pkg, W, H, 0.3, which=2)] * 2, W, H)),
                       ("a tile launch", launch([p] * 2, W, H, tiles=N.TileSet(16, 16, 2, 1, 1)))):
        cached, grew = off_then_on(pkg, scene, [step] * 4)
        assert grew == {"entries_built": 0, "launches_cached": 0}, what
    # a frame over the byte cap (the variable is read where an entry would be built): 64 x 48 x 28 bytes is 84 KB
    monkeypatch.setenv("SHRAY_VIEW_CACHE_MAX_MB", "0")
    cached, grew = off_then_on(pkg, scene, [launch([p] * 2, W, H)] * 4)
    assert grew == {"entries_built": 0, "launches_cached": 0}, "over the cap"
    monkeypatch.setenv("SHRAY_VIEW_CACHE_MAX_MB", "1")
    big = frame(pkg, 256, 160, 0.3)                           # 1.1 MB
    cached, grew = off_then_on(pkg, scene, [launch([big] * 2, 256, 160)] * 3 + [launch([p] * 2, W, H)] * 3)
    assert grew == {"entries_built": 1, "launches_cached": 2}, "one frame over the cap, one under"


@pytest.mark.parametrize("W,H", SIZES)
def test_out_of_range_eye_ray(pkg, oracle_mod, triangle, env, W, H):
    """An image plane wider than exact_div.h admits (2^10 against 2^9), and one narrower (2^-31 against 2^-30): the eye ray is
    normalised by true divisions in the frame kernels, and in the prepass too."""
    hand, scene = triangle
    for ipw in (1024.0, 2.0 ** -31):
        p = frame(pkg, W, H, 0.2, image_plane_width=ipw)
        cached, grew = off_then_on(pkg, scene, [launch([p] * 2, W, H) for _ in range(3)])
        assert grew == {"entries_built": 1, "launches_cached": 2}
        assert_oracle(oracle_mod, hand.desc, env, p, W, H, cached[2][0], f"image_plane_width {ipw}")


@pytest.mark.parametrize("bounces", [0, 1])
def test_bounce_counts(pkg, oracle_mod, lobed, env, bounces):
    world, desc, scene = lobed
    for W, H in SIZES:
        p = world.frame_params(W, H)
        p.bounce_count = bounces
        cached, grew = off_then_on(pkg, scene, [launch([p] * 4, W, H) for _ in range(3)])
        assert grew == {"entries_built": 1, "launches_cached": 2}
        assert_oracle(oracle_mod, desc, env, p, W, H, cached[2][3], f"bounce_count {bounces} {W}x{H}")
