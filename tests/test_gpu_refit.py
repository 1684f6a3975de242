"""The refit on the GPU (include/shader_ray_refit.h) against the scene the full pipeline makes for the same tree and the new
vertices: the tree (World.export_tree, or shray_device_tree_download for a DeviceWorld) with the restated boxes
(tests/refit_ref.py) and the moved vertex data, flattened by shray_flatten_device and created by shray_scene_create.  After a
refit every array of the scene, its frames and work counters, and its ray-query hits and counters equal that scene's; the
SAH cost and the exact-division flag equal the restatement's.  Also: round trips through both input forms and every stride,
the device path on a non-null stream, every argument error (the scene is left unchanged), and a scene without a packed tree."""
import ctypes as C
import os

import numpy as np
import pytest

import helpers
import refit_ref as R
from test_gpu_ray_query import random_rays
from test_oracle_kat import chain_scene

pytestmark = pytest.mark.gpu

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SCENES = ["lobed_528", "quads_nonormals", "bunny"]
DEFORMATIONS = ["identity", "twist", "inside_out", "collapse", "huge"]
N_RAYS = 1 << 14
INVALID, BAD_TREE = -1, -6


def scene_path(name):
    return {"lobed_528": os.path.join(GOLDEN, "lobed_528.trisrc"), "quads_nonormals": os.path.join(GOLDEN, "quads_nonormals.obj"),
            "bunny": helpers.bunny_trisrc()}[name]


class Subject:
    """A scene to refit, its tree and its vertex data [V, 9] (load numbering; the tree's triangle_vertices index it)."""

    def __init__(self, pkg, name, how):
        self.name, self.how = name, how
        self.env = pkg.scenes.environment_constant()
        if how == "host":
            self.world = pkg.World(scene_path(name))
            desc = self.world.export_tree()
            self.scene = pkg.Scene(self.world.flatten(), self.env)
            self.frame_params = self.world.frame_params
        else:
            self.world = pkg.tracer.DeviceWorld(scene_path(name), self.env)
            desc, order = pkg._native.TreeDesc(), C.POINTER(C.c_int32)()
            pkg._native.check(self.world._hip.shray_device_tree_download(self.world._tree, C.byref(desc), C.byref(order)))
            self.scene = self.world.scene
            self.frame_params = self.world.frame_params
        self.tree = R.TreeArrays.of(desc)
        self.vertex_data = np.ctypeslib.as_array(desc.vertex_data, shape=(desc.vertex_count * 9,)).reshape(-1, 9).copy()

    def refit(self, vd, **kw):
        if self.how == "device":
            return self.world.refit(vd)          # DeviceWorld.refit: [V, 9], normals from column 6, the tree's indices
        return self.scene.refit(vd, self.tree.triangle_vertices, normal_offset=6, **kw)

    def close(self):
        self.world.close()


def deform(vd, how):
    """seeded float32 deformations of the positions (and, to follow them, the normals) of vertex data [V, 9]"""
    out = vd.copy()
    p = vd[:, :3].astype(np.float64)
    lo, hi = p.min(0), p.max(0)
    c, ext = (lo + hi) / 2, float(np.max(hi - lo))
    q = p - c
    rng = np.random.default_rng(DEFORMATIONS.index(how) + 5)
    if how == "identity":
        return out
    if how == "twist":
        ang = 0.6 * q[:, 1] / ext
        r = 1.0 + 0.15 * np.sin(3.0 * q[:, 1] / ext * np.pi) + 0.01 * rng.standard_normal(len(q))
        x = (q[:, 0] * np.cos(ang) - q[:, 2] * np.sin(ang)) * r
        z = (q[:, 0] * np.sin(ang) + q[:, 2] * np.cos(ang)) * r
        q = np.stack([x, q[:, 1], z], 1)
    elif how == "inside_out":
        d = np.linalg.norm(q, axis=1, keepdims=True)
        q = np.where(d > 0, q / np.maximum(d, 1e-30) * (d.max() - d), q)
    elif how == "collapse":
        q = np.zeros_like(q) + rng.standard_normal(3) * 0.1 * ext
    elif how == "huge":
        # some coordinate reaches 2^60 (exact_div.h's operand range ends there): exact_div_ok must turn 0
        q = (p / np.max(np.abs(p))) * 2.0 ** 61
        out[:, :3] = q.astype(F)
        out[:, 6:9] = -vd[:, 6:9]
        return out
    out[:, :3] = (q + c).astype(F)
    out[:, 6:9] = np.roll(vd[:, 6:9], 1, axis=1)     # new normals, so that "normals given" is visible
    return out


def expected_scene(pkg, subject, vd):
    """shray_flatten_device + shray_scene_create of the subject's tree with the restated boxes over `vd`; and the boxes"""
    boxes = R.node_boxes(subject.tree, vd[subject.tree.triangle_vertices][:, :, :3])
    flat = pkg.tracer.DeviceFlat(R.tree_desc(subject.tree, boxes, vd))
    scene = pkg.Scene(flat.download(), subject.env)
    flat.close()
    return scene, boxes


def assert_same_scene(got, want, what):
    a, b = got.derived_arrays(), want.derived_arrays()
    assert a["stack_levels"] == b["stack_levels"], what
    for key in ("packed_nodes", "packed_tris", "normals16", "pair_nodes"):
        assert a[key].shape == b[key].shape and a[key].size > 0, (what, key)
        bad = int((a[key] != b[key]).sum())
        assert bad == 0, f"{what}: {bad} words of {key} differ"
    ga, gb = got.geometry(), want.geometry()
    for key in ga:
        assert ga[key].size and np.array_equal(ga[key].view(np.uint32), gb[key].view(np.uint32)), (what, key)


def snapshot(scene):
    return scene.derived_arrays(), scene.geometry()


def assert_unchanged(scene, before, what):
    d, g = snapshot(scene)
    for key in ("packed_nodes", "packed_tris", "normals16", "pair_nodes"):
        assert np.array_equal(d[key], before[0][key]), (what, key)
    for key in g:
        assert np.array_equal(g[key].view(np.uint32), before[1][key].view(np.uint32)), (what, key)


class Positions:
    def __init__(self, corners):
        self.positions = corners


@pytest.fixture(scope="module")
def subject(pkg, gpu):
    """subject(name, how): one Subject per scene and creation path for this module, refit to its loaded vertices whenever it
    is handed out (so that no test depends on where another left it), closed at the module's end"""
    made = {}

    def get(name, how):
        if (name, how) not in made:
            made[(name, how)] = Subject(pkg, name, how)
        s = made[(name, how)]
        s.refit(s.vertex_data)
        return s

    yield get
    for s in made.values():
        s.close()


@pytest.mark.parametrize("how", ["host", "device"])
@pytest.mark.parametrize("name", SCENES)
def test_refit_equals_the_rebuilt_scene(pkg, gpu, subject, name, how):
    s = subject(name, how)
    for deformation in DEFORMATIONS + ["identity"]:       # (and back)
        vd = deform(s.vertex_data, deformation)
        what = f"{name}/{how}/{deformation}"
        stats = s.refit(vd)
        want, boxes = expected_scene(pkg, s, vd)
        assert_same_scene(s.scene, want, what)
        assert stats["exact_div_ok"] == int(R.exact_div_ok(boxes)), what
        assert stats["exact_div_ok"] == (0 if deformation == "huge" else 1), what
        assert stats["sah_cost"] == pytest.approx(R.sah_cost(s.tree, boxes), rel=1e-12, abs=0.0), what
        # frames and work counters, kernels 0 and 1, gold and plaster (framed on the mesh as loaded)
        for material in (0, 6):
            params = s.frame_params(64, 48, material=material)
            for kernel in (0, 1):
                s.scene.set_kernel(kernel)
                want.set_kernel(kernel)
                img, cnt = s.scene.render_counters(params, 64, 48, 1)
                wimg, wcnt = want.render_counters(params, 64, 48, 1)
                assert np.array_equal(img.view(np.uint32), wimg.view(np.uint32)) and cnt == wcnt, (what, material, kernel)
        # ray queries: the seeded ray set about the moved mesh, closest and any hit
        corners = vd[s.tree.triangle_vertices][:, :, :3]
        o, d, tmax = random_rays(Positions(corners), N_RAYS, seed=DEFORMATIONS.index(deformation) + 40)
        rays = pkg.tracer.make_rays(o, d, tmax)
        for kernel in (0, 1):
            s.scene.set_kernel(kernel)
            want.set_kernel(kernel)
            for any_hit in (False, True):
                got, gc = s.scene.trace_rays(rays, any_hit=any_hit, counters=True)
                exp, ec = want.trace_rays(rays, any_hit=any_hit, counters=True)
                assert np.array_equal(got.view(np.uint32), exp.view(np.uint32)) and gc == ec, (what, kernel, any_hit)
        s.scene.set_kernel(0)
        want.close()


def test_round_trips_through_every_input_form(pkg, gpu, subject):
    s = subject("lobed_528", "host")
    original = snapshot(s.scene)
    moved = deform(s.vertex_data, "twist")
    tv = s.tree.triangle_vertices
    want, _ = expected_scene(pkg, s, moved)
    kept = moved.copy()
    kept[:, 6:9] = s.vertex_data[:, 6:9]
    want_kept, _ = expected_scene(pkg, s, kept)
    corners9 = moved[tv].reshape(-1, 9)
    stride12 = np.concatenate([moved[:, :3], np.full((len(moved), 3), 7, F), moved[:, 6:9], moved[:, 3:6]], 1)
    forms = [  # (what, call, the scene it must equal)
        ("indexed, stride 9, normals given", lambda: s.scene.refit(moved, tv, normal_offset=6), want),
        ("indexed, stride 3, normals kept", lambda: s.scene.refit(np.ascontiguousarray(moved[:, :3]), tv), want_kept),
        ("indexed, stride 9, normals kept", lambda: s.scene.refit(moved, tv), want_kept),
        ("corners, stride 9, normals given", lambda: s.scene.refit(corners9, normal_offset=6), want),
        ("corners, stride 3, normals kept", lambda: s.scene.refit(np.ascontiguousarray(corners9[:, :3])), want_kept),
        ("indexed, stride 12, normals given", lambda: s.scene.refit(stride12, tv, normal_offset=6), want),
    ]
    for what, call, target in forms:
        call()
        assert_same_scene(s.scene, target, what)
        # ... and back: A -> B -> A gives the original arrays bit for bit
        s.scene.refit(s.vertex_data, tv, normal_offset=6)
        assert_unchanged(s.scene, original, what + ", back")
    for w in (want, want_kept):
        w.close()


def test_device_path_on_a_stream_equals_the_host_path(pkg, gpu, subject):
    import torch
    s = subject("bunny", "host")
    other = pkg.Scene(s.world.flatten(), s.env)
    moved = deform(s.vertex_data, "twist")
    host_stats = s.scene.refit(moved, s.tree.triangle_vertices, normal_offset=6)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        vd = torch.from_numpy(moved).cuda()
        tv = torch.from_numpy(s.tree.triangle_vertices.copy()).cuda()
        dev_stats = other.refit(vd, tv, normal_offset=6, stream_ptr=stream.cuda_stream)
    assert dev_stats == host_stats
    assert_same_scene(other, s.scene, "device path on a stream")
    s.scene.refit(s.vertex_data, s.tree.triangle_vertices, normal_offset=6)
    other.close()


def test_argument_errors_leave_the_scene_unchanged(pkg, gpu, subject):
    import torch
    N = pkg._native
    lib = N.load_refit()
    s = subject("lobed_528", "host")
    before = snapshot(s.scene)
    vd, tv = s.vertex_data, s.tree.triangle_vertices

    def raw(vertex_data, triangle_vertices, count=None, stride=9, normal_offset=6, size=None, device=False, stream=None):
        inp = N.RefitInput()
        inp.struct_size = C.sizeof(N.RefitInput) if size is None else size
        inp.vertex_count = len(vertex_data) if count is None else count
        inp.vertex_stride_floats, inp.normal_offset_floats = stride, normal_offset
        if device:
            inp.vertex_data = vertex_data.data_ptr()
            inp.triangle_vertices = triangle_vertices.data_ptr() if triangle_vertices is not None else None
            return lib.shray_scene_refit_device(s.scene._handle, C.byref(inp), None, C.c_void_p(stream))
        inp.vertex_data = vertex_data.ctypes.data if vertex_data is not None else None
        inp.triangle_vertices = triangle_vertices.ctypes.data if triangle_vertices is not None else None
        return lib.shray_scene_refit(s.scene._handle, C.byref(inp), None)

    nan, inf = vd.copy(), vd.copy()
    nan[17, 1] = np.nan
    inf[3, 7] = np.inf                          # a normal
    bad_low, bad_high = tv.copy(), tv.copy()
    bad_low[5, 2] = -1
    bad_high[9, 0] = len(vd)
    corners = np.ascontiguousarray(vd[tv].reshape(-1, 9))
    cases = {
        "NULL input": lambda: lib.shray_scene_refit(s.scene._handle, None, None),
        "NULL vertex_data": lambda: raw(None, tv, count=len(vd)),
        "wrong struct_size": lambda: raw(vd, tv, size=C.sizeof(N.RefitInput) - 8),
        "stride 2": lambda: raw(vd, tv, stride=2, normal_offset=-1),
        "normal beyond the stride": lambda: raw(vd, tv, normal_offset=7),
        "negative normal offset": lambda: raw(vd, tv, normal_offset=-2),
        "index below 0": lambda: raw(vd, bad_low),
        "index at vertex_count": lambda: raw(vd, bad_high),
        "corner count": lambda: raw(corners[:-3], None),
        "NaN position": lambda: raw(nan, tv),
        "infinite normal": lambda: raw(inf, tv),
        "negative vertex_count": lambda: raw(vd, tv, count=-1),
    }
    d_vd = torch.from_numpy(vd).cuda()
    d_bad = torch.from_numpy(bad_high).cuda()
    d_nan = torch.from_numpy(nan).cuda()
    torch.cuda.synchronize()
    cases["device path: index out of range"] = lambda: raw(d_vd, d_bad, device=True)
    cases["device path: NaN position"] = lambda: raw(d_nan, torch.from_numpy(tv.copy()).cuda(), device=True)
    for what, call in cases.items():
        assert call() == INVALID, what
        assert_unchanged(s.scene, before, what)
    # the stats pointer may be NULL; a valid call after all of them still works
    assert raw(vd, tv) == 0
    assert_unchanged(s.scene, before, "identity after the errors")


def test_host_memory_never_reaches_the_device_path(pkg, gpu, subject):
    """CPU tensors take the host path (the same result as numpy); the device form refuses host memory before any launch, and
    Scene.refit refuses a triangle_vertices array of the wrong length; a refused call leaves the scene unchanged"""
    import torch
    N = pkg._native
    lib = N.load_refit()
    s = subject("lobed_528", "host")
    before = snapshot(s.scene)
    vd, tv = s.vertex_data, s.tree.triangle_vertices
    moved = deform(vd, "twist")
    want, _ = expected_scene(pkg, s, moved)
    stats = s.scene.refit(torch.from_numpy(moved), torch.from_numpy(tv.copy()), normal_offset=6)
    assert_same_scene(s.scene, want, "CPU tensors")
    assert stats == s.scene.refit(moved, tv, normal_offset=6)
    want.close()
    s.scene.refit(vd, tv, normal_offset=6)
    assert_unchanged(s.scene, before, "back from CPU tensors")
    # a bad index in a CPU tensor: refused by the host path's validation
    bad = tv.copy()
    bad[2, 1] = len(vd)
    with pytest.raises(N.ShrayError) as err:
        s.scene.refit(torch.from_numpy(vd), torch.from_numpy(bad), normal_offset=6)
    assert err.value.code == INVALID
    assert_unchanged(s.scene, before, "CPU tensor, bad index")
    # host pointers handed to the device form directly
    inp = N.RefitInput()
    inp.struct_size = C.sizeof(N.RefitInput)
    inp.vertex_count, inp.vertex_stride_floats, inp.normal_offset_floats = len(vd), 9, 6
    inp.vertex_data, inp.triangle_vertices = vd.ctypes.data, tv.ctypes.data
    assert lib.shray_scene_refit_device(s.scene._handle, C.byref(inp), None, None) == INVALID
    d_vd = torch.from_numpy(vd).cuda()
    inp.vertex_data = d_vd.data_ptr()                     # device vertices, host indices
    assert lib.shray_scene_refit_device(s.scene._handle, C.byref(inp), None, None) == INVALID
    assert_unchanged(s.scene, before, "host memory on the device path")
    # the wrong number of indices, host and device
    for short in (tv.reshape(-1)[:-3], torch.from_numpy(tv.reshape(-1)[:-3].copy()).cuda()):
        with pytest.raises(ValueError):
            s.scene.refit(moved if isinstance(short, np.ndarray) else torch.from_numpy(moved).cuda(), short, normal_offset=6)
    assert_unchanged(s.scene, before, "short triangle_vertices")
    # a valid device-path call after the refusals still works
    s.scene.refit(d_vd, torch.from_numpy(tv.copy()).cuda(), normal_offset=6)
    assert_unchanged(s.scene, before, "device path after the refusals")


def test_a_scene_without_a_packed_tree_is_refused(pkg, gpu):
    hand = chain_scene(5)                        # five leaves threaded one after another: not a canonical binary tree
    scene = pkg.Scene(hand.desc)
    before = snapshot(scene)
    assert before[0]["packed_nodes"].size == 0
    corners = np.ascontiguousarray(before[1]["vertex_positions"].reshape(-1, 3) + F(1))
    with pytest.raises(pkg._native.ShrayError) as err:
        scene.refit(corners)
    assert err.value.code == BAD_TREE
    assert_unchanged(scene, before, "no packed tree")
    scene.close()
