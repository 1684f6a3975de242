"""include/shader_ray_instance_sdf.h against libshray_instance_sdf.so and the ctypes mirror: exactly the declared functions are
exported and bound, the header compiles as C with the struct sizes the mirror has, the signed-distance library exports the
accessor the new library reads a member scene's sign data through (and keeps it out of its header), the new library links the
libraries it calls, the Python wrappers exist, and every argument refusal the header lists returns SHRAY_ERR_INVALID_ARGUMENT
before any set or device is touched."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "shader_ray_instance_sdf.h")
FUNCTIONS = {"shray_signed_distance_instances_device", "shray_signed_distance_instances", "shray_signed_distance_instances_counters"}


def declared():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return set(re.findall(r"^\s*(?:int|void)\s+\**(shray_\w+)\s*\(", text, flags=re.M))


def test_header_symbols_are_exactly_the_exported_and_bound_ones(pkg):
    names = declared()
    assert names == FUNCTIONS
    assert names == {n for n, _, _ in pkg._native.INSTANCE_SDF_SYMBOLS}
    lib = pkg._native.load_instance_sdf()
    out = subprocess.run(["nm", "-D", "--defined-only", pkg._native.INSTANCE_SDF_LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\b[TW] (shrayi?_\w+)", out))
    assert exported == names, exported ^ names
    for n in names:
        assert getattr(lib, n).argtypes is not None


def test_the_header_compiles_as_c_and_the_struct_sizes_match(pkg, tmp_path):
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include "shader_ray_instance_sdf.h"\nint main(void) {\n'
                   '    int (*f)(shray_instance_set *, const shray_point *, int64_t, float *, shray_closest *, int32_t *, void *) = 0;\n'
                   '    (void)f;\n'
                   '    printf("%zu %zu %zu %d %d\\n", sizeof(shray_point), sizeof(shray_closest), sizeof(shray_counters),\n'
                   '           (int)SHRAY_POINT_MAX_HEIGHT, (int)SHRAY_SIGN_DATA_FLOATS);\n    return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    N = pkg._native
    want = [C.sizeof(N.Point), C.sizeof(N.Closest), C.sizeof(N.Counters), N.POINT_MAX_HEIGHT, N.SIGN_DATA_FLOATS]
    assert list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split())) == want
    assert want == [16, 32, 64, 128, 21]


def test_the_sdf_library_exports_the_sign_data_accessor(pkg):
    out = subprocess.run(["nm", "-D", "--defined-only", pkg._native.SDF_LIB], capture_output=True, text=True, check=True).stdout
    assert "shrayi_scene_sign_data" in set(re.findall(r"\bT (shray\w+)", out))
    for header in os.listdir(os.path.join(ROOT, "include")):
        assert "shrayi_scene_sign_data" not in open(os.path.join(ROOT, "include", header)).read(), header
    assert "shrayi_scene_sign_data" not in {n for n, _, _ in pkg._native.SDF_SYMBOLS}
    needed = subprocess.run(["readelf", "-d", pkg._native.INSTANCE_SDF_LIB], capture_output=True, text=True, check=True).stdout
    for lib in ("libshray_instance_point.so", "libshray_sdf.so", "libshray_instance.so", "libshray_hip.so"):
        assert lib in needed, lib
    # a NULL scene or a NULL result pointer is refused at the call
    pkg._native.load_sdf()
    lib = C.CDLL(pkg._native.SDF_LIB)
    lib.shrayi_scene_sign_data.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
    got = C.c_void_p(7)
    assert lib.shrayi_scene_sign_data(None, None, C.byref(got)) == -1
    assert lib.shrayi_scene_sign_data(C.c_void_p(1), None, None) == -1


def test_the_python_wrappers_are_bound(pkg):
    S = pkg.tracer.InstanceSet
    assert list(inspect.signature(S.signed_distance).parameters) == ["self", "points", "max_dist2", "closest", "counters"]
    assert list(inspect.signature(S.signed_distance_into).parameters) == ["self", "points_ptr", "count", "out_ptr", "closest_ptr",
                                                                         "instances_ptr", "stream_ptr"]
    assert list(inspect.signature(S.closed).parameters) == ["self"]
    assert callable(pkg._native.load_instance_sdf)


def test_argument_errors(pkg):
    """Each call below fails with SHRAY_ERR_INVALID_ARGUMENT before it reads the (fake) set; count 0 with valid arguments is a
    no-op that needs no set data or device."""
    N = pkg._native
    lib = N.load_instance_sdf()
    host, dev, cnt = lib.shray_signed_distance_instances, lib.shray_signed_distance_instances_device, lib.shray_signed_distance_instances_counters
    pts = (N.Point * 2)()
    val = (C.c_float * 2)()
    out = (N.Closest * 2)()
    inst = (C.c_int32 * 2)()
    c = N.Counters()
    buf = np.zeros(320, np.uint8)
    base = (buf.ctypes.data + 15) & ~15
    b, b64, b128, b192 = C.c_void_p(base), C.c_void_p(base + 64), C.c_void_p(base + 128), C.c_void_p(base + 192)
    fake = C.c_void_p(1)   # never read
    cases = {
        "NULL set": lambda: host(None, pts, 2, val, out, inst),
        "NULL points": lambda: host(fake, None, 2, val, out, inst),
        "NULL signed": lambda: host(fake, pts, 2, None, out, inst),
        "negative count": lambda: host(fake, pts, -1, val, out, inst),
        "counters, NULL counters": lambda: cnt(fake, pts, 2, val, out, inst, None),
        "counters, NULL set": lambda: cnt(None, pts, 2, val, out, inst, C.byref(c)),
        "counters, NULL points": lambda: cnt(fake, None, 2, val, out, inst, C.byref(c)),
        "counters, negative count": lambda: cnt(fake, pts, -3, val, out, inst, C.byref(c)),
        "device, NULL set": lambda: dev(None, b, 1, b192, b64, b128, None),
        "device, NULL points": lambda: dev(fake, None, 1, b192, b64, b128, None),
        "device, NULL signed": lambda: dev(fake, b, 1, None, b64, b128, None),
        "device, negative count": lambda: dev(fake, b, -1, b192, b64, b128, None),
        "device, misaligned points": lambda: dev(fake, C.c_void_p(base + 4), 1, b192, b64, b128, None),
        "device, misaligned records": lambda: dev(fake, b, 1, b192, C.c_void_p(base + 72), b128, None),
        "device, misaligned signed": lambda: dev(fake, b, 1, C.c_void_p(base + 194), b64, b128, None),
        "device, misaligned instances": lambda: dev(fake, b, 1, b192, b64, C.c_void_p(base + 130), None),
        "device, misaligned instances, count 0": lambda: dev(fake, b, 0, b192, b64, C.c_void_p(base + 129), None),
    }
    for what, call in cases.items():
        assert call() == -1, what
        assert N.load_hip().shray_last_error(), what
    assert host(fake, pts, 0, val, out, inst) == 0
    assert host(fake, pts, 0, val, None, None) == 0
    assert dev(fake, b, 0, b192, None, None, None) == 0
    assert dev(fake, b, 0, C.c_void_p(base + 196), b64, C.c_void_p(base + 132), None) == 0      # 4-byte alignment is enough for both
    c.samples = 99
    c.node_visits = 5
    assert cnt(fake, pts, 0, None, None, None, C.byref(c)) == 0
    assert c.as_dict() == dict.fromkeys(c.as_dict(), 0)
