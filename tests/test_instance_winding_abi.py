"""include/shader_ray_instance_winding.h against libshray_instance_winding.so and the ctypes mirror: exactly the declared functions
are exported and bound, the header compiles as C with the struct sizes the mirror has, the winding library exports the accessor
the new library reads a member scene's node records through (and keeps it out of every header and ctypes list), the new
library links the libraries it calls, the Python wrappers exist with their signatures, and every argument refusal the header
lists returns SHRAY_ERR_INVALID_ARGUMENT before any set or device is touched."""
import ctypes as C
import inspect
import math
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "shader_ray_instance_winding.h")
FUNCTIONS = {"shray_winding_number_instances_device", "shray_winding_number_instances", "shray_winding_signed_distance_instances_device",
             "shray_winding_signed_distance_instances", "shray_instance_set_orientations"}
ACCESSOR = "shrayi_scene_winding_records"


def declared():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return set(re.findall(r"^\s*(?:int|void)\s+\**(shray_\w+)\s*\(", text, flags=re.M))


def test_header_symbols_are_exactly_the_exported_and_bound_ones(pkg):
    names = declared()
    assert names == FUNCTIONS
    assert names == {n for n, _, _ in pkg._native.INSTANCE_WINDING_SYMBOLS}
    lib = pkg._native.load_instance_winding()
    out = subprocess.run(["nm", "-D", "--defined-only", pkg._native.INSTANCE_WINDING_LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\b[TW] (shrayi?_\w+)", out))
    assert exported == names, exported ^ names
    for n in names:
        assert getattr(lib, n).argtypes is not None


def test_the_header_compiles_as_c_and_the_struct_sizes_match(pkg, tmp_path):
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include "shader_ray_instance_winding.h"\nint main(void) {\n'
                   '    int (*f)(shray_instance_set *, const shray_point *, int64_t, float, float *, int32_t *, void *) = 0;\n'
                   '    int (*g)(shray_instance_set *, const shray_point *, int64_t, float, float *, shray_closest *, int32_t *, void *) = 0;\n'
                   '    int (*h)(shray_instance_set *, float *) = 0;\n'
                   '    printf("%zu %zu %d %d %d\\n", sizeof(shray_point), sizeof(shray_closest), (int)SHRAY_POINT_MAX_HEIGHT,\n'
                   '           (int)SHRAY_WINDING_DATA_FLOATS, (f == 0) + (g == 0) + (h == 0));\n    return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    N = pkg._native
    want = [C.sizeof(N.Point), C.sizeof(N.Closest), N.POINT_MAX_HEIGHT, N.WINDING_DATA_FLOATS, 3]
    assert list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split())) == want
    assert want == [16, 32, 128, 20, 3]


def test_the_winding_library_exports_the_record_accessor(pkg):
    out = subprocess.run(["nm", "-D", "--defined-only", pkg._native.WINDING_LIB], capture_output=True, text=True, check=True).stdout
    assert ACCESSOR in set(re.findall(r"\bT (shray\w+)", out))
    for header in os.listdir(os.path.join(ROOT, "include")):
        assert ACCESSOR not in open(os.path.join(ROOT, "include", header)).read(), header
    for name in dir(pkg._native):
        if name.endswith("_SYMBOLS"):
            assert ACCESSOR not in {n for n, _, _ in getattr(pkg._native, name)}, name
    needed = subprocess.run(["readelf", "-d", pkg._native.INSTANCE_WINDING_LIB], capture_output=True, text=True, check=True).stdout
    linked = set(re.findall(r"\[(libshray_\w+\.so)\]", needed))
    assert linked == {"libshray_instance_point.so", "libshray_winding.so", "libshray_instance.so", "libshray_hip.so"}, linked
    # a NULL scene or a NULL result pointer is refused at the call
    pkg._native.load_winding()
    lib = C.CDLL(pkg._native.WINDING_LIB)
    fn = getattr(lib, ACCESSOR)
    fn.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
    got = C.c_void_p(7)
    assert fn(None, None, C.byref(got)) == -1
    assert fn(C.c_void_p(1), None, None) == -1


def test_the_python_wrappers_are_bound(pkg):
    S = pkg.tracer.InstanceSet
    assert list(inspect.signature(S.winding_number).parameters) == ["self", "points", "beta", "containing"]
    assert inspect.signature(S.winding_number).parameters["beta"].default == 2.0
    assert inspect.signature(S.winding_number).parameters["containing"].default is False
    assert list(inspect.signature(S.winding_number_into).parameters) == ["self", "points_ptr", "count", "out_ptr", "containing_ptr", "beta",
                                                                         "stream_ptr"]
    assert list(inspect.signature(S.winding_signed_distance).parameters) == ["self", "points", "max_dist2", "beta", "closest"]
    assert inspect.signature(S.winding_signed_distance).parameters["beta"].default == 2.0
    assert list(inspect.signature(S.winding_signed_distance_into).parameters) == ["self", "points_ptr", "count", "out_ptr", "closest_ptr",
                                                                                  "instances_ptr", "beta", "stream_ptr"]
    assert list(inspect.signature(S.orientations).parameters) == ["self"]
    assert callable(pkg._native.load_instance_winding)


def test_argument_errors(pkg):
    """Each call below fails with SHRAY_ERR_INVALID_ARGUMENT before it reads the (fake) set; count 0 with valid arguments is a
    no-op that needs no set data or device."""
    N = pkg._native
    lib = N.load_instance_winding()
    num, num_dev = lib.shray_winding_number_instances, lib.shray_winding_number_instances_device
    sgn, sgn_dev = lib.shray_winding_signed_distance_instances, lib.shray_winding_signed_distance_instances_device
    pts = (N.Point * 2)()
    val = (C.c_float * 2)()
    out = (N.Closest * 2)()
    inst = (C.c_int32 * 2)()
    buf = np.zeros(320, np.uint8)
    base = (buf.ctypes.data + 15) & ~15
    b, b64, b128, b192 = C.c_void_p(base), C.c_void_p(base + 64), C.c_void_p(base + 128), C.c_void_p(base + 192)
    fake = C.c_void_p(1)   # never read
    nan, inf = math.nan, math.inf
    cases = {
        "number, NULL set": lambda: num(None, pts, 2, 2.0, val, inst),
        "number, NULL points": lambda: num(fake, None, 2, 2.0, val, inst),
        "number, NULL values": lambda: num(fake, pts, 2, 2.0, None, inst),
        "number, negative count": lambda: num(fake, pts, -1, 2.0, val, inst),
        "number, NaN beta": lambda: num(fake, pts, 2, nan, val, inst),
        "number, negative beta": lambda: num(fake, pts, 2, -1.0, val, inst),
        "number, NaN beta, count 0": lambda: num(fake, pts, 0, nan, val, inst),
        "signed, NULL set": lambda: sgn(None, pts, 2, 2.0, val, out, inst),
        "signed, NULL points": lambda: sgn(fake, None, 2, 2.0, val, out, inst),
        "signed, NULL values": lambda: sgn(fake, pts, 2, 2.0, None, out, inst),
        "signed, negative count": lambda: sgn(fake, pts, -1, 2.0, val, out, inst),
        "signed, NaN beta": lambda: sgn(fake, pts, 2, nan, val, out, inst),
        "signed, negative beta": lambda: sgn(fake, pts, 2, -inf, val, out, inst),
        "number device, NULL set": lambda: num_dev(None, b, 1, 2.0, b192, b128, None),
        "number device, NULL points": lambda: num_dev(fake, None, 1, 2.0, b192, b128, None),
        "number device, NULL values": lambda: num_dev(fake, b, 1, 2.0, None, b128, None),
        "number device, negative count": lambda: num_dev(fake, b, -1, 2.0, b192, b128, None),
        "number device, NaN beta": lambda: num_dev(fake, b, 1, nan, b192, b128, None),
        "number device, negative beta": lambda: num_dev(fake, b, 1, -0.5, b192, b128, None),
        "number device, misaligned points": lambda: num_dev(fake, C.c_void_p(base + 4), 1, 2.0, b192, b128, None),
        "number device, misaligned values": lambda: num_dev(fake, b, 1, 2.0, C.c_void_p(base + 194), b128, None),
        "number device, misaligned containing": lambda: num_dev(fake, b, 1, 2.0, b192, C.c_void_p(base + 130), None),
        "number device, misaligned containing, count 0": lambda: num_dev(fake, b, 0, 2.0, b192, C.c_void_p(base + 129), None),
        "signed device, NULL set": lambda: sgn_dev(None, b, 1, 2.0, b192, b64, b128, None),
        "signed device, NULL points": lambda: sgn_dev(fake, None, 1, 2.0, b192, b64, b128, None),
        "signed device, NULL values": lambda: sgn_dev(fake, b, 1, 2.0, None, b64, b128, None),
        "signed device, negative count": lambda: sgn_dev(fake, b, -1, 2.0, b192, b64, b128, None),
        "signed device, NaN beta": lambda: sgn_dev(fake, b, 1, nan, b192, b64, b128, None),
        "signed device, misaligned points": lambda: sgn_dev(fake, C.c_void_p(base + 8), 1, 2.0, b192, b64, b128, None),
        "signed device, misaligned records": lambda: sgn_dev(fake, b, 1, 2.0, b192, C.c_void_p(base + 72), b128, None),
        "signed device, misaligned values": lambda: sgn_dev(fake, b, 1, 2.0, C.c_void_p(base + 194), b64, b128, None),
        "signed device, misaligned instances": lambda: sgn_dev(fake, b, 1, 2.0, b192, b64, C.c_void_p(base + 130), None),
        "orientations, NULL set": lambda: lib.shray_instance_set_orientations(None, val),
        "orientations, NULL out": lambda: lib.shray_instance_set_orientations(fake, None),
    }
    for what, call in cases.items():
        assert call() == -1, what
        assert N.load_hip().shray_last_error(), what
    assert num(fake, pts, 0, 2.0, val, inst) == 0
    assert num(fake, pts, 0, inf, val, None) == 0
    assert sgn(fake, pts, 0, 0.0, val, None, None) == 0
    assert num_dev(fake, b, 0, 2.0, C.c_void_p(base + 196), None, None) == 0       # 4-byte alignment is enough
    assert sgn_dev(fake, b, 0, 2.0, C.c_void_p(base + 196), b64, C.c_void_p(base + 132), None) == 0
