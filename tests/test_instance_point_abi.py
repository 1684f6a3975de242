"""include/shader_ray_instance_point.h against libshray_instance_point.so and the ctypes mirror: exactly the declared
functions are exported and bound, the header compiles as C, the instance library exports the accessor the new library reads a
set's forward maps through (and keeps it out of its header), the Python wrappers exist, and every argument refusal the header
lists returns SHRAY_ERR_INVALID_ARGUMENT before any set or device is touched."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "shader_ray_instance_point.h")
FUNCTIONS = {"shray_closest_points_instances_device", "shray_closest_points_instances", "shray_closest_points_instances_counters"}


def declared():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return set(re.findall(r"^\s*(?:int|void)\s+\**(shray_\w+)\s*\(", text, flags=re.M))


def test_header_symbols_are_exactly_the_exported_and_bound_ones(pkg):
    names = declared()
    assert names == FUNCTIONS
    assert names == {n for n, _, _ in pkg._native.INSTANCE_POINT_SYMBOLS}
    lib = pkg._native.load_instance_point()
    out = subprocess.run(["nm", "-D", "--defined-only", pkg._native.INSTANCE_POINT_LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\b[TW] (shrayi?_\w+)", out))
    assert exported == names, exported ^ names
    for n in names:
        assert getattr(lib, n).argtypes is not None


def test_the_header_compiles_as_c(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include "shader_ray_instance_point.h"\nint main(void) {\n'
                   '    int (*f)(shray_instance_set *, const shray_point *, int64_t, shray_closest *, int32_t *, void *) = 0;\n'
                   '    (void)f;\n'
                   '    printf("%zu %zu %d\\n", sizeof(shray_point), sizeof(shray_closest), (int)SHRAY_POINT_MAX_HEIGHT);\n    return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split() == ["16", "32", "128"]


def test_the_instance_library_exports_the_forward_maps_accessor(pkg):
    out = subprocess.run(["nm", "-D", "--defined-only", pkg._native.INSTANCE_LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (shray\w+)", out))
    assert "shrayi_instance_set_forward_maps" in exported and "shrayi_instance_set_device_arrays" in exported
    header = open(os.path.join(ROOT, "include", "shader_ray_instance.h")).read()
    assert "shrayi_instance_set_forward_maps" not in header
    assert "shrayi_instance_set_forward_maps" not in {n for n, _, _ in pkg._native.INSTANCE_SYMBOLS}
    needed = subprocess.run(["readelf", "-d", pkg._native.INSTANCE_POINT_LIB], capture_output=True, text=True, check=True).stdout
    assert "libshray_instance.so" in needed and "libshray_hip.so" in needed
    # a NULL set or a NULL result pointer is refused at the call
    lib = C.CDLL(pkg._native.INSTANCE_LIB)
    lib.shrayi_instance_set_forward_maps.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
    got = C.c_void_p(7)
    assert lib.shrayi_instance_set_forward_maps(None, None, C.byref(got)) == -1
    assert lib.shrayi_instance_set_forward_maps(C.c_void_p(1), None, None) == -1


def test_the_python_wrappers_are_bound(pkg):
    S = pkg.tracer.InstanceSet
    assert list(inspect.signature(S.closest_points).parameters) == ["self", "points", "max_dist2", "counters"]
    assert list(inspect.signature(S.closest_points_into).parameters) == ["self", "points_ptr", "count", "out_ptr", "instances_ptr",
                                                                        "stream_ptr"]
    assert callable(pkg._native.load_instance_point)


def test_argument_errors(pkg):
    """Each call below fails with SHRAY_ERR_INVALID_ARGUMENT before it reads the (fake) set; count 0 with valid arguments is a
    no-op that needs no set data or device."""
    N = pkg._native
    lib = N.load_instance_point()
    host, dev, cnt = lib.shray_closest_points_instances, lib.shray_closest_points_instances_device, lib.shray_closest_points_instances_counters
    pts = (N.Point * 2)()
    out = (N.Closest * 2)()
    inst = (C.c_int32 * 2)()
    c = N.Counters()
    buf = np.zeros(256, np.uint8)
    base = (buf.ctypes.data + 15) & ~15
    b, b64, b128 = C.c_void_p(base), C.c_void_p(base + 64), C.c_void_p(base + 128)
    fake = C.c_void_p(1)   # never read
    cases = {
        "NULL set": lambda: host(None, pts, 2, out, inst),
        "NULL points": lambda: host(fake, None, 2, out, inst),
        "NULL out": lambda: host(fake, pts, 2, None, inst),
        "negative count": lambda: host(fake, pts, -1, out, inst),
        "counters, NULL counters": lambda: cnt(fake, pts, 2, out, inst, None),
        "counters, NULL set": lambda: cnt(None, pts, 2, out, inst, C.byref(c)),
        "counters, NULL points": lambda: cnt(fake, None, 2, out, inst, C.byref(c)),
        "counters, negative count": lambda: cnt(fake, pts, -3, out, inst, C.byref(c)),
        "device, NULL set": lambda: dev(None, b, 1, b64, b128, None),
        "device, NULL points": lambda: dev(fake, None, 1, b64, b128, None),
        "device, NULL out": lambda: dev(fake, b, 1, None, b128, None),
        "device, negative count": lambda: dev(fake, b, -1, b64, b128, None),
        "device, misaligned points": lambda: dev(fake, C.c_void_p(base + 4), 1, b64, b128, None),
        "device, misaligned out": lambda: dev(fake, b, 1, C.c_void_p(base + 72), b128, None),
        "device, misaligned instances": lambda: dev(fake, b, 1, b64, C.c_void_p(base + 130), None),
        "device, misaligned instances, count 0": lambda: dev(fake, b, 0, b64, C.c_void_p(base + 129), None),
    }
    for what, call in cases.items():
        assert call() == -1, what
        assert N.load_hip().shray_last_error(), what
    assert host(fake, pts, 0, out, inst) == 0
    assert host(fake, pts, 0, out, None) == 0
    assert dev(fake, b, 0, b64, None, None) == 0
    assert dev(fake, b, 0, b64, C.c_void_p(base + 132), None) == 0      # 4-byte alignment is enough for the instances
    c.samples = 99
    c.node_visits = 5
    assert cnt(fake, pts, 0, None, None, C.byref(c)) == 0
    assert c.as_dict() == dict.fromkeys(c.as_dict(), 0)
