"""include/shader_ray_instance_near.h against libshray_instance_near.so and the ctypes mirror: exactly the declared functions
are exported and bound, the header compiles as C, the library is a client of libshray_hip.so and libshray_instance.so, the
Python wrappers exist, and every argument refusal the header lists returns SHRAY_ERR_INVALID_ARGUMENT before any set or device
is touched, in point/first_k_query.h's order behind include/shader_ray_near.h's params check."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "shader_ray_instance_near.h")
FUNCTIONS = {"shray_near_triangles_instances_device", "shray_near_triangles_instances", "shray_near_triangles_instances_counters"}


def declared():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return set(re.findall(r"^\s*(?:int|void)\s+\**(shray_\w+)\s*\(", text, flags=re.M))


def test_header_symbols_are_exactly_the_exported_and_bound_ones(pkg):
    names = declared()
    assert names == FUNCTIONS
    assert names == {n for n, _, _ in pkg._native.INSTANCE_NEAR_SYMBOLS}
    lib = pkg._native.load_instance_near()
    out = subprocess.run(["nm", "-D", "--defined-only", pkg._native.INSTANCE_NEAR_LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\b[TW] (shrayi?_\w+)", out))
    assert exported == names, exported ^ names
    for n in names:
        assert getattr(lib, n).argtypes is not None
    needed = subprocess.run(["readelf", "-d", pkg._native.INSTANCE_NEAR_LIB], capture_output=True, text=True, check=True).stdout
    assert "libshray_instance.so" in needed and "libshray_hip.so" in needed
    assert "libshray_near.so" not in needed and "libshray_instance_point.so" not in needed


def test_the_header_compiles_as_c(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include "shader_ray_instance_near.h"\nint main(void) {\n'
                   '    int (*f)(shray_instance_set *, const shray_near_params *, const shray_point *, int64_t, shray_closest *, int32_t *,\n'
                   '             int32_t *, void *) = 0;\n'
                   '    (void)f;\n'
                   '    printf("%zu %zu %zu %d %d\\n", sizeof(shray_point), sizeof(shray_closest), sizeof(shray_near_params), (int)SHRAY_NEAR_MAX,\n'
                   '           (int)SHRAY_POINT_MAX_HEIGHT);\n    return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split() == ["16", "32", "16", "64", "128"]


def test_the_python_wrappers_are_bound(pkg):
    S = pkg.tracer.InstanceSet
    assert list(inspect.signature(S.triangles_within).parameters) == ["self", "points", "max_near", "counts", "counters"]
    assert list(inspect.signature(S.triangles_within_into).parameters) == ["self", "points_ptr", "count", "out_ptr", "instances_ptr",
                                                                          "counts_ptr", "max_near", "stream_ptr"]
    assert list(inspect.signature(S.near_counts).parameters) == ["self", "points"]
    assert inspect.signature(S.triangles_within).parameters["max_near"].default == 8
    assert callable(pkg._native.load_instance_near)
    assert os.path.basename(pkg._native.INSTANCE_NEAR_LIB) == "libshray_instance_near.so"


def params(pkg, k=8, size=None, reserved=(0, 0)):
    np_ = pkg._native.NearParams()
    np_.struct_size = C.sizeof(pkg._native.NearParams) if size is None else size
    np_.max_near = k
    np_.reserved[0], np_.reserved[1] = reserved
    return np_


def last_error(pkg):
    return pkg._native.load_hip().shray_last_error().decode()


def test_argument_errors(pkg):
    """Each call below fails with SHRAY_ERR_INVALID_ARGUMENT before it reads the (fake) set; count 0 with valid arguments is a
    no-op that needs no set data or device."""
    N = pkg._native
    lib = N.load_instance_near()
    host, dev, cnt = lib.shray_near_triangles_instances, lib.shray_near_triangles_instances_device, lib.shray_near_triangles_instances_counters
    pts = (N.Point * 2)()
    out = (N.Closest * 16)()
    inst = (C.c_int32 * 16)()
    counts = (C.c_int32 * 2)()
    c = N.Counters()
    buf = np.zeros(512, np.uint8)
    base = (buf.ctypes.data + 15) & ~15
    b, b64, b128, b192 = (C.c_void_p(base + o) for o in (0, 64, 128, 192))
    fake = C.c_void_p(1)   # never read
    ok, k0 = C.byref(params(pkg)), C.byref(params(pkg, 0))
    cases = {
        "NULL params": lambda: host(fake, None, pts, 2, out, inst, counts),
        "a wrong struct_size": lambda: host(fake, C.byref(params(pkg, size=12)), pts, 2, out, inst, counts),
        "K below 0": lambda: host(fake, C.byref(params(pkg, -1)), pts, 2, out, inst, counts),
        "K above SHRAY_NEAR_MAX": lambda: host(fake, C.byref(params(pkg, 65)), pts, 2, out, inst, counts),
        "a reserved field set": lambda: host(fake, C.byref(params(pkg, reserved=(0, 1))), pts, 2, out, inst, counts),
        "negative count": lambda: host(fake, ok, pts, -1, out, inst, counts),
        "NULL set": lambda: host(None, ok, pts, 2, out, inst, counts),
        "NULL points": lambda: host(fake, ok, None, 2, out, inst, counts),
        "NULL out with K > 0": lambda: host(fake, ok, pts, 2, None, inst, counts),
        "K = 0 and no counts": lambda: host(fake, k0, pts, 2, None, None, None),
        "counters, NULL counters": lambda: cnt(fake, ok, pts, 2, out, inst, counts, None),
        "counters, NULL params": lambda: cnt(fake, None, pts, 2, out, inst, counts, C.byref(c)),
        "counters, NULL set": lambda: cnt(None, ok, pts, 2, out, inst, counts, C.byref(c)),
        "counters, negative count": lambda: cnt(fake, ok, pts, -3, out, inst, counts, C.byref(c)),
        "counters, K = 0 and no counts": lambda: cnt(fake, k0, pts, 2, None, None, None, C.byref(c)),
        "device, NULL params": lambda: dev(fake, None, b, 1, b64, b128, b192, None),
        "device, K above SHRAY_NEAR_MAX": lambda: dev(fake, C.byref(params(pkg, 65)), b, 1, b64, b128, b192, None),
        "device, NULL set": lambda: dev(None, ok, b, 1, b64, b128, b192, None),
        "device, NULL points": lambda: dev(fake, ok, None, 1, b64, b128, b192, None),
        "device, NULL out with K > 0": lambda: dev(fake, ok, b, 1, None, b128, b192, None),
        "device, K = 0 and no counts": lambda: dev(fake, k0, b, 1, None, None, None, None),
        "device, negative count": lambda: dev(fake, ok, b, -1, b64, b128, b192, None),
        "device, misaligned points": lambda: dev(fake, ok, C.c_void_p(base + 4), 1, b64, b128, b192, None),
        "device, misaligned out": lambda: dev(fake, ok, b, 1, C.c_void_p(base + 72), b128, b192, None),
        "device, misaligned instances": lambda: dev(fake, ok, b, 1, b64, C.c_void_p(base + 130), b192, None),
        "device, misaligned counts": lambda: dev(fake, ok, b, 1, b64, b128, C.c_void_p(base + 193), None),
        "device, misaligned counts, count 0": lambda: dev(fake, ok, b, 0, b64, b128, C.c_void_p(base + 194), None),
    }
    for what, call in cases.items():
        assert call() == -1, what
        assert last_error(pkg), what
    assert host(fake, ok, pts, 0, out, inst, counts) == 0
    assert host(fake, ok, pts, 0, out, None, None) == 0
    assert host(fake, k0, pts, 0, None, None, counts) == 0
    assert dev(fake, ok, b, 0, b64, None, None, None) == 0
    assert dev(fake, ok, b, 0, b64, C.c_void_p(base + 132), C.c_void_p(base + 196), None) == 0      # 4-byte alignment is enough
    assert dev(fake, k0, b, 0, C.c_void_p(base + 72), None, b192, None) == 0        # with K = 0 the record pointer is not looked at
    c.samples = 99
    c.node_visits = 5
    assert cnt(fake, ok, pts, 0, out, None, None, C.byref(c)) == 0
    assert c.as_dict() == dict.fromkeys(c.as_dict(), 0)


def test_the_refusals_come_in_order(pkg):
    """Params first, then point/first_k_query.h's order: the count, the set and points, the records, nothing asked for; the
    alignments after them (device form)."""
    N = pkg._native
    dev = N.load_instance_near().shray_near_triangles_instances_device
    bad = C.byref(params(pkg, 65))
    ok, k0 = C.byref(params(pkg)), C.byref(params(pkg, 0))
    odd = C.c_void_p(20)
    assert dev(None, bad, None, -1, None, None, None, None) == -1 and "near params" in last_error(pkg)
    assert dev(None, ok, None, -1, None, None, None, None) == -1 and "negative point count" in last_error(pkg)
    assert dev(None, ok, None, 1, None, None, None, None) == -1 and "set or points is NULL" in last_error(pkg)
    assert dev(C.c_void_p(1), ok, odd, 1, None, None, None, None) == -1 and "out is NULL with max_near 8" in last_error(pkg)
    assert dev(C.c_void_p(1), k0, odd, 1, None, None, None, None) == -1 and "nothing is asked for" in last_error(pkg)
    assert dev(C.c_void_p(1), k0, odd, 1, None, None, C.c_void_p(64), None) == -1 and "aligned" in last_error(pkg)
