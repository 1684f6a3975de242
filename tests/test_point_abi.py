"""include/shader_ray_point.h against libshray_point.so and the ctypes mirror: every declared function is exported and bound,
shray_point and shray_closest lie as the compiled header lays them out, the record dtypes match, and bad arguments are refused
before any scene or device is touched."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import point_query_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "shader_ray_point.h")


def declared():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return set(re.findall(r"^\s*(?:int|void)\s+\**(shray_\w+)\s*\(", text, flags=re.M))


def test_header_symbols_are_exported_and_bound(pkg):
    names = declared()
    assert names == {"shray_closest_points_device", "shray_closest_points", "shray_closest_points_counters"}
    assert names == {n for n, _, _ in pkg._native.POINT_SYMBOLS}
    lib = pkg._native.load_point()
    out = subprocess.run(["nm", "-D", "--defined-only", pkg._native.POINT_LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (shray_\w+)", out))
    assert names <= exported, names - exported
    for n in names:
        assert getattr(lib, n).argtypes is not None


def test_layouts_match_the_header(pkg, tmp_path):
    src = tmp_path / "layout.c"
    fields = ["sizeof(shray_point)", "offsetof(shray_point, p)", "offsetof(shray_point, max_dist2)",
              "sizeof(shray_closest)", "offsetof(shray_closest, q)", "offsetof(shray_closest, dist2)", "offsetof(shray_closest, u)",
              "offsetof(shray_closest, v)", "offsetof(shray_closest, triangle)", "offsetof(shray_closest, region)",
              "SHRAY_POINT_MAX_HEIGHT", "SHRAY_REGION_A", "SHRAY_REGION_B", "SHRAY_REGION_C", "SHRAY_REGION_AB", "SHRAY_REGION_AC",
              "SHRAY_REGION_BC", "SHRAY_REGION_FACE", "SHRAY_REGION_NONE"]
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "shader_ray_point.h"\nint main(void) {\n'
                   + "".join(f'    printf("%lld\\n", (long long)({f}));\n' for f in fields) + "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    N = pkg._native
    P, Q = N.Point, N.Closest
    want = [C.sizeof(P), P.p.offset, P.max_dist2.offset, C.sizeof(Q), Q.q.offset, Q.dist2.offset, Q.u.offset, Q.v.offset,
            Q.triangle.offset, Q.region.offset, N.POINT_MAX_HEIGHT, N.REGION_A, N.REGION_B, N.REGION_C, N.REGION_AB, N.REGION_AC,
            N.REGION_BC, N.REGION_FACE, N.REGION_NONE]
    assert got == want
    assert got[0] == 16 and got[3] == 32
    T = pkg.tracer
    for dt, st in ((T.POINT_DTYPE, P), (T.CLOSEST_DTYPE, Q), (R.POINT_DTYPE, P), (R.CLOSEST_DTYPE, Q)):
        assert dt.itemsize == C.sizeof(st)
        assert [dt.fields[name][1] for name, _ in st._fields_] == [getattr(st, name).offset for name, _ in st._fields_]
    assert T.POINT_DTYPE == R.POINT_DTYPE and T.CLOSEST_DTYPE == R.CLOSEST_DTYPE


def test_argument_errors(pkg):
    """NULL pointers, a negative count and misaligned device buffers fail with SHRAY_ERR_INVALID_ARGUMENT; count 0 with
    valid pointers is a no-op that needs no scene data or device."""
    N = pkg._native
    lib = N.load_point()
    pts = (N.Point * 2)()
    out = (N.Closest * 2)()
    c = N.Counters()
    buf = np.zeros(64, np.uint8)
    base = (buf.ctypes.data + 15) & ~15
    fake = C.c_void_p(1)   # never read: every call below is refused (or a no-op) before the scene is touched
    cases = {
        "NULL scene": lambda: lib.shray_closest_points(None, pts, 2, out),
        "NULL points": lambda: lib.shray_closest_points(fake, None, 2, out),
        "NULL out": lambda: lib.shray_closest_points(fake, pts, 2, None),
        "negative count": lambda: lib.shray_closest_points(fake, pts, -1, out),
        "NULL counters": lambda: lib.shray_closest_points_counters(fake, pts, 2, out, None),
        "counters, negative count": lambda: lib.shray_closest_points_counters(fake, pts, -3, out, C.byref(c)),
        "device, NULL scene": lambda: lib.shray_closest_points_device(None, C.c_void_p(base), 1, C.c_void_p(base), None),
        "device, NULL points": lambda: lib.shray_closest_points_device(fake, None, 1, C.c_void_p(base), None),
        "device, NULL out": lambda: lib.shray_closest_points_device(fake, C.c_void_p(base), 1, None, None),
        "device, negative count": lambda: lib.shray_closest_points_device(fake, C.c_void_p(base), -1, C.c_void_p(base), None),
        "device, misaligned points": lambda: lib.shray_closest_points_device(fake, C.c_void_p(base + 4), 1, C.c_void_p(base), None),
        "device, misaligned out": lambda: lib.shray_closest_points_device(fake, C.c_void_p(base), 1, C.c_void_p(base + 8), None),
    }
    for what, call in cases.items():
        assert call() == -1, what
        assert N.load_hip().shray_last_error(), what
    assert lib.shray_closest_points(fake, pts, 0, out) == 0
    assert lib.shray_closest_points_device(fake, C.c_void_p(base), 0, C.c_void_p(base), None) == 0
    c.samples = 99
    c.node_visits = 5
    assert lib.shray_closest_points_counters(fake, pts, 0, None, C.byref(c)) == 0
    assert c.as_dict() == dict.fromkeys(c.as_dict(), 0)


def test_make_points(pkg):
    T = pkg.tracer
    p = T.make_points([[1, 2, 3], [4, 5, 6]])
    assert p.dtype == T.POINT_DTYPE and p["p"].tolist() == [[1, 2, 3], [4, 5, 6]] and np.isinf(p["max_dist2"]).all()
    p = T.make_points(np.zeros((3, 3)), max_dist2=[0, 1, 2])
    assert p["max_dist2"].tolist() == [0, 1, 2]
    q = T._host_points(np.arange(8, dtype=np.float32).reshape(2, 4), max_dist2=7)
    assert q["p"].tolist() == [[0, 1, 2], [4, 5, 6]] and q["max_dist2"].tolist() == [7, 7]
