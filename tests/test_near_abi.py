"""include/shader_ray_near.h against libshray_near.so and the ctypes mirror: exactly the declared functions are exported and
bound, shray_near_params has the header's layout, SHRAY_NEAR_MAX is the mirror's, and every argument refusal the header lists
returns SHRAY_ERR_INVALID_ARGUMENT before any scene or device is touched."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "shader_ray_near.h")
FUNCTIONS = {"shray_near_params_init", "shray_near_triangles_device", "shray_near_triangles", "shray_near_triangles_counters"}


def declared():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return set(re.findall(r"^\s*(?:int|void)\s+\**(shray_\w+)\s*\(", text, flags=re.M))


def test_header_symbols_are_exactly_the_exported_and_bound_ones(pkg):
    names = declared()
    assert names == FUNCTIONS
    assert names == {n for n, _, _ in pkg._native.NEAR_SYMBOLS}
    lib = pkg._native.load_near()
    out = subprocess.run(["nm", "-D", "--defined-only", pkg._native.NEAR_LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\b[TW] (shrayi?_\w+)", out))
    assert exported == names, exported ^ names
    for n in names:
        assert getattr(lib, n).argtypes is not None


def test_params_layout_and_constants_match_the_header(pkg, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "shader_ray_near.h"\nint main(void) {\n'
                   '    printf("%zu %zu %zu %zu %zu %d %zu %zu\\n", sizeof(shray_near_params), offsetof(shray_near_params, struct_size),\n'
                   '           offsetof(shray_near_params, max_near), offsetof(shray_near_params, reserved),\n'
                   '           sizeof(((shray_near_params *)0)->reserved), (int)SHRAY_NEAR_MAX, sizeof(shray_point), sizeof(shray_closest));\n'
                   '    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    P = pkg._native.NearParams
    assert got == [C.sizeof(P), P.struct_size.offset, P.max_near.offset, P.reserved.offset, P.reserved.size,
                   pkg._native.NEAR_MAX, C.sizeof(pkg._native.Point), C.sizeof(pkg._native.Closest)]
    assert got == [16, 0, 4, 8, 8, 64, 16, 32]
    np_ = P()
    np_.reserved[0] = np_.reserved[1] = 9
    pkg._native.load_near().shray_near_params_init(C.byref(np_))
    assert (np_.struct_size, np_.max_near, np_.reserved[0], np_.reserved[1]) == (16, 8, 0, 0)
    pkg._native.load_near().shray_near_params_init(None)   # a no-op
    assert pkg.tracer.near_params(5).max_near == 5 and pkg.tracer.near_params().max_near == 8


def test_argument_errors(pkg):
    """Each call below fails with SHRAY_ERR_INVALID_ARGUMENT before it reads the (fake) scene; count 0 with valid arguments
    is a no-op that needs no scene data or device."""
    N = pkg._native
    lib = N.load_near()
    host, dev, cnt = lib.shray_near_triangles, lib.shray_near_triangles_device, lib.shray_near_triangles_counters
    pts = (N.Point * 2)()
    out = (N.Closest * 16)()
    counts = (C.c_int32 * 2)()
    tallies = N.Counters()
    buf = np.zeros(256, np.uint8)
    base = (buf.ctypes.data + 15) & ~15
    b, b64 = C.c_void_p(base), C.c_void_p(base + 64)
    fake = C.c_void_p(1)   # never read

    def params(max_near=8, reserved=(0, 0), struct_size=16):
        np_ = N.NearParams()
        np_.struct_size, np_.max_near = struct_size, max_near
        np_.reserved[0], np_.reserved[1] = reserved
        return C.byref(np_)

    cases = {
        "NULL scene": lambda: host(None, params(), pts, 2, out, counts),
        "NULL params": lambda: host(fake, None, pts, 2, out, counts),
        "NULL points": lambda: host(fake, params(), None, 2, out, counts),
        "NULL out with K > 0": lambda: host(fake, params(), pts, 2, None, counts),
        "both outputs NULL": lambda: host(fake, params(), pts, 2, None, None),
        "K == 0 and no counts": lambda: host(fake, params(0), pts, 2, None, None),
        "K == 0, out given, no counts": lambda: host(fake, params(0), pts, 2, out, None),
        "negative count": lambda: host(fake, params(), pts, -1, out, counts),
        "max_near -1": lambda: host(fake, params(-1), pts, 2, out, counts),
        "max_near 65": lambda: host(fake, params(65), pts, 2, out, counts),
        "reserved[0] 1": lambda: host(fake, params(8, (1, 0)), pts, 2, out, counts),
        "reserved[1] 1": lambda: host(fake, params(8, (0, 1)), pts, 2, out, counts),
        "struct_size 12": lambda: host(fake, params(struct_size=12), pts, 2, out, counts),
        "struct_size 20": lambda: host(fake, params(struct_size=20), pts, 2, out, counts),
        "device, NULL scene": lambda: dev(None, params(), b, 1, b64, None, None),
        "device, NULL params": lambda: dev(fake, None, b, 1, b64, None, None),
        "device, NULL points": lambda: dev(fake, params(), None, 1, b64, None, None),
        "device, NULL out with K > 0": lambda: dev(fake, params(), b, 1, None, b64, None),
        "device, both outputs NULL": lambda: dev(fake, params(0), b, 1, None, None, None),
        "device, negative count": lambda: dev(fake, params(), b, -1, b64, None, None),
        "device, max_near 65": lambda: dev(fake, params(65), b, 1, b64, None, None),
        "device, reserved": lambda: dev(fake, params(8, (0, 7)), b, 1, b64, None, None),
        "device, struct_size": lambda: dev(fake, params(struct_size=8), b, 1, b64, None, None),
        "device, misaligned points": lambda: dev(fake, params(), C.c_void_p(base + 4), 1, b64, None, None),
        "device, misaligned out": lambda: dev(fake, params(), b, 1, C.c_void_p(base + 72), None, None),
        "device, misaligned counts": lambda: dev(fake, params(), b, 1, b64, C.c_void_p(base + 130), None),
        "device, misaligned counts, K == 0": lambda: dev(fake, params(0), b, 1, None, C.c_void_p(base + 129), None),
        "counters, NULL counters": lambda: cnt(fake, params(), pts, 2, out, counts, None),
        "counters, NULL points": lambda: cnt(fake, params(), None, 2, out, counts, C.byref(tallies)),
        "counters, both outputs NULL": lambda: cnt(fake, params(), pts, 2, None, None, C.byref(tallies)),
        "counters, negative count": lambda: cnt(fake, params(), pts, -2, out, counts, C.byref(tallies)),
        "counters, max_near": lambda: cnt(fake, params(100), pts, 2, out, counts, C.byref(tallies)),
    }
    for what, call in cases.items():
        assert call() == -1, what
        assert N.load_hip().shray_last_error(), what
    assert host(fake, params(), pts, 0, out, counts) == 0
    assert host(fake, params(0), pts, 0, None, counts) == 0
    assert host(fake, params(64), pts, 0, out, None) == 0
    assert dev(fake, params(), b, 0, b64, None, None) == 0
    assert cnt(fake, params(), pts, 0, out, counts, C.byref(tallies)) == 0 and tallies.samples == 0


def test_refusal_texts(pkg):
    """One refusal of each kind leaves in shray_last_error() the text this library has always given for it."""
    N = pkg._native
    lib = N.load_near()
    host, cnt = lib.shray_near_triangles, lib.shray_near_triangles_counters
    pts, out, counts = (N.Point * 2)(), (N.Closest * 16)(), (C.c_int32 * 2)()
    fake = C.c_void_p(1)   # never read

    def params(max_near=8, struct_size=16):
        np_ = N.NearParams()
        np_.struct_size, np_.max_near = struct_size, max_near
        return C.byref(np_)

    cases = {
        "negative point count -1": lambda: host(fake, params(), pts, -1, out, counts),
        "scene or points is NULL": lambda: host(fake, params(), None, 2, out, counts),
        "out is NULL with max_near 8": lambda: host(fake, params(), pts, 2, None, counts),
        "nothing is asked for: max_near is 0 and counts is NULL": lambda: host(fake, params(0), pts, 2, None, None),
        "near params out of range (max_near 65 of 0 .. 64, reserved 0, 0)": lambda: host(fake, params(65), pts, 2, out, counts),
        "shray_near_params.struct_size is 12, this library expects 16": lambda: host(fake, params(struct_size=12), pts, 2, out, counts),
        "near params are NULL": lambda: host(fake, None, pts, 2, out, counts),
        "counters is NULL": lambda: cnt(fake, params(), pts, 2, out, counts, None),
    }
    for text, call in cases.items():
        assert call() == -1, text
        assert N.load_hip().shray_last_error().decode() == text
