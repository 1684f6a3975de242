"""include/shader_ray_sdf.h against libshray_sdf.so and the ctypes mirror: every declared function is exported and bound,
shray_surface_info lies as the compiled header lays it out, and bad arguments are refused before any scene or device is
touched."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "shader_ray_sdf.h")


def declared():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return set(re.findall(r"^\s*(?:int|void)\s+\**(shray_\w+)\s*\(", text, flags=re.M))


def test_header_symbols_are_exported_and_bound(pkg):
    names = declared()
    assert names == {"shray_signed_distance_device", "shray_signed_distance", "shray_scene_surface_info",
                     "shray_scene_sign_data_download"}
    assert names == {n for n, _, _ in pkg._native.SDF_SYMBOLS}
    lib = pkg._native.load_sdf()
    out = subprocess.run(["nm", "-D", "--defined-only", pkg._native.SDF_LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (shray_\w+)", out))
    assert names <= exported, names - exported
    for n in names:
        assert getattr(lib, n).argtypes is not None


def test_layouts_match_the_header(pkg, tmp_path):
    src = tmp_path / "layout.c"
    S = pkg._native.SurfaceInfo
    fields = ["sizeof(shray_surface_info)"] + [f"offsetof(shray_surface_info, {n})" for n, _ in S._fields_] + ["SHRAY_SIGN_DATA_FLOATS"]
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "shader_ray_sdf.h"\nint main(void) {\n'
                   + "".join(f'    printf("%lld\\n", (long long)({f}));\n' for f in fields) + "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert got == [C.sizeof(S)] + [getattr(S, n).offset for n, _ in S._fields_] + [pkg._native.SIGN_DATA_FLOATS]
    assert got[0] == 56 and got[-1] == 21


def test_argument_errors(pkg):
    """NULL pointers, a negative count and misaligned device buffers fail with SHRAY_ERR_INVALID_ARGUMENT; count 0 with
    valid pointers is a no-op that needs no scene data or device."""
    N = pkg._native
    lib = N.load_sdf()
    pts = (N.Point * 2)()
    out = (C.c_float * 2)()
    rec = (N.Closest * 2)()
    info = N.SurfaceInfo()
    buf = np.zeros(64, np.uint8)
    base = (buf.ctypes.data + 15) & ~15
    fake = C.c_void_p(1)   # never read: every call below is refused (or a no-op) before the scene is touched
    dev = lib.shray_signed_distance_device
    cases = {
        "NULL scene": lambda: lib.shray_signed_distance(None, pts, 2, out, rec),
        "NULL points": lambda: lib.shray_signed_distance(fake, None, 2, out, rec),
        "NULL signed": lambda: lib.shray_signed_distance(fake, pts, 2, None, rec),
        "negative count": lambda: lib.shray_signed_distance(fake, pts, -1, out, None),
        "device, NULL scene": lambda: dev(None, C.c_void_p(base), 1, C.c_void_p(base), None, None),
        "device, NULL points": lambda: dev(fake, None, 1, C.c_void_p(base), None, None),
        "device, NULL signed": lambda: dev(fake, C.c_void_p(base), 1, None, C.c_void_p(base), None),
        "device, negative count": lambda: dev(fake, C.c_void_p(base), -1, C.c_void_p(base), None, None),
        "device, misaligned points": lambda: dev(fake, C.c_void_p(base + 4), 1, C.c_void_p(base), None, None),
        "device, misaligned records": lambda: dev(fake, C.c_void_p(base), 1, C.c_void_p(base), C.c_void_p(base + 8), None),
        "device, misaligned signed": lambda: dev(fake, C.c_void_p(base), 1, C.c_void_p(base + 2), None, None),
        "surface_info, NULL scene": lambda: lib.shray_scene_surface_info(None, C.byref(info)),
        "surface_info, NULL info": lambda: lib.shray_scene_surface_info(fake, None),
        "sign data, NULL scene": lambda: lib.shray_scene_sign_data_download(None, out),
        "sign data, NULL out": lambda: lib.shray_scene_sign_data_download(fake, None),
    }
    for what, call in cases.items():
        assert call() == -1, what
        assert N.load_hip().shray_last_error(), what
    assert lib.shray_signed_distance(fake, pts, 0, out, None) == 0
    assert dev(fake, C.c_void_p(base), 0, C.c_void_p(base + 4), None, None) == 0
