"""include/shader_ray_winding.h against libshray_winding.so and the ctypes mirror: every declared function is exported and
bound, the record size is the header's, and bad arguments (NULL pointers, a negative count, a NaN or negative beta,
misaligned device buffers) are refused before any scene or device is touched."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "shader_ray_winding.h")


def declared():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return set(re.findall(r"^\s*(?:int|void)\s+\**(shray_\w+)\s*\(", text, flags=re.M))


def test_header_symbols_are_exported_and_bound(pkg):
    names = declared()
    assert names == {"shray_winding_number_device", "shray_winding_number", "shray_winding_signed_distance_device",
                     "shray_winding_signed_distance", "shray_scene_winding_data_download"}
    assert names == {n for n, _, _ in pkg._native.WINDING_SYMBOLS}
    lib = pkg._native.load_winding()
    out = subprocess.run(["nm", "-D", "--defined-only", pkg._native.WINDING_LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (shray_\w+)", out))
    assert names <= exported, names - exported
    for n in names:
        assert getattr(lib, n).argtypes is not None


def test_constants_match_the_header(pkg, tmp_path):
    src = tmp_path / "consts.c"
    src.write_text('#include <stdio.h>\n#include "shader_ray_winding.h"\nint main(void) {\n'
                   '    printf("%d %.9g\\n", (int)SHRAY_WINDING_DATA_FLOATS, (double)SHRAY_WINDING_BETA);\n    return 0;\n}\n')
    exe = tmp_path / "consts"
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    floats, beta = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert int(floats) == pkg._native.WINDING_DATA_FLOATS == 20 and float(beta) == 2.0


def test_argument_errors(pkg):
    """Each call below fails with SHRAY_ERR_INVALID_ARGUMENT before it reads the (fake) scene; count 0 with valid arguments is
    a no-op that needs no scene data or device."""
    N = pkg._native
    lib = N.load_winding()
    pts = (N.Point * 2)()
    out = (C.c_float * 2)()
    rec = (N.Closest * 2)()
    buf = np.zeros(64, np.uint8)
    base = (buf.ctypes.data + 15) & ~15
    fake = C.c_void_p(1)   # never read
    nan = float("nan")
    num, num_d = lib.shray_winding_number, lib.shray_winding_number_device
    sd, sd_d = lib.shray_winding_signed_distance, lib.shray_winding_signed_distance_device
    b = C.c_void_p(base)
    cases = {
        "NULL scene": lambda: num(None, pts, 2, 2.0, out),
        "NULL points": lambda: num(fake, None, 2, 2.0, out),
        "NULL out": lambda: num(fake, pts, 2, 2.0, None),
        "negative count": lambda: num(fake, pts, -1, 2.0, out),
        "NaN beta": lambda: num(fake, pts, 2, nan, out),
        "negative beta": lambda: num(fake, pts, 2, -0.5, out),
        "-inf beta": lambda: num(fake, pts, 2, float("-inf"), out),
        "device, NULL scene": lambda: num_d(None, b, 1, 2.0, b, None),
        "device, NULL points": lambda: num_d(fake, None, 1, 2.0, b, None),
        "device, NULL out": lambda: num_d(fake, b, 1, 2.0, None, None),
        "device, negative count": lambda: num_d(fake, b, -1, 2.0, b, None),
        "device, NaN beta": lambda: num_d(fake, b, 1, nan, b, None),
        "device, negative beta": lambda: num_d(fake, b, 1, -1.0, b, None),
        "device, misaligned points": lambda: num_d(fake, C.c_void_p(base + 4), 1, 2.0, b, None),
        "device, misaligned out": lambda: num_d(fake, b, 1, 2.0, C.c_void_p(base + 2), None),
        "signed, NULL scene": lambda: sd(None, pts, 2, 2.0, out, rec),
        "signed, NULL points": lambda: sd(fake, None, 2, 2.0, out, rec),
        "signed, NULL out": lambda: sd(fake, pts, 2, 2.0, None, rec),
        "signed, negative count": lambda: sd(fake, pts, -1, 2.0, out, None),
        "signed, NaN beta": lambda: sd(fake, pts, 2, nan, out, None),
        "signed device, NULL points": lambda: sd_d(fake, None, 1, 2.0, b, None, None),
        "signed device, negative beta": lambda: sd_d(fake, b, 1, -2.0, b, None, None),
        "signed device, misaligned points": lambda: sd_d(fake, C.c_void_p(base + 4), 1, 2.0, b, None, None),
        "signed device, misaligned records": lambda: sd_d(fake, b, 1, 2.0, b, C.c_void_p(base + 8), None),
        "signed device, misaligned signed": lambda: sd_d(fake, b, 1, 2.0, C.c_void_p(base + 2), None, None),
        "data, NULL scene": lambda: lib.shray_scene_winding_data_download(None, out),
        "data, NULL out": lambda: lib.shray_scene_winding_data_download(fake, None),
    }
    for what, call in cases.items():
        assert call() == -1, what
        assert N.load_hip().shray_last_error(), what
    assert num(fake, pts, 0, 2.0, out) == 0
    assert num(fake, pts, 0, float("inf"), out) == 0
    assert num_d(fake, b, 0, 2.0, b, None) == 0
    assert sd_d(fake, b, 0, 2.0, C.c_void_p(base + 4), None, None) == 0
