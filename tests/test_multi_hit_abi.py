"""include/shader_ray_multihit.h against libshray_multihit.so and the ctypes mirror: exactly the declared functions are
exported and bound, shray_multihit_params has the header's layout, SHRAY_MULTIHIT_MAX is the mirror's, and every argument
refusal the header lists returns SHRAY_ERR_INVALID_ARGUMENT before any scene or device is touched."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "shader_ray_multihit.h")
FUNCTIONS = {"shray_multihit_params_init", "shray_trace_all_hits_device", "shray_trace_all_hits", "shray_trace_all_hits_counters"}


def declared():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return set(re.findall(r"^\s*(?:int|void)\s+\**(shray_\w+)\s*\(", text, flags=re.M))


def test_header_symbols_are_exactly_the_exported_and_bound_ones(pkg):
    names = declared()
    assert names == FUNCTIONS
    assert names == {n for n, _, _ in pkg._native.MULTIHIT_SYMBOLS}
    lib = pkg._native.load_multihit()
    out = subprocess.run(["nm", "-D", "--defined-only", pkg._native.MULTIHIT_LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\b[TW] (shrayi?_\w+)", out))
    assert exported == names, exported ^ names
    for n in names:
        assert getattr(lib, n).argtypes is not None


def test_params_layout_and_constants_match_the_header(pkg, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "shader_ray_multihit.h"\nint main(void) {\n'
                   '    printf("%zu %zu %zu %zu %zu %d %zu %zu\\n", sizeof(shray_multihit_params), offsetof(shray_multihit_params, struct_size),\n'
                   '           offsetof(shray_multihit_params, max_hits), offsetof(shray_multihit_params, max_leaf_tests),\n'
                   '           offsetof(shray_multihit_params, reserved), (int)SHRAY_MULTIHIT_MAX, sizeof(shray_ray), sizeof(shray_hit));\n'
                   '    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    P = pkg._native.MultihitParams
    assert got == [C.sizeof(P), P.struct_size.offset, P.max_hits.offset, P.max_leaf_tests.offset, P.reserved.offset,
                   pkg._native.MULTIHIT_MAX, C.sizeof(pkg._native.Ray), C.sizeof(pkg._native.Hit)]
    assert got == [16, 0, 4, 8, 12, 64, 32, 16]
    mp = P()
    pkg._native.load_multihit().shray_multihit_params_init(C.byref(mp))
    assert (mp.struct_size, mp.max_hits, mp.max_leaf_tests, mp.reserved) == (16, 8, 10, 0)
    pkg._native.load_multihit().shray_multihit_params_init(None)   # a no-op


def test_argument_errors(pkg):
    """Each call below fails with SHRAY_ERR_INVALID_ARGUMENT before it reads the (fake) scene; count 0 with valid arguments
    is a no-op that needs no scene data or device."""
    N = pkg._native
    lib = N.load_multihit()
    host, dev, cnt = lib.shray_trace_all_hits, lib.shray_trace_all_hits_device, lib.shray_trace_all_hits_counters
    rays = (N.Ray * 2)()
    hits = (N.Hit * 16)()
    counts = (C.c_int32 * 2)()
    tallies = N.Counters()
    buf = np.zeros(256, np.uint8)
    base = (buf.ctypes.data + 15) & ~15
    b, b64 = C.c_void_p(base), C.c_void_p(base + 64)
    fake = C.c_void_p(1)   # never read

    def params(max_hits=8, max_leaf_tests=10, reserved=0, struct_size=16):
        mp = N.MultihitParams()
        mp.struct_size, mp.max_hits, mp.max_leaf_tests, mp.reserved = struct_size, max_hits, max_leaf_tests, reserved
        return C.byref(mp)

    cases = {
        "NULL scene": lambda: host(None, params(), rays, 2, hits, counts),
        "NULL params": lambda: host(fake, None, rays, 2, hits, counts),
        "NULL rays": lambda: host(fake, params(), None, 2, hits, counts),
        "NULL hits with K > 0": lambda: host(fake, params(), rays, 2, None, counts),
        "both outputs NULL": lambda: host(fake, params(), rays, 2, None, None),
        "K == 0 and no counts": lambda: host(fake, params(0), rays, 2, None, None),
        "K == 0, hits given, no counts": lambda: host(fake, params(0), rays, 2, hits, None),
        "negative count": lambda: host(fake, params(), rays, -1, hits, counts),
        "max_hits -1": lambda: host(fake, params(-1), rays, 2, hits, counts),
        "max_hits 65": lambda: host(fake, params(65), rays, 2, hits, counts),
        "max_leaf_tests -1": lambda: host(fake, params(8, -1), rays, 2, hits, counts),
        "reserved 1": lambda: host(fake, params(8, 10, 1), rays, 2, hits, counts),
        "struct_size 12": lambda: host(fake, params(struct_size=12), rays, 2, hits, counts),
        "struct_size 20": lambda: host(fake, params(struct_size=20), rays, 2, hits, counts),
        "device, NULL scene": lambda: dev(None, params(), b, 1, b64, None, None),
        "device, NULL params": lambda: dev(fake, None, b, 1, b64, None, None),
        "device, NULL rays": lambda: dev(fake, params(), None, 1, b64, None, None),
        "device, NULL hits with K > 0": lambda: dev(fake, params(), b, 1, None, b64, None),
        "device, both outputs NULL": lambda: dev(fake, params(0), b, 1, None, None, None),
        "device, negative count": lambda: dev(fake, params(), b, -1, b64, None, None),
        "device, max_hits 65": lambda: dev(fake, params(65), b, 1, b64, None, None),
        "device, reserved": lambda: dev(fake, params(8, 10, 7), b, 1, b64, None, None),
        "device, struct_size": lambda: dev(fake, params(struct_size=8), b, 1, b64, None, None),
        "device, misaligned rays": lambda: dev(fake, params(), C.c_void_p(base + 4), 1, b64, None, None),
        "device, misaligned hits": lambda: dev(fake, params(), b, 1, C.c_void_p(base + 72), None, None),
        "device, misaligned counts": lambda: dev(fake, params(), b, 1, b64, C.c_void_p(base + 130), None),
        "device, misaligned counts, K == 0": lambda: dev(fake, params(0), b, 1, None, C.c_void_p(base + 129), None),
        "counters, NULL counters": lambda: cnt(fake, params(), rays, 2, hits, counts, None),
        "counters, NULL rays": lambda: cnt(fake, params(), None, 2, hits, counts, C.byref(tallies)),
        "counters, both outputs NULL": lambda: cnt(fake, params(), rays, 2, None, None, C.byref(tallies)),
        "counters, negative count": lambda: cnt(fake, params(), rays, -2, hits, counts, C.byref(tallies)),
        "counters, max_hits": lambda: cnt(fake, params(100), rays, 2, hits, counts, C.byref(tallies)),
    }
    for what, call in cases.items():
        assert call() == -1, what
        assert N.load_hip().shray_last_error(), what
    assert host(fake, params(), rays, 0, hits, counts) == 0
    assert host(fake, params(0), rays, 0, None, counts) == 0
    assert host(fake, params(64), rays, 0, hits, None) == 0
    assert dev(fake, params(), b, 0, b64, None, None) == 0
    assert cnt(fake, params(), rays, 0, hits, counts, C.byref(tallies)) == 0 and tallies.samples == 0


def test_refusal_texts(pkg):
    """One refusal of each kind leaves in shray_last_error() the text this library has always given for it."""
    N = pkg._native
    lib = N.load_multihit()
    host, cnt = lib.shray_trace_all_hits, lib.shray_trace_all_hits_counters
    rays, hits, counts = (N.Ray * 2)(), (N.Hit * 16)(), (C.c_int32 * 2)()
    fake = C.c_void_p(1)   # never read

    def params(max_hits=8, max_leaf_tests=10, struct_size=16):
        mp = N.MultihitParams()
        mp.struct_size, mp.max_hits, mp.max_leaf_tests, mp.reserved = struct_size, max_hits, max_leaf_tests, 0
        return C.byref(mp)

    cases = {
        "negative ray count -1": lambda: host(fake, params(), rays, -1, hits, counts),
        "scene or rays is NULL": lambda: host(fake, params(), None, 2, hits, counts),
        "hits is NULL with max_hits 8": lambda: host(fake, params(), rays, 2, None, counts),
        "nothing is asked for: max_hits is 0 and counts is NULL": lambda: host(fake, params(0), rays, 2, None, None),
        "multihit params out of range (max_hits 65 of 0 .. 64, max_leaf_tests 10, reserved 0)":
            lambda: host(fake, params(65), rays, 2, hits, counts),
        "shray_multihit_params.struct_size is 12, this library expects 16": lambda: host(fake, params(struct_size=12), rays, 2, hits, counts),
        "multihit params are NULL": lambda: host(fake, None, rays, 2, hits, counts),
        "counters is NULL": lambda: cnt(fake, params(), rays, 2, hits, counts, None),
    }
    for text, call in cases.items():
        assert call() == -1, text
        assert N.load_hip().shray_last_error().decode() == text
