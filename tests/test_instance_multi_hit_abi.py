"""include/shader_ray_instance_multihit.h against libshray_instance_multihit.so and the ctypes mirror: exactly the declared
functions are exported and bound, the header compiles as C, the instance library exports the accessor the new library reads
a set through (and keeps it out of its header), the Python wrappers exist, and every argument refusal the header lists
returns SHRAY_ERR_INVALID_ARGUMENT before any set or device is touched."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "shader_ray_instance_multihit.h")
FUNCTIONS = {"shray_trace_instances_all_hits_device", "shray_trace_instances_all_hits", "shray_trace_instances_all_hits_counters"}


def declared():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return set(re.findall(r"^\s*(?:int|void)\s+\**(shray_\w+)\s*\(", text, flags=re.M))


def test_header_symbols_are_exactly_the_exported_and_bound_ones(pkg):
    names = declared()
    assert names == FUNCTIONS
    assert names == {n for n, _, _ in pkg._native.INSTANCE_MULTIHIT_SYMBOLS}
    lib = pkg._native.load_instance_multihit()
    out = subprocess.run(["nm", "-D", "--defined-only", pkg._native.INSTANCE_MULTIHIT_LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\b[TW] (shrayi?_\w+)", out))
    assert exported == names, exported ^ names
    for n in names:
        assert getattr(lib, n).argtypes is not None


def test_the_header_compiles_as_c(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include "shader_ray_instance_multihit.h"\nint main(void) {\n'
                   '    int (*f)(shray_instance_set *, const shray_multihit_params *, const shray_ray *, int64_t, shray_hit *, int32_t *,\n'
                   '             int32_t *, void *) = 0;\n'
                   '    (void)f;\n'
                   '    printf("%zu %d\\n", sizeof(shray_multihit_params), (int)SHRAY_MULTIHIT_MAX);\n    return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split() == ["16", "64"]


def test_the_instance_library_exports_the_device_arrays_accessor(pkg):
    out = subprocess.run(["nm", "-D", "--defined-only", pkg._native.INSTANCE_LIB], capture_output=True, text=True, check=True).stdout
    assert "shrayi_instance_set_device_arrays" in set(re.findall(r"\bT (shray\w+)", out))
    assert "shrayi_instance_set_device_arrays" not in open(os.path.join(ROOT, "include", "shader_ray_instance.h")).read()
    needed = subprocess.run(["readelf", "-d", pkg._native.INSTANCE_MULTIHIT_LIB], capture_output=True, text=True, check=True).stdout
    assert "libshray_instance.so" in needed and "libshray_hip.so" in needed


def test_the_python_wrappers_are_bound(pkg):
    S = pkg.tracer.InstanceSet
    for name in ("trace_all_hits", "trace_all_hits_into", "crossing_counts"):
        assert callable(getattr(S, name))
    import inspect
    assert list(inspect.signature(S.trace_all_hits).parameters) == ["self", "rays", "max_hits", "counts", "max_leaf_tests", "counters"]
    assert list(inspect.signature(S.trace_all_hits_into).parameters) == ["self", "rays_ptr", "count", "hits_ptr", "instances_ptr", "counts_ptr",
                                                                        "max_hits", "stream_ptr", "max_leaf_tests"]


def test_argument_errors(pkg):
    """Each call below fails with SHRAY_ERR_INVALID_ARGUMENT before it reads the (fake) set; count 0 with valid arguments is a
    no-op that needs no set data or device."""
    N = pkg._native
    lib = N.load_instance_multihit()
    host, dev, cnt = lib.shray_trace_instances_all_hits, lib.shray_trace_instances_all_hits_device, lib.shray_trace_instances_all_hits_counters
    rays = (N.Ray * 2)()
    hits = (N.Hit * 16)()
    inst = (C.c_int32 * 16)()
    counts = (C.c_int32 * 2)()
    tallies = N.Counters()
    buf = np.zeros(512, np.uint8)
    base = (buf.ctypes.data + 15) & ~15
    b, b64, b256 = C.c_void_p(base), C.c_void_p(base + 64), C.c_void_p(base + 256)
    fake = C.c_void_p(1)   # never read

    def params(max_hits=8, max_leaf_tests=10, reserved=0, struct_size=16):
        mp = N.MultihitParams()
        mp.struct_size, mp.max_hits, mp.max_leaf_tests, mp.reserved = struct_size, max_hits, max_leaf_tests, reserved
        return C.byref(mp)

    cases = {
        "NULL set": lambda: host(None, params(), rays, 2, hits, inst, counts),
        "NULL params": lambda: host(fake, None, rays, 2, hits, inst, counts),
        "NULL rays": lambda: host(fake, params(), None, 2, hits, inst, counts),
        "NULL hits with K > 0": lambda: host(fake, params(), rays, 2, None, inst, counts),
        "K == 0 and no counts": lambda: host(fake, params(0), rays, 2, None, None, None),
        "K == 0, hits and instances given, no counts": lambda: host(fake, params(0), rays, 2, hits, inst, None),
        "negative count": lambda: host(fake, params(), rays, -1, hits, inst, counts),
        "max_hits -1": lambda: host(fake, params(-1), rays, 2, hits, inst, counts),
        "max_hits 65": lambda: host(fake, params(65), rays, 2, hits, inst, counts),
        "max_leaf_tests -1": lambda: host(fake, params(8, -1), rays, 2, hits, inst, counts),
        "reserved 1": lambda: host(fake, params(8, 10, 1), rays, 2, hits, inst, counts),
        "struct_size 12": lambda: host(fake, params(struct_size=12), rays, 2, hits, inst, counts),
        "struct_size 20": lambda: host(fake, params(struct_size=20), rays, 2, hits, inst, counts),
        "device, NULL set": lambda: dev(None, params(), b, 1, b64, None, None, None),
        "device, NULL params": lambda: dev(fake, None, b, 1, b64, None, None, None),
        "device, NULL rays": lambda: dev(fake, params(), None, 1, b64, None, None, None),
        "device, NULL hits with K > 0": lambda: dev(fake, params(), b, 1, None, b256, b256, None),
        "device, K == 0 and no counts": lambda: dev(fake, params(0), b, 1, None, None, None, None),
        "device, negative count": lambda: dev(fake, params(), b, -1, b64, None, None, None),
        "device, max_hits 65": lambda: dev(fake, params(65), b, 1, b64, None, None, None),
        "device, reserved": lambda: dev(fake, params(8, 10, 7), b, 1, b64, None, None, None),
        "device, struct_size": lambda: dev(fake, params(struct_size=8), b, 1, b64, None, None, None),
        "device, misaligned rays": lambda: dev(fake, params(), C.c_void_p(base + 4), 1, b64, None, None, None),
        "device, misaligned hits": lambda: dev(fake, params(), b, 1, C.c_void_p(base + 72), None, None, None),
        "device, misaligned instances": lambda: dev(fake, params(), b, 1, b64, C.c_void_p(base + 258), None, None),
        "device, misaligned counts": lambda: dev(fake, params(), b, 1, b64, None, C.c_void_p(base + 258), None),
        "device, misaligned counts, K == 0": lambda: dev(fake, params(0), b, 1, None, None, C.c_void_p(base + 257), None),
        "counters, NULL counters": lambda: cnt(fake, params(), rays, 2, hits, inst, counts, None),
        "counters, NULL rays": lambda: cnt(fake, params(), None, 2, hits, inst, counts, C.byref(tallies)),
        "counters, K == 0 and no counts": lambda: cnt(fake, params(0), rays, 2, None, None, None, C.byref(tallies)),
        "counters, negative count": lambda: cnt(fake, params(), rays, -2, hits, inst, counts, C.byref(tallies)),
        "counters, max_hits": lambda: cnt(fake, params(100), rays, 2, hits, inst, counts, C.byref(tallies)),
    }
    for what, call in cases.items():
        assert call() == -1, what
        assert N.load_hip().shray_last_error(), what
    assert host(fake, params(), rays, 0, hits, inst, counts) == 0
    assert host(fake, params(0), rays, 0, None, None, counts) == 0
    assert host(fake, params(64), rays, 0, hits, None, None) == 0
    assert dev(fake, params(), b, 0, b64, None, None, None) == 0
    assert cnt(fake, params(), rays, 0, hits, inst, counts, C.byref(tallies)) == 0 and tallies.samples == 0


def test_refusal_texts(pkg):
    """One refusal of each kind leaves in shray_last_error() the text this library has always given for it."""
    N = pkg._native
    lib = N.load_instance_multihit()
    host, cnt = lib.shray_trace_instances_all_hits, lib.shray_trace_instances_all_hits_counters
    rays, hits, inst, counts = (N.Ray * 2)(), (N.Hit * 16)(), (C.c_int32 * 16)(), (C.c_int32 * 2)()
    fake = C.c_void_p(1)   # never read

    def params(max_hits=8, max_leaf_tests=10, struct_size=16):
        mp = N.MultihitParams()
        mp.struct_size, mp.max_hits, mp.max_leaf_tests, mp.reserved = struct_size, max_hits, max_leaf_tests, 0
        return C.byref(mp)

    cases = {
        "negative ray count -1": lambda: host(fake, params(), rays, -1, hits, inst, counts),
        "set or rays is NULL": lambda: host(fake, params(), None, 2, hits, inst, counts),
        "hits is NULL with max_hits 8": lambda: host(fake, params(), rays, 2, None, inst, counts),
        "nothing is asked for: max_hits is 0 and counts is NULL": lambda: host(fake, params(0), rays, 2, None, None, None),
        "multihit params out of range (max_hits 65 of 0 .. 64, max_leaf_tests 10, reserved 0)":
            lambda: host(fake, params(65), rays, 2, hits, inst, counts),
        "shray_multihit_params.struct_size is 12, this library expects 16":
            lambda: host(fake, params(struct_size=12), rays, 2, hits, inst, counts),
        "multihit params are NULL": lambda: host(fake, None, rays, 2, hits, inst, counts),
        "counters is NULL": lambda: cnt(fake, params(), rays, 2, hits, inst, counts, None),
    }
    for text, call in cases.items():
        assert call() == -1, text
        assert N.load_hip().shray_last_error().decode() == text
