"""include/shader_ray_instance_pairs.h against libshray_instance_pairs.so and the ctypes mirror: exactly the declared functions
are exported and bound, the header compiles as C with a 16-byte shray_pairs_params and the stated flag values, the library is
a client of libshray_hip.so and libshray_instance.so and of none of libshray_intersect.so, libshray_instance_intersect.so and
libshray_instance_point.so, the Python wrappers exist, and every refusal that comes before the set is read returns
SHRAY_ERR_INVALID_ARGUMENT, in the header's order: the params, the misuse of SHRAY_PAIRS_ANY, a negative row range, a NULL
set.  (The refusals from the fifth on read the set -- rows beyond it, both outputs NULL, the alignment -- and are in
tests/test_gpu_instance_pairs.py.)"""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "shader_ray_instance_pairs.h")
FUNCTIONS = {"shray_instance_pairs_intersect_device", "shray_instance_pairs_intersect", "shray_instance_pairs_intersect_counters"}


def declared():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return set(re.findall(r"^\s*(?:int|void)\s+\**(shray_\w+)\s*\(", text, flags=re.M))


def test_header_symbols_are_exactly_the_exported_and_bound_ones(pkg):
    names = declared()
    assert names == FUNCTIONS
    assert names == {n for n, _, _ in pkg._native.INSTANCE_PAIRS_SYMBOLS}
    lib = pkg._native.load_instance_pairs()
    out = subprocess.run(["nm", "-D", "--defined-only", pkg._native.INSTANCE_PAIRS_LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\b[TW] (shrayi?_\w+)", out))
    assert exported == names, exported ^ names
    for n in names:
        assert getattr(lib, n).argtypes is not None


def test_the_library_needs_two_libraries_and_not_the_three_it_restates(pkg):
    needed = subprocess.run(["readelf", "-d", pkg._native.INSTANCE_PAIRS_LIB], capture_output=True, text=True, check=True).stdout
    assert "libshray_instance.so" in needed and "libshray_hip.so" in needed
    for other in ("libshray_intersect.so", "libshray_instance_intersect.so", "libshray_instance_point.so"):
        assert other not in needed, other


def test_the_header_compiles_as_c(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "shader_ray_instance_pairs.h"\nint main(void) {\n'
                   '    int (*f)(shray_instance_set *, const shray_pairs_params *, uint64_t *, int64_t *, void *) = 0;\n'
                   '    int (*g)(shray_instance_set *, const shray_pairs_params *, uint64_t *, int64_t *, shray_counters *) = 0;\n'
                   '    (void)f;\n    (void)g;\n'
                   '    printf("%zu %zu %zu %zu %zu %d %d %d %d %u %d\\n", sizeof(shray_pairs_params), offsetof(shray_pairs_params, struct_size),\n'
                   '           offsetof(shray_pairs_params, flags), offsetof(shray_pairs_params, first_row), offsetof(shray_pairs_params, row_count),\n'
                   '           (int)SHRAY_PAIRS_ANY, (int)SHRAY_PAIRS_SKIP_SHARED, (int)SHRAY_PAIRS_UPPER, SHRAY_PAIRS_NONE == UINT64_MAX,\n'
                   '           (unsigned)SHRAY_PAIRS_MAX_WORKGROUPS, (int)SHRAY_POINT_MAX_HEIGHT);\n    return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split() == \
        ["16", "0", "4", "8", "12", "1", "2", "4", "1", str(1 << 24), "128"]


def test_the_python_wrappers_are_bound(pkg):
    S = pkg.tracer.InstanceSet
    N = pkg._native
    names = lambda f: list(inspect.signature(f).parameters)
    assert names(S.collision_matrix) == ["self", "rows", "upper", "skip_shared"]
    assert names(S.collision_pairs) == ["self", "rows", "counts", "upper", "skip_shared", "counters", "device"]
    assert names(S.collision_pairs_into) == ["self", "first_ptr", "counts_ptr", "first_row", "row_count", "any_only", "upper", "skip_shared",
                                             "stream_ptr"]
    assert names(S.colliding_pairs) == ["self", "upper"]
    assert names(S.instances_colliding) == ["self"]
    p = inspect.signature(S.collision_pairs).parameters
    assert p["rows"].default is None and p["counts"].default is True and p["upper"].default is False and p["skip_shared"].default is False
    assert p["counters"].default is False and p["device"].default is False
    p = inspect.signature(S.collision_pairs_into).parameters
    assert p["first_row"].default == 0 and p["row_count"].default is None and p["any_only"].default is False and p["stream_ptr"].default == 0
    assert inspect.signature(S.colliding_pairs).parameters["upper"].default is True
    assert inspect.signature(S.collision_matrix).parameters["upper"].default is False
    assert callable(N.load_instance_pairs) and os.path.basename(N.INSTANCE_PAIRS_LIB) == "libshray_instance_pairs.so"
    assert (N.PAIRS_ANY, N.PAIRS_SKIP_SHARED, N.PAIRS_UPPER, N.PAIRS_NONE, N.PAIRS_MAX_WORKGROUPS) == (1, 2, 4, 2 ** 64 - 1, 1 << 24)
    assert C.sizeof(N.PairsParams) == 16
    op = pkg.tracer._pairs_params(3, 4, True, True, True)
    assert (op.struct_size, op.flags, op.first_row, op.row_count) == (16, 7, 3, 4)
    assert pkg.tracer._pairs_params(0, 9).flags == 0


def params(pkg, first_row=0, row_count=1, flags=0, size=None):
    op = pkg._native.PairsParams()
    op.struct_size = C.sizeof(pkg._native.PairsParams) if size is None else size
    op.flags, op.first_row, op.row_count = flags, first_row, row_count
    return op


def last_error(pkg):
    return pkg._native.load_hip().shray_last_error().decode()


def test_argument_errors(pkg):
    """Each call below fails with SHRAY_ERR_INVALID_ARGUMENT before it reads the (fake) set."""
    N = pkg._native
    lib = N.load_instance_pairs()
    host, dev, cnt = lib.shray_instance_pairs_intersect, lib.shray_instance_pairs_intersect_device, lib.shray_instance_pairs_intersect_counters
    buf = np.zeros(512, np.uint8)
    base = (buf.ctypes.data + 15) & ~15
    first, counts = C.c_void_p(base), C.c_void_p(base + 128)
    c = N.Counters()
    fake = C.c_void_p(1)   # never read
    ok, any_ = C.byref(params(pkg)), C.byref(params(pkg, flags=N.PAIRS_ANY))
    cases = {
        "NULL params": lambda: host(fake, None, first, counts),
        "a wrong struct_size": lambda: host(fake, C.byref(params(pkg, size=12)), first, counts),
        "an unknown flag": lambda: host(fake, C.byref(params(pkg, flags=8)), first, counts),
        "an unknown flag beside known ones": lambda: host(fake, C.byref(params(pkg, flags=7 | 16)), None, counts),
        "ANY with first": lambda: host(fake, any_, first, counts),
        "ANY without counts": lambda: host(fake, any_, None, None),
        "ANY | UPPER with first": lambda: host(fake, C.byref(params(pkg, flags=N.PAIRS_ANY | N.PAIRS_UPPER)), first, None),
        "a negative first row": lambda: host(fake, C.byref(params(pkg, -1, 1)), first, counts),
        "a negative row count": lambda: host(fake, C.byref(params(pkg, 0, -1)), first, counts),
        "NULL set": lambda: host(None, ok, first, counts),
        "NULL set, no rows": lambda: host(None, C.byref(params(pkg, 0, 0)), first, counts),
        "counters, NULL counters": lambda: cnt(fake, ok, first, counts, None),
        "counters, NULL params": lambda: cnt(fake, None, first, counts, C.byref(c)),
        "counters, ANY with first": lambda: cnt(fake, any_, first, counts, C.byref(c)),
        "counters, a negative row count": lambda: cnt(fake, C.byref(params(pkg, 2, -2)), first, counts, C.byref(c)),
        "counters, NULL set": lambda: cnt(None, ok, first, counts, C.byref(c)),
        "device, NULL params": lambda: dev(fake, None, first, counts, None),
        "device, a wrong struct_size": lambda: dev(fake, C.byref(params(pkg, size=20)), first, counts, None),
        "device, an unknown flag": lambda: dev(fake, C.byref(params(pkg, flags=1 << 31)), first, counts, None),
        "device, ANY with first": lambda: dev(fake, any_, first, counts, None),
        "device, ANY without counts": lambda: dev(fake, any_, None, None, None),
        "device, a negative first row": lambda: dev(fake, C.byref(params(pkg, -3, 0)), first, counts, None),
        "device, NULL set": lambda: dev(None, ok, first, counts, None),
    }
    for what, call in cases.items():
        assert call() == -1, what
        assert last_error(pkg), what


def test_the_refusals_come_in_order(pkg):
    """The params first, then the misuse of SHRAY_PAIRS_ANY, then a negative row range, then the NULL set: each call below is
    wrong in every later way too."""
    N = pkg._native
    lib = N.load_instance_pairs()
    dev, cnt = lib.shray_instance_pairs_intersect_device, lib.shray_instance_pairs_intersect_counters
    odd = C.c_void_p(20)
    assert dev(None, None, odd, None, None) == -1 and "pairs params are NULL" in last_error(pkg)
    assert dev(None, C.byref(params(pkg, -1, -1, flags=N.PAIRS_ANY, size=8)), odd, None, None) == -1 and "struct_size is 8" in last_error(pkg)
    assert dev(None, C.byref(params(pkg, -1, -1, flags=N.PAIRS_ANY | 8)), odd, None, None) == -1 and "flags 0x9" in last_error(pkg)
    assert dev(None, C.byref(params(pkg, -1, -1, flags=N.PAIRS_ANY)), odd, None, None) == -1 and "SHRAY_PAIRS_ANY needs" in last_error(pkg)
    assert dev(None, C.byref(params(pkg, -1, -1, flags=N.PAIRS_ANY)), None, None, None) == -1 and "SHRAY_PAIRS_ANY needs" in last_error(pkg)
    assert dev(None, C.byref(params(pkg, -1, 1)), None, None, None) == -1 and "negative first row -1" in last_error(pkg)
    assert dev(None, C.byref(params(pkg, 0, -4)), None, None, None) == -1 and "row count -4" in last_error(pkg)
    assert dev(None, C.byref(params(pkg, 0, 1 << 30)), None, None, None) == -1 and "set is NULL" in last_error(pkg)
    assert cnt(None, None, None, None, None) == -1 and "counters is NULL" in last_error(pkg)
