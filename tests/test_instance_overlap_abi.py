"""include/shader_ray_instance_overlap.h against libshray_instance_overlap.so and the ctypes mirror: exactly the declared
functions are exported and bound, the header compiles as C, the library is a client of libshray_hip.so and libshray_instance.so
and of neither libshray_overlap.so nor libshray_instance_point.so, the Python wrappers exist, and every argument refusal the
header lists returns SHRAY_ERR_INVALID_ARGUMENT before any set or device is touched: include/shader_ray_overlap.h's params check
first (the misuse of SHRAY_OVERLAP_ANY included), then point/first_k_query.h's order, then the alignments."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "shader_ray_instance_overlap.h")
FUNCTIONS = {"shray_overlap_triangles_instances_device", "shray_overlap_triangles_instances",
             "shray_overlap_triangles_instances_counters"}


def declared():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return set(re.findall(r"^\s*(?:int|void)\s+\**(shray_\w+)\s*\(", text, flags=re.M))


def test_header_symbols_are_exactly_the_exported_and_bound_ones(pkg):
    names = declared()
    assert names == FUNCTIONS
    assert names == {n for n, _, _ in pkg._native.INSTANCE_OVERLAP_SYMBOLS}
    lib = pkg._native.load_instance_overlap()
    out = subprocess.run(["nm", "-D", "--defined-only", pkg._native.INSTANCE_OVERLAP_LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\b[TW] (shrayi?_\w+)", out))
    assert exported == names, exported ^ names
    for n in names:
        assert getattr(lib, n).argtypes is not None


def test_the_library_needs_two_libraries_and_not_the_two_it_restates(pkg):
    needed = subprocess.run(["readelf", "-d", pkg._native.INSTANCE_OVERLAP_LIB], capture_output=True, text=True, check=True).stdout
    assert "libshray_instance.so" in needed and "libshray_hip.so" in needed
    assert "libshray_overlap.so" not in needed and "libshray_instance_point.so" not in needed


def test_the_header_compiles_as_c(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include "shader_ray_instance_overlap.h"\nint main(void) {\n'
                   '    int (*f)(shray_instance_set *, const shray_overlap_params *, const shray_box *, int64_t, int32_t *, int32_t *,\n'
                   '             int32_t *, void *) = 0;\n'
                   '    (void)f;\n'
                   '    printf("%zu %zu %d %d %d\\n", sizeof(shray_box), sizeof(shray_overlap_params), (int)SHRAY_OVERLAP_MAX,\n'
                   '           (int)SHRAY_OVERLAP_ANY, (int)SHRAY_POINT_MAX_HEIGHT);\n    return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split() == ["32", "16", "64", "1", "128"]


def test_the_python_wrappers_are_bound(pkg):
    S = pkg.tracer.InstanceSet
    assert list(inspect.signature(S.triangles_in_boxes).parameters) == ["self", "boxes", "max_triangles", "counts", "counters", "any_only"]
    assert list(inspect.signature(S.triangles_in_boxes_into).parameters) == ["self", "boxes_ptr", "count", "out_ptr", "instances_ptr",
                                                                            "counts_ptr", "max_triangles", "any_only", "stream_ptr"]
    assert list(inspect.signature(S.box_counts).parameters) == ["self", "boxes"]
    assert list(inspect.signature(S.boxes_touched).parameters) == ["self", "boxes"]
    assert list(inspect.signature(S.surface_voxels).parameters) == ["self", "origin", "cell", "dims", "device"]
    p = inspect.signature(S.triangles_in_boxes).parameters
    assert p["max_triangles"].default == 8 and p["counts"].default is True and p["counters"].default is False and p["any_only"].default is False
    assert callable(pkg._native.load_instance_overlap)
    assert os.path.basename(pkg._native.INSTANCE_OVERLAP_LIB) == "libshray_instance_overlap.so"


def params(pkg, k=8, size=None, flags=0, reserved=0):
    op = pkg._native.OverlapParams()
    op.struct_size = C.sizeof(pkg._native.OverlapParams) if size is None else size
    op.max_triangles, op.flags, op.reserved = k, flags, reserved
    return op


def last_error(pkg):
    return pkg._native.load_hip().shray_last_error().decode()


def test_argument_errors(pkg):
    """Each call below fails with SHRAY_ERR_INVALID_ARGUMENT before it reads the (fake) set; count 0 with valid arguments is a
    no-op that needs no set data or device."""
    N = pkg._native
    lib = N.load_instance_overlap()
    host, dev, cnt = (lib.shray_overlap_triangles_instances, lib.shray_overlap_triangles_instances_device,
                      lib.shray_overlap_triangles_instances_counters)
    buf = np.zeros(1024, np.uint8)
    base = (buf.ctypes.data + 15) & ~15
    at = lambda o: C.c_void_p(base + o)
    bx, out, inst, counts = at(0), at(64), at(256), at(512)      # two boxes, 16 indices, 16 instances, two counts
    c = N.Counters()
    fake = C.c_void_p(1)   # never read
    ANY = N.OVERLAP_ANY
    ok, k0, any0 = C.byref(params(pkg)), C.byref(params(pkg, 0)), C.byref(params(pkg, 0, flags=ANY))
    cases = {
        "NULL params": lambda: host(fake, None, bx, 2, out, inst, counts),
        "a wrong struct_size": lambda: host(fake, C.byref(params(pkg, size=12)), bx, 2, out, inst, counts),
        "K below 0": lambda: host(fake, C.byref(params(pkg, -1)), bx, 2, out, inst, counts),
        "K above SHRAY_OVERLAP_MAX": lambda: host(fake, C.byref(params(pkg, 65)), bx, 2, out, inst, counts),
        "an unknown flag": lambda: host(fake, C.byref(params(pkg, flags=2)), bx, 2, out, inst, counts),
        "the reserved field set": lambda: host(fake, C.byref(params(pkg, reserved=1)), bx, 2, out, inst, counts),
        "ANY with K > 0": lambda: host(fake, C.byref(params(pkg, 8, flags=ANY)), bx, 2, out, inst, counts),
        "ANY without counts": lambda: host(fake, any0, bx, 2, None, None, None),
        "negative count": lambda: host(fake, ok, bx, -1, out, inst, counts),
        "NULL set": lambda: host(None, ok, bx, 2, out, inst, counts),
        "NULL boxes": lambda: host(fake, ok, None, 2, out, inst, counts),
        "NULL out with K > 0": lambda: host(fake, ok, bx, 2, None, inst, counts),
        "K = 0 and no counts": lambda: host(fake, k0, bx, 2, None, None, None),
        "misaligned boxes": lambda: host(fake, ok, at(8), 2, out, inst, counts),
        "misaligned out": lambda: host(fake, ok, bx, 2, at(66), inst, counts),
        "misaligned instances": lambda: host(fake, ok, bx, 2, out, at(258), counts),
        "misaligned counts": lambda: host(fake, ok, bx, 2, out, inst, at(513)),
        "counters, NULL counters": lambda: cnt(fake, ok, bx, 2, out, inst, counts, None),
        "counters, NULL params": lambda: cnt(fake, None, bx, 2, out, inst, counts, C.byref(c)),
        "counters, NULL set": lambda: cnt(None, ok, bx, 2, out, inst, counts, C.byref(c)),
        "counters, negative count": lambda: cnt(fake, ok, bx, -3, out, inst, counts, C.byref(c)),
        "counters, K = 0 and no counts": lambda: cnt(fake, k0, bx, 2, None, None, None, C.byref(c)),
        "counters, ANY with K > 0": lambda: cnt(fake, C.byref(params(pkg, 1, flags=ANY)), bx, 2, out, inst, counts, C.byref(c)),
        "device, NULL params": lambda: dev(fake, None, bx, 1, out, inst, counts, None),
        "device, K above SHRAY_OVERLAP_MAX": lambda: dev(fake, C.byref(params(pkg, 65)), bx, 1, out, inst, counts, None),
        "device, ANY with K > 0": lambda: dev(fake, C.byref(params(pkg, 8, flags=ANY)), bx, 1, out, inst, counts, None),
        "device, ANY without counts": lambda: dev(fake, any0, bx, 1, None, None, None, None),
        "device, NULL set": lambda: dev(None, ok, bx, 1, out, inst, counts, None),
        "device, NULL boxes": lambda: dev(fake, ok, None, 1, out, inst, counts, None),
        "device, NULL out with K > 0": lambda: dev(fake, ok, bx, 1, None, inst, counts, None),
        "device, K = 0 and no counts": lambda: dev(fake, k0, bx, 1, None, None, None, None),
        "device, negative count": lambda: dev(fake, ok, bx, -1, out, inst, counts, None),
        "device, misaligned boxes": lambda: dev(fake, ok, at(4), 1, out, inst, counts, None),
        "device, misaligned out": lambda: dev(fake, ok, bx, 1, at(65), inst, counts, None),
        "device, misaligned instances": lambda: dev(fake, ok, bx, 1, out, at(258), counts, None),
        "device, misaligned counts": lambda: dev(fake, ok, bx, 1, out, inst, at(513), None),
        "device, misaligned counts, count 0": lambda: dev(fake, ok, bx, 0, out, inst, at(514), None),
    }
    for what, call in cases.items():
        assert call() == -1, what
        assert last_error(pkg), what
    assert host(fake, ok, bx, 0, out, inst, counts) == 0
    assert host(fake, ok, bx, 0, out, None, None) == 0
    assert host(fake, k0, bx, 0, None, None, counts) == 0
    assert host(fake, any0, bx, 0, None, None, counts) == 0
    assert dev(fake, ok, bx, 0, out, None, None, None) == 0
    assert dev(fake, ok, bx, 0, at(68), at(260), at(516), None) == 0      # 4-byte alignment is enough
    c.samples = 99
    c.node_visits = 5
    assert cnt(fake, ok, bx, 0, out, None, None, C.byref(c)) == 0
    assert c.as_dict() == dict.fromkeys(c.as_dict(), 0)


def test_the_refusals_come_in_order(pkg):
    """Params first, the misuse of SHRAY_OVERLAP_ANY with them; then point/first_k_query.h's order: the count, the set and
    boxes, the indices, nothing asked for; the alignments after them."""
    N = pkg._native
    dev = N.load_instance_overlap().shray_overlap_triangles_instances_device
    bad = C.byref(params(pkg, 65))
    any8 = C.byref(params(pkg, 8, flags=N.OVERLAP_ANY))
    any0 = C.byref(params(pkg, 0, flags=N.OVERLAP_ANY))
    ok, k0 = C.byref(params(pkg)), C.byref(params(pkg, 0))
    odd = C.c_void_p(20)
    assert dev(None, bad, None, -1, None, None, None, None) == -1 and "overlap params" in last_error(pkg)
    assert dev(None, any8, None, -1, None, None, None, None) == -1 and "SHRAY_OVERLAP_ANY needs" in last_error(pkg)
    assert dev(None, any0, None, -1, None, None, None, None) == -1 and "SHRAY_OVERLAP_ANY needs" in last_error(pkg)
    assert dev(None, any0, None, -1, None, None, C.c_void_p(64), None) == -1 and "negative box count" in last_error(pkg)
    assert dev(None, ok, None, -1, None, None, None, None) == -1 and "negative box count" in last_error(pkg)
    assert dev(None, ok, None, 1, None, None, None, None) == -1 and "set or boxes is NULL" in last_error(pkg)
    assert dev(C.c_void_p(1), ok, odd, 1, None, None, None, None) == -1 and "out is NULL with max_triangles 8" in last_error(pkg)
    assert dev(C.c_void_p(1), k0, odd, 1, None, None, None, None) == -1 and "nothing is asked for" in last_error(pkg)
    assert dev(C.c_void_p(1), k0, odd, 1, None, None, C.c_void_p(64), None) == -1 and "aligned" in last_error(pkg)
