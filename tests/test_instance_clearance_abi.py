"""include/shader_ray_instance_clearance.h against libshray_instance_clearance.so and the ctypes mirror: exactly the declared
functions are exported and bound, the header compiles as C, the library is a client of libshray_hip.so and libshray_instance.so
and of none of libshray_clearance.so, libshray_instance_point.so and libshray_instance_intersect.so, the Python wrappers exist,
and every argument refusal that needs no device returns SHRAY_ERR_INVALID_ARGUMENT before any set or device is touched:
include/shader_ray_clearance.h's params check first (the misuse of SHRAY_CLEARANCE_ANY included), in the instance form a negative
first, then point/first_k_query.h's order, then the alignments.  SHRAY_CLEARANCE_SKIP_OWN_INSTANCE is an unknown flag to the item
forms and to libshray_clearance.so.  (The refusals that read the set -- an instance outside it, a range beyond its scene's
triangles -- are in tests/test_gpu_instance_clearance.py.)"""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "shader_ray_instance_clearance.h")
FUNCTIONS = {"shray_clearance_triangles_instances_device", "shray_clearance_triangles_instances",
             "shray_clearance_triangles_instances_counters", "shray_clearance_instance_device", "shray_clearance_instance"}


def declared():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return set(re.findall(r"^\s*(?:int|void)\s+\**(shray_\w+)\s*\(", text, flags=re.M))


def test_header_symbols_are_exactly_the_exported_and_bound_ones(pkg):
    names = declared()
    assert names == FUNCTIONS
    assert names == {n for n, _, _ in pkg._native.INSTANCE_CLEARANCE_SYMBOLS}
    lib = pkg._native.load_instance_clearance()
    out = subprocess.run(["nm", "-D", "--defined-only", pkg._native.INSTANCE_CLEARANCE_LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\b[TW] (shrayi?_\w+)", out))
    assert exported == names, exported ^ names
    for n in names:
        assert getattr(lib, n).argtypes is not None


def test_the_library_needs_two_libraries_and_not_the_three_it_restates(pkg):
    needed = subprocess.run(["readelf", "-d", pkg._native.INSTANCE_CLEARANCE_LIB], capture_output=True, text=True, check=True).stdout
    assert "libshray_instance.so" in needed and "libshray_hip.so" in needed
    for other in ("libshray_clearance.so", "libshray_instance_point.so", "libshray_instance_intersect.so"):
        assert other not in needed, other


def test_the_header_compiles_as_c(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include "shader_ray_instance_clearance.h"\nint main(void) {\n'
                   '    int (*f)(shray_instance_set *, const shray_clearance_params *, const shray_triangle *, int64_t, shray_pair_distance *,\n'
                   '             int32_t *, int32_t *, void *) = shray_clearance_triangles_instances_device;\n'
                   '    int (*g)(shray_instance_set *, const shray_clearance_params *, int32_t, int64_t, int64_t, shray_pair_distance *,\n'
                   '             int32_t *, int32_t *, void *) = shray_clearance_instance_device;\n'
                   '    (void)f;\n    (void)g;\n'
                   '    printf("%zu %zu %zu %d %d %d %d %d %d\\n", sizeof(shray_triangle), sizeof(shray_clearance_params),\n'
                   '           sizeof(shray_pair_distance), (int)SHRAY_CLEARANCE_MAX, (int)SHRAY_CLEARANCE_ANY, (int)SHRAY_CLEARANCE_SKIP_SHARED,\n'
                   '           (int)SHRAY_CLEARANCE_SKIP_OWN_INSTANCE, (int)SHRAY_PAIR_INTERSECTING, (int)SHRAY_POINT_MAX_HEIGHT);\n    return 0;\n}\n')
    # the declarations match these pointer types (compiled only: the probe that runs is linked against nothing)
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "probe.o")],
                   check=True)
    src.write_text(src.read_text().replace(" = shray_clearance_triangles_instances_device", " = 0")
                   .replace(" = shray_clearance_instance_device", " = 0"))
    exe = tmp_path / "probe"
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split() == ["48", "16", "48", "64", "1", "2", "4", "15",
                                                                                                    "128"]


def test_the_python_wrappers_are_bound(pkg):
    S = pkg.tracer.InstanceSet
    names = lambda f: list(inspect.signature(f).parameters)
    assert names(S.triangle_distances) == ["self", "triangles", "max_dist2", "max_pairs", "counts", "counters", "skip_shared", "any_only"]
    assert names(S.triangle_distances_into) == ["self", "triangles_ptr", "count", "out_ptr", "instances_ptr", "counts_ptr", "max_dist2",
                                                "max_pairs", "any_only", "skip_shared", "stream_ptr"]
    assert names(S.clearance_counts) == ["self", "triangles", "max_dist2", "skip_shared"]
    assert names(S.within_tolerance) == ["self", "triangles", "max_dist2", "skip_shared"]
    assert names(S.instance_clearance) == ["self", "instance", "max_dist2", "max_pairs", "skip_shared", "skip_own", "first", "count", "counts",
                                           "any_only", "device"]
    assert names(S.instance_clearance_into) == ["self", "instance", "first", "count", "out_ptr", "instances_ptr", "counts_ptr", "max_dist2",
                                                "max_pairs", "any_only", "skip_shared", "skip_own", "stream_ptr"]
    assert names(S.instances_within) == ["self", "max_dist2"]
    assert names(S.instance_distance)[:2] == ["self", "instance"]
    p = inspect.signature(S.triangle_distances).parameters
    assert p["max_dist2"].default == float("inf") and p["max_pairs"].default == 1 and p["counts"].default is True
    assert p["counters"].default is False and p["skip_shared"].default is False and p["any_only"].default is False
    p = inspect.signature(S.instance_clearance).parameters
    assert p["max_dist2"].default == float("inf") and p["max_pairs"].default == 1 and p["skip_shared"].default is False
    assert p["skip_own"].default is True and p["first"].default == 0 and p["count"].default is None and p["device"].default is False
    assert callable(pkg._native.load_instance_clearance) and pkg._native.CLEARANCE_SKIP_OWN_INSTANCE == 4
    assert os.path.basename(pkg._native.INSTANCE_CLEARANCE_LIB) == "libshray_instance_clearance.so"
    op = pkg.tracer._set_clearance_params(5, 0.25, False, True, True)
    assert (op.struct_size, op.max_pairs, op.flags, op.max_dist2) == (16, 5, 6, 0.25)
    assert pkg.tracer._set_clearance_params(0, any_only=True).flags == 1
    assert "load_instance_clearance" in open(os.path.join(ROOT, "__graft_entry__.py")).read()


def params(pkg, k=8, size=None, flags=0, max_dist2=float("inf")):
    op = pkg._native.ClearanceParams()
    op.struct_size = C.sizeof(pkg._native.ClearanceParams) if size is None else size
    op.max_pairs, op.flags, op.max_dist2 = k, flags, max_dist2
    return op


def last_error(pkg):
    return pkg._native.load_hip().shray_last_error().decode()


def test_argument_errors(pkg):
    """Each call below fails with SHRAY_ERR_INVALID_ARGUMENT before it reads the (fake) set; count 0 with valid arguments is a
    no-op of the item forms that needs no set data or device."""
    N = pkg._native
    lib = N.load_instance_clearance()
    host, dev, cnt = (lib.shray_clearance_triangles_instances, lib.shray_clearance_triangles_instances_device,
                      lib.shray_clearance_triangles_instances_counters)
    own, own_dev = lib.shray_clearance_instance, lib.shray_clearance_instance_device
    buf = np.zeros(4096, np.uint8)
    base = (buf.ctypes.data + 15) & ~15
    at = lambda o: C.c_void_p(base + o)
    tr, out, inst, counts = at(0), at(128), at(1024), at(1280)      # two triangles, 16 records, 16 instances, two counts
    c = N.Counters()
    fake = C.c_void_p(1)   # never read
    ANY, SHARED, OWN = N.CLEARANCE_ANY, N.CLEARANCE_SKIP_SHARED, N.CLEARANCE_SKIP_OWN_INSTANCE
    ok, k0, any0 = C.byref(params(pkg)), C.byref(params(pkg, 0)), C.byref(params(pkg, 0, flags=ANY))
    shared = C.byref(params(pkg, flags=SHARED))
    cases = {
        "NULL params": lambda: host(fake, None, tr, 2, out, inst, counts),
        "a wrong struct_size": lambda: host(fake, C.byref(params(pkg, size=12)), tr, 2, out, inst, counts),
        "K below 0": lambda: host(fake, C.byref(params(pkg, -1)), tr, 2, out, inst, counts),
        "K above SHRAY_CLEARANCE_MAX": lambda: host(fake, C.byref(params(pkg, 65)), tr, 2, out, inst, counts),
        "an unknown flag": lambda: host(fake, C.byref(params(pkg, flags=8)), tr, 2, out, inst, counts),
        "SKIP_OWN_INSTANCE in the item form": lambda: host(fake, C.byref(params(pkg, flags=OWN)), tr, 2, out, inst, counts),
        "ANY with K > 0": lambda: host(fake, C.byref(params(pkg, 8, flags=ANY)), tr, 2, out, inst, counts),
        "ANY without counts": lambda: host(fake, any0, tr, 2, None, None, None),
        "negative count": lambda: host(fake, ok, tr, -1, out, inst, counts),
        "NULL set": lambda: host(None, ok, tr, 2, out, inst, counts),
        "NULL triangles": lambda: host(fake, ok, None, 2, out, inst, counts),
        "NULL out with K > 0": lambda: host(fake, shared, tr, 2, None, inst, counts),
        "K = 0 and no counts": lambda: host(fake, k0, tr, 2, None, None, None),
        "misaligned triangles": lambda: host(fake, ok, at(8), 2, out, inst, counts),
        "misaligned out": lambda: host(fake, ok, tr, 2, at(132), inst, counts),
        "misaligned instances": lambda: host(fake, ok, tr, 2, out, at(1026), counts),
        "misaligned counts": lambda: host(fake, ok, tr, 2, out, inst, at(1281)),
        "counters, NULL counters": lambda: cnt(fake, ok, tr, 2, out, inst, counts, None),
        "counters, NULL params": lambda: cnt(fake, None, tr, 2, out, inst, counts, C.byref(c)),
        "counters, NULL set": lambda: cnt(None, ok, tr, 2, out, inst, counts, C.byref(c)),
        "counters, negative count": lambda: cnt(fake, ok, tr, -3, out, inst, counts, C.byref(c)),
        "counters, K = 0 and no counts": lambda: cnt(fake, k0, tr, 2, None, None, None, C.byref(c)),
        "counters, ANY with K > 0": lambda: cnt(fake, C.byref(params(pkg, 1, flags=ANY)), tr, 2, out, inst, counts, C.byref(c)),
        "counters, SKIP_OWN_INSTANCE": lambda: cnt(fake, C.byref(params(pkg, flags=OWN | SHARED)), tr, 2, out, inst, counts, C.byref(c)),
        "device, NULL params": lambda: dev(fake, None, tr, 1, out, inst, counts, None),
        "device, K above SHRAY_CLEARANCE_MAX": lambda: dev(fake, C.byref(params(pkg, 65)), tr, 1, out, inst, counts, None),
        "device, SKIP_OWN_INSTANCE": lambda: dev(fake, C.byref(params(pkg, flags=OWN)), tr, 1, out, inst, counts, None),
        "device, ANY with K > 0": lambda: dev(fake, C.byref(params(pkg, 8, flags=ANY)), tr, 1, out, inst, counts, None),
        "device, ANY without counts": lambda: dev(fake, any0, tr, 1, None, None, None, None),
        "device, NULL set": lambda: dev(None, ok, tr, 1, out, inst, counts, None),
        "device, NULL triangles": lambda: dev(fake, ok, None, 1, out, inst, counts, None),
        "device, NULL out with K > 0": lambda: dev(fake, ok, tr, 1, None, inst, counts, None),
        "device, K = 0 and no counts": lambda: dev(fake, k0, tr, 1, None, None, None, None),
        "device, negative count": lambda: dev(fake, ok, tr, -1, out, inst, counts, None),
        "device, misaligned triangles": lambda: dev(fake, ok, at(4), 1, out, inst, counts, None),
        "device, misaligned out": lambda: dev(fake, ok, tr, 1, at(136), inst, counts, None),
        "device, misaligned instances": lambda: dev(fake, ok, tr, 1, out, at(1026), counts, None),
        "device, misaligned counts": lambda: dev(fake, ok, tr, 1, out, inst, at(1281), None),
        "device, misaligned counts, count 0": lambda: dev(fake, ok, tr, 0, out, inst, at(1282), None),
        # the instance form: what it refuses before it reads the set
        "instance form, NULL params": lambda: own(fake, None, 0, 0, 2, out, inst, counts),
        "instance form, an unknown flag": lambda: own(fake, C.byref(params(pkg, flags=8 | OWN)), 0, 0, 2, out, inst, counts),
        "instance form, K above SHRAY_CLEARANCE_MAX": lambda: own(fake, C.byref(params(pkg, 65, flags=OWN)), 0, 0, 2, out, inst, counts),
        "instance form, ANY with K > 0": lambda: own(fake, C.byref(params(pkg, 8, flags=ANY | OWN)), 0, 0, 2, out, inst, counts),
        "instance form, ANY without counts": lambda: own(fake, C.byref(params(pkg, 0, flags=ANY | OWN)), 0, 0, 2, None, None, None),
        "instance form, negative first": lambda: own(fake, C.byref(params(pkg, flags=OWN)), 0, -1, 2, out, inst, counts),
        "instance form, NULL set": lambda: own(None, ok, 0, 0, 2, out, inst, counts),
        "instance form, NULL set, negative count": lambda: own(None, ok, 0, 0, -2, out, inst, counts),
        "device instance form, negative first": lambda: own_dev(fake, ok, 0, -5, 2, out, inst, counts, None),
        "device instance form, NULL set": lambda: own_dev(None, C.byref(params(pkg, flags=OWN | SHARED)), 0, 0, 2, out, inst, counts, None),
        "device instance form, a wrong struct_size": lambda: own_dev(fake, C.byref(params(pkg, size=20)), 0, 0, 2, out, inst, counts, None),
    }
    for what, call in cases.items():
        assert call() == -1, what
        assert last_error(pkg), what
    assert host(fake, ok, tr, 0, out, inst, counts) == 0
    assert host(fake, ok, tr, 0, out, None, None) == 0
    assert host(fake, k0, tr, 0, None, None, counts) == 0
    assert host(fake, any0, tr, 0, None, None, counts) == 0
    assert host(fake, C.byref(params(pkg, flags=SHARED)), tr, 0, out, None, None) == 0
    assert host(fake, C.byref(params(pkg, max_dist2=float("nan"))), tr, 0, out, None, None) == 0    # max_dist2 is never refused
    assert dev(fake, ok, tr, 0, out, None, None, None) == 0
    assert dev(fake, ok, tr, 0, at(144), at(1028), at(1284), None) == 0      # 16 bytes for the records, 4 for the rest
    assert dev(fake, k0, tr, 0, at(132), None, at(1284), None) == 0          # K = 0: the record pointer is not looked at
    c.samples = 99
    c.node_visits = 5
    assert cnt(fake, ok, tr, 0, out, None, None, C.byref(c)) == 0
    assert c.as_dict() == dict.fromkeys(c.as_dict(), 0)


def test_the_refusals_come_in_order(pkg):
    """Params first, the misuse of SHRAY_CLEARANCE_ANY with them; in the instance form a negative first next; then
    point/first_k_query.h's order: the count, the set and triangles, the records, nothing asked for; the alignments after them."""
    N = pkg._native
    lib = N.load_instance_clearance()
    dev, own = lib.shray_clearance_triangles_instances_device, lib.shray_clearance_instance_device
    bad = C.byref(params(pkg, 65))
    any8 = C.byref(params(pkg, 8, flags=N.CLEARANCE_ANY))
    any0 = C.byref(params(pkg, 0, flags=N.CLEARANCE_ANY))
    ok, k0 = C.byref(params(pkg)), C.byref(params(pkg, 0))
    odd = C.c_void_p(20)
    assert dev(None, bad, None, -1, None, None, None, None) == -1 and "clearance params" in last_error(pkg)
    assert dev(None, C.byref(params(pkg, flags=4)), None, -1, None, None, None, None) == -1 and "flags 0x4" in last_error(pkg)
    assert dev(None, any8, None, -1, None, None, None, None) == -1 and "SHRAY_CLEARANCE_ANY needs" in last_error(pkg)
    assert dev(None, any0, None, -1, None, None, None, None) == -1 and "SHRAY_CLEARANCE_ANY needs" in last_error(pkg)
    assert dev(None, any0, None, -1, None, None, C.c_void_p(64), None) == -1 and "negative triangle count" in last_error(pkg)
    assert dev(None, ok, None, -1, None, None, None, None) == -1 and "negative triangle count" in last_error(pkg)
    assert dev(None, ok, None, 1, None, None, None, None) == -1 and "set or triangles is NULL" in last_error(pkg)
    assert dev(C.c_void_p(1), ok, odd, 1, None, None, None, None) == -1 and "out is NULL with max_pairs 8" in last_error(pkg)
    assert dev(C.c_void_p(1), k0, odd, 1, None, None, None, None) == -1 and "nothing is asked for" in last_error(pkg)
    assert dev(C.c_void_p(1), k0, odd, 1, None, None, C.c_void_p(64), None) == -1 and "aligned" in last_error(pkg)
    # the instance form
    assert own(None, bad, 0, -1, -1, None, None, None, None) == -1 and "clearance params" in last_error(pkg)
    assert own(None, any8, 0, -1, -1, None, None, None, None) == -1 and "SHRAY_CLEARANCE_ANY needs" in last_error(pkg)
    assert own(None, ok, 0, -1, -1, None, None, None, None) == -1 and "negative first triangle" in last_error(pkg)
    assert own(None, ok, 0, 0, -1, None, None, None, None) == -1 and "negative triangle count" in last_error(pkg)
    assert own(None, ok, 0, 0, 1, None, None, None, None) == -1 and "set or triangles is NULL" in last_error(pkg)
    assert own(None, C.byref(params(pkg, flags=4)), 0, 0, -1, None, None, None, None) == -1 and "negative triangle count" in last_error(pkg)


def test_the_plain_library_refuses_the_new_flag(pkg):
    """libshray_clearance.so does not change: bit 4 is an unknown flag to all of its forms, refused before the scene is read"""
    N = pkg._native
    lib = N.load_clearance()
    buf = np.zeros(512, np.uint8)
    base = (buf.ctypes.data + 15) & ~15
    op = N.ClearanceParams()
    lib.shray_clearance_params_init(C.byref(op))
    op.flags = N.CLEARANCE_SKIP_OWN_INSTANCE
    fake = C.c_void_p(1)
    assert lib.shray_clearance_triangles(fake, C.byref(op), C.c_void_p(base), 1, C.c_void_p(base + 64), C.c_void_p(base + 128)) == -1
    assert "flags 0x4" in last_error(pkg)
    assert lib.shray_clearance_self(fake, C.byref(op), 0, 1, C.c_void_p(base + 64), C.c_void_p(base + 128)) == -1
    assert "flags 0x4" in last_error(pkg)
    assert lib.shray_clearance_triangles_device(fake, C.byref(op), C.c_void_p(base), 1, C.c_void_p(base + 64), None, None) == -1
    op.flags = N.CLEARANCE_SKIP_OWN_INSTANCE | N.CLEARANCE_SKIP_SHARED
    assert lib.shray_clearance_self_device(fake, C.byref(op), 0, 1, C.c_void_p(base + 64), None, None) == -1 and "flags 0x6" in last_error(pkg)
