"""include/shader_ray_intersect.h against libshray_intersect.so and the ctypes mirror: exactly the declared functions are
exported and bound, shray_triangle and shray_intersect_params have the header's layout, the constants are the mirror's, and
every argument refusal the header lists returns SHRAY_ERR_INVALID_ARGUMENT before any scene or device is touched."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "shader_ray_intersect.h")
FUNCTIONS = {"shray_intersect_params_init", "shray_intersect_triangles_device", "shray_intersect_triangles",
             "shray_intersect_triangles_counters", "shray_intersect_self_device", "shray_intersect_self"}


def declared():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return set(re.findall(r"^\s*(?:int|void)\s+\**(shray_\w+)\s*\(", text, flags=re.M))


def test_header_symbols_are_exactly_the_exported_and_bound_ones(pkg):
    names = declared()
    assert names == FUNCTIONS
    assert names == {n for n, _, _ in pkg._native.INTERSECT_SYMBOLS}
    lib = pkg._native.load_intersect()
    out = subprocess.run(["nm", "-D", "--defined-only", pkg._native.INTERSECT_LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\b[TW] (shrayi?_\w+)", out))
    assert exported == names, exported ^ names
    for n in names:
        assert getattr(lib, n).argtypes is not None


def test_layouts_and_constants_match_the_header(pkg, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "shader_ray_intersect.h"\nint main(void) {\n'
                   '    printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %d\\n", sizeof(shray_triangle), offsetof(shray_triangle, a),\n'
                   '           offsetof(shray_triangle, pad0), offsetof(shray_triangle, b), offsetof(shray_triangle, pad1),\n'
                   '           offsetof(shray_triangle, c), offsetof(shray_triangle, pad2), sizeof(shray_intersect_params),\n'
                   '           offsetof(shray_intersect_params, struct_size), offsetof(shray_intersect_params, max_triangles),\n'
                   '           offsetof(shray_intersect_params, flags), offsetof(shray_intersect_params, reserved), (int)SHRAY_INTERSECT_MAX,\n'
                   '           (int)SHRAY_INTERSECT_ANY, (int)SHRAY_INTERSECT_SKIP_SHARED);\n'
                   '    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    N, T = pkg._native, pkg.tracer
    R, P = N.Triangle, N.IntersectParams
    assert got == [C.sizeof(R), R.a.offset, R.pad0.offset, R.b.offset, R.pad1.offset, R.c.offset, R.pad2.offset, C.sizeof(P),
                   P.struct_size.offset, P.max_triangles.offset, P.flags.offset, P.reserved.offset, N.INTERSECT_MAX, N.INTERSECT_ANY,
                   N.INTERSECT_SKIP_SHARED]
    assert got == [48, 0, 12, 16, 28, 32, 44, 16, 0, 4, 8, 12, 64, 1, 2]
    assert T.TRIANGLE_DTYPE.itemsize == 48
    assert [T.TRIANGLE_DTYPE.fields[f][1] for f in ("a", "pad0", "b", "pad1", "c", "pad2")] == [0, 12, 16, 28, 32, 44]
    op = P()
    op.flags, op.reserved = 9, 9
    N.load_intersect().shray_intersect_params_init(C.byref(op))
    assert (op.struct_size, op.max_triangles, op.flags, op.reserved) == (16, 8, 0, 0)
    N.load_intersect().shray_intersect_params_init(None)   # a no-op
    assert T.intersect_params(5).max_triangles == 5 and T.intersect_params().max_triangles == 8
    assert [T.intersect_params(0, a, s).flags for a, s in ((False, False), (True, False), (False, True), (True, True))] == [0, 1, 2, 3]
    want = [0, 1, 2, 0, 3, 4, 5, 0, 6, 7, 8, 0]
    corners = np.arange(9, dtype=np.float32)
    for made in (T.make_triangles(corners.reshape(1, 3, 3)), T.make_triangles(corners.reshape(1, 9)),
                 T.make_triangles([(0, 1, 2)], [(3, 4, 5)], [(6, 7, 8)]), T._host_triangles(corners.reshape(1, 3, 3)),
                 T._host_triangles(corners.reshape(1, 9)), T._host_triangles(np.asarray([want], np.float32))):
        assert made.dtype == T.TRIANGLE_DTYPE and made.view(np.float32).tolist() == want
    with pytest.raises(ValueError):
        T._host_triangles(np.zeros((4, 8), np.float32))


def forms(N):
    """name -> call(scene, params, triangles, count, out, counts): the item forms; the self forms take first = 0 in place of the
    triangles"""
    lib = N.load_intersect()
    tallies = N.Counters()
    return {"host": lambda s, p, t, n, o, c: lib.shray_intersect_triangles(s, p, t, n, o, c),
            "device": lambda s, p, t, n, o, c: lib.shray_intersect_triangles_device(s, p, t, n, o, c, None),
            "counters": lambda s, p, t, n, o, c: lib.shray_intersect_triangles_counters(s, p, t, n, o, c, C.byref(tallies))}


def test_argument_errors(pkg):
    """Each call below fails with SHRAY_ERR_INVALID_ARGUMENT before it reads the (fake) scene; count 0 with valid arguments
    is a no-op that needs no scene data or device."""
    N = pkg._native
    lib = N.load_intersect()
    buf = np.zeros(2048, np.uint8)
    base = (buf.ctypes.data + 15) & ~15
    tris, out, counts = C.c_void_p(base), C.c_void_p(base + 96), C.c_void_p(base + 1024)
    fake = C.c_void_p(1)   # never read
    ANY, SKIP = N.INTERSECT_ANY, N.INTERSECT_SKIP_SHARED

    def params(k=8, flags=0, reserved=0, struct_size=16):
        op = N.IntersectParams()
        op.struct_size, op.max_triangles, op.flags, op.reserved = struct_size, k, flags, reserved
        return C.byref(op)

    self_forms = {"self": lambda s, p, first, n, o, c: lib.shray_intersect_self(s, p, first, n, o, c),
                  "self device": lambda s, p, first, n, o, c: lib.shray_intersect_self_device(s, p, first, n, o, c, None)}
    cases = {}
    for name, call in list(forms(N).items()) + list(self_forms.items()):
        items = 0 if name in self_forms else tris
        cases.update({
            f"{name}, NULL scene": lambda call=call, items=items: call(None, params(), items, 2, out, counts),
            f"{name}, NULL params": lambda call=call, items=items: call(fake, None, items, 2, out, counts),
            f"{name}, NULL out with K > 0": lambda call=call, items=items: call(fake, params(), items, 2, None, counts),
            f"{name}, K == 0 and no counts": lambda call=call, items=items: call(fake, params(0), items, 2, None, None),
            f"{name}, K == 0, out given, no counts": lambda call=call, items=items: call(fake, params(0), items, 2, out, None),
            f"{name}, negative count": lambda call=call, items=items: call(fake, params(), items, -1, out, counts),
            f"{name}, K -1": lambda call=call, items=items: call(fake, params(-1), items, 2, out, counts),
            f"{name}, K 65": lambda call=call, items=items: call(fake, params(65), items, 2, out, counts),
            f"{name}, unknown flag": lambda call=call, items=items: call(fake, params(8, 4), items, 2, out, counts),
            f"{name}, unknown flag beside ANY": lambda call=call, items=items: call(fake, params(0, ANY | 0x80000000), items, 2, None, counts),
            f"{name}, unknown flag beside both": lambda call=call, items=items: call(fake, params(0, ANY | SKIP | 8), items, 2, None, counts),
            f"{name}, reserved": lambda call=call, items=items: call(fake, params(8, 0, 1), items, 2, out, counts),
            f"{name}, struct_size 12": lambda call=call, items=items: call(fake, params(struct_size=12), items, 2, out, counts),
            f"{name}, struct_size 20": lambda call=call, items=items: call(fake, params(struct_size=20), items, 2, out, counts),
            f"{name}, ANY with K > 0": lambda call=call, items=items: call(fake, params(8, ANY), items, 2, out, counts),
            f"{name}, ANY | SKIP_SHARED with K > 0": lambda call=call, items=items: call(fake, params(1, ANY | SKIP), items, 2, out, counts),
            f"{name}, ANY without counts": lambda call=call, items=items: call(fake, params(0, ANY), items, 2, None, None),
            f"{name}, misaligned out": lambda call=call, items=items: call(fake, params(), items, 2, C.c_void_p(base + 98), counts),
            f"{name}, misaligned counts": lambda call=call, items=items: call(fake, params(), items, 2, out, C.c_void_p(base + 1025)),
            f"{name}, misaligned counts, K == 0": lambda call=call, items=items: call(fake, params(0), items, 2, None, C.c_void_p(base + 1026)),
        })
        if name in self_forms:
            cases.update({
                f"{name}, negative first": lambda call=call: call(fake, params(), -1, 2, out, counts),
                f"{name}, negative first, count 0": lambda call=call: call(fake, params(), -5, 0, out, counts),
                f"{name}, negative first and count": lambda call=call: call(fake, params(), -1, -1, out, counts),
            })
        else:
            cases.update({
                f"{name}, NULL triangles": lambda call=call: call(fake, params(), None, 2, out, counts),
                f"{name}, misaligned triangles": lambda call=call: call(fake, params(), C.c_void_p(base + 4), 2, out, counts),
                f"{name}, misaligned triangles by 8": lambda call=call: call(fake, params(), C.c_void_p(base + 8), 2, out, counts),
            })
    cases["counters, NULL counters"] = lambda: lib.shray_intersect_triangles_counters(fake, params(), tris, 2, out, counts, None)
    for what, call in cases.items():
        assert call() == -1, what
        assert N.load_hip().shray_last_error(), what
    host, dev, cnt = lib.shray_intersect_triangles, lib.shray_intersect_triangles_device, lib.shray_intersect_triangles_counters
    tallies = N.Counters()
    assert host(fake, params(), tris, 0, out, counts) == 0
    assert host(fake, params(0), tris, 0, None, counts) == 0
    assert host(fake, params(0, ANY | SKIP), tris, 0, None, counts) == 0
    assert host(fake, params(64, SKIP), tris, 0, out, None) == 0
    assert dev(fake, params(), tris, 0, out, None, None) == 0
    assert cnt(fake, params(), tris, 0, out, counts, C.byref(tallies)) == 0 and tallies.samples == 0


def test_refusal_texts(pkg):
    """One refusal of each kind leaves its text in shray_last_error(), in the words of the box-overlap library's."""
    N = pkg._native
    lib = N.load_intersect()
    host, cnt, own = lib.shray_intersect_triangles, lib.shray_intersect_triangles_counters, lib.shray_intersect_self
    buf = np.zeros(2048, np.uint8)
    base = (buf.ctypes.data + 15) & ~15
    tris, out, counts = C.c_void_p(base), C.c_void_p(base + 96), C.c_void_p(base + 1024)
    fake = C.c_void_p(1)   # never read

    def params(k=8, flags=0, struct_size=16):
        op = N.IntersectParams()
        op.struct_size, op.max_triangles, op.flags, op.reserved = struct_size, k, flags, 0
        return C.byref(op)

    cases = {
        "negative triangle count -1": lambda: host(fake, params(), tris, -1, out, counts),
        "scene or triangles is NULL": lambda: host(fake, params(), None, 2, out, counts),
        "out is NULL with max_triangles 8": lambda: host(fake, params(), tris, 2, None, counts),
        "nothing is asked for: max_triangles is 0 and counts is NULL": lambda: host(fake, params(0), tris, 2, None, None),
        "intersect params out of range (max_triangles 65 of 0 .. 64, flags 0x0, reserved 0)": lambda: host(fake, params(65), tris, 2, out, counts),
        "intersect params out of range (max_triangles 8 of 0 .. 64, flags 0x4, reserved 0)": lambda: host(fake, params(8, 4), tris, 2, out, counts),
        "shray_intersect_params.struct_size is 12, this library expects 16": lambda: host(fake, params(struct_size=12), tris, 2, out, counts),
        "intersect params are NULL": lambda: host(fake, None, tris, 2, out, counts),
        # the library's own refusals keep their place: after the NULL triangles, before the NULL out
        "SHRAY_INTERSECT_ANY needs max_triangles 0 (it is 8) and counts": lambda: host(fake, params(8, N.INTERSECT_ANY), tris, 2, None, counts),
        "negative first triangle -3": lambda: own(fake, params(), -3, 2, None, counts),
        "the triangles must be 16-byte aligned, the indices and the counts 4-byte aligned":
            lambda: host(fake, params(), C.c_void_p(base + 4), 2, out, counts),
        "counters is NULL": lambda: cnt(fake, params(), tris, 2, out, counts, None),
    }
    for text, call in cases.items():
        assert call() == -1, text
        assert N.load_hip().shray_last_error().decode() == text


def test_a_valid_call_fails_loudly_without_a_gpu(pkg):
    """No CPU fallback: where there is no HIP device a valid query on a real scene is an error with a message, never an answer
    (the scene it needs cannot be created)."""
    import helpers
    N = pkg._native
    n = C.c_int()
    if N.load_hip().shray_device_count(C.byref(n)) == 0 and n.value > 0:
        pytest.skip("a GPU is present: the query runs (tests/test_gpu_intersect.py)")
    hand = helpers.single_leaf_scene([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]])
    with pytest.raises(N.ShrayError) as err:
        pkg.Scene(hand.desc).intersecting_triangles(np.zeros((2, 9), np.float32))
    assert err.value.code in (-2, -3) and str(err.value)
