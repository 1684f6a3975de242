"""include/shader_ray_clearance.h against libshray_clearance.so and the ctypes mirror: exactly the declared functions are
exported and bound, shray_pair_distance and shray_clearance_params have the header's layout, the constants are the mirror's,
shray_clearance_params_init sets the header's defaults, and every argument refusal the header lists returns
SHRAY_ERR_INVALID_ARGUMENT before any scene or device is touched."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "shader_ray_clearance.h")
FUNCTIONS = {"shray_clearance_params_init", "shray_clearance_triangles_device", "shray_clearance_triangles",
             "shray_clearance_triangles_counters", "shray_clearance_self_device", "shray_clearance_self"}


def declared():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return set(re.findall(r"^\s*(?:int|void)\s+\**(shray_\w+)\s*\(", text, flags=re.M))


def test_header_symbols_are_exactly_the_exported_and_bound_ones(pkg):
    names = declared()
    assert names == FUNCTIONS
    assert names == {n for n, _, _ in pkg._native.CLEARANCE_SYMBOLS}
    lib = pkg._native.load_clearance()
    out = subprocess.run(["nm", "-D", "--defined-only", pkg._native.CLEARANCE_LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\b[TW] (shrayi?_\w+)", out))
    assert exported == names, exported ^ names
    for n in names:
        assert getattr(lib, n).argtypes is not None


def test_layouts_and_constants_match_the_header(pkg, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "shader_ray_clearance.h"\nint main(void) {\n'
                   '    printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %d %d\\n", sizeof(shray_pair_distance),\n'
                   '           offsetof(shray_pair_distance, on_query), offsetof(shray_pair_distance, dist2),\n'
                   '           offsetof(shray_pair_distance, on_scene), offsetof(shray_pair_distance, triangle),\n'
                   '           offsetof(shray_pair_distance, feature), offsetof(shray_pair_distance, reserved),\n'
                   '           sizeof(shray_clearance_params), offsetof(shray_clearance_params, struct_size),\n'
                   '           offsetof(shray_clearance_params, max_pairs), offsetof(shray_clearance_params, flags),\n'
                   '           offsetof(shray_clearance_params, max_dist2), (int)SHRAY_CLEARANCE_MAX, (int)SHRAY_CLEARANCE_ANY,\n'
                   '           (int)SHRAY_CLEARANCE_SKIP_SHARED, (int)SHRAY_PAIR_INTERSECTING);\n'
                   '    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    N, T = pkg._native, pkg.tracer
    R, P = N.PairDistance, N.ClearanceParams
    assert got == [C.sizeof(R), R.on_query.offset, R.dist2.offset, R.on_scene.offset, R.triangle.offset, R.feature.offset, R.reserved.offset,
                   C.sizeof(P), P.struct_size.offset, P.max_pairs.offset, P.flags.offset, P.max_dist2.offset, N.CLEARANCE_MAX,
                   N.CLEARANCE_ANY, N.CLEARANCE_SKIP_SHARED, N.PAIR_INTERSECTING]
    assert got == [48, 0, 12, 16, 28, 32, 36, 16, 0, 4, 8, 12, 64, 1, 2, 15]
    D = T.PAIR_DISTANCE_DTYPE
    assert D.itemsize == 48
    assert [D.fields[f][1] for f in ("on_query", "dist2", "on_scene", "triangle", "feature", "reserved")] == [0, 12, 16, 28, 32, 36]
    import clearance_ref
    assert clearance_ref.PAIR_DISTANCE_DTYPE == D and clearance_ref.PAIR_INTERSECTING == N.PAIR_INTERSECTING


def test_params_init_defaults(pkg):
    N, T = pkg._native, pkg.tracer
    op = N.ClearanceParams()
    op.struct_size, op.max_pairs, op.flags, op.max_dist2 = 9, 9, 9, 9.0
    N.load_clearance().shray_clearance_params_init(C.byref(op))
    assert (op.struct_size, op.max_pairs, op.flags) == (16, 1, 0) and op.max_dist2 == math.inf
    N.load_clearance().shray_clearance_params_init(None)   # a no-op
    d = T.clearance_params()
    assert (d.struct_size, d.max_pairs, d.flags, d.max_dist2) == (16, 1, 0, math.inf)
    assert T.clearance_params(5, 0.25).max_pairs == 5 and T.clearance_params(5, 0.25).max_dist2 == 0.25
    assert [T.clearance_params(0, 1.0, a, s).flags for a, s in ((False, False), (True, False), (False, True), (True, True))] == [0, 1, 2, 3]
    assert math.isnan(T.clearance_params(1, math.nan).max_dist2) and T.clearance_params(1, -1.0).max_dist2 == -1.0


def forms(N):
    """name -> call(scene, params, triangles, count, out, counts): the item forms"""
    lib = N.load_clearance()
    tallies = N.Counters()
    return {"host": lambda s, p, t, n, o, c: lib.shray_clearance_triangles(s, p, t, n, o, c),
            "device": lambda s, p, t, n, o, c: lib.shray_clearance_triangles_device(s, p, t, n, o, c, None),
            "counters": lambda s, p, t, n, o, c: lib.shray_clearance_triangles_counters(s, p, t, n, o, c, C.byref(tallies))}


def test_argument_errors(pkg):
    """Each call below fails with SHRAY_ERR_INVALID_ARGUMENT before it reads the (fake) scene; count 0 with valid arguments
    is a no-op that needs no scene data or device."""
    N = pkg._native
    lib = N.load_clearance()
    buf = np.zeros(4096, np.uint8)
    base = (buf.ctypes.data + 15) & ~15
    tris, out, counts = C.c_void_p(base), C.c_void_p(base + 96), C.c_void_p(base + 2048)
    fake = C.c_void_p(1)   # never read
    ANY, SKIP = N.CLEARANCE_ANY, N.CLEARANCE_SKIP_SHARED

    def params(k=8, flags=0, struct_size=16, max_dist2=1.0):
        op = N.ClearanceParams()
        op.struct_size, op.max_pairs, op.flags, op.max_dist2 = struct_size, k, flags, max_dist2
        return C.byref(op)

    self_forms = {"self": lambda s, p, first, n, o, c: lib.shray_clearance_self(s, p, first, n, o, c),
                  "self device": lambda s, p, first, n, o, c: lib.shray_clearance_self_device(s, p, first, n, o, c, None)}
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
            f"{name}, struct_size 12": lambda call=call, items=items: call(fake, params(struct_size=12), items, 2, out, counts),
            f"{name}, struct_size 20": lambda call=call, items=items: call(fake, params(struct_size=20), items, 2, out, counts),
            f"{name}, ANY with K > 0": lambda call=call, items=items: call(fake, params(8, ANY), items, 2, out, counts),
            f"{name}, ANY | SKIP_SHARED with K > 0": lambda call=call, items=items: call(fake, params(1, ANY | SKIP), items, 2, out, counts),
            f"{name}, ANY without counts": lambda call=call, items=items: call(fake, params(0, ANY), items, 2, None, None),
            f"{name}, misaligned records by 4": lambda call=call, items=items: call(fake, params(), items, 2, C.c_void_p(base + 100), counts),
            f"{name}, misaligned records by 8": lambda call=call, items=items: call(fake, params(), items, 2, C.c_void_p(base + 104), counts),
            f"{name}, misaligned counts": lambda call=call, items=items: call(fake, params(), items, 2, out, C.c_void_p(base + 2049)),
            f"{name}, misaligned counts, K == 0": lambda call=call, items=items: call(fake, params(0), items, 2, None, C.c_void_p(base + 2050)),
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
    cases["counters, NULL counters"] = lambda: lib.shray_clearance_triangles_counters(fake, params(), tris, 2, out, counts, None)
    for what, call in cases.items():
        assert call() == -1, what
        assert N.load_hip().shray_last_error(), what
    host, dev, cnt = lib.shray_clearance_triangles, lib.shray_clearance_triangles_device, lib.shray_clearance_triangles_counters
    tallies = N.Counters()
    assert host(fake, params(), tris, 0, out, counts) == 0
    assert host(fake, params(0), tris, 0, None, counts) == 0
    assert host(fake, params(0, ANY | SKIP), tris, 0, None, counts) == 0
    assert host(fake, params(64, SKIP), tris, 0, out, None) == 0
    assert host(fake, params(8, 0, 16, math.nan), tris, 0, out, None) == 0   # (max_dist2 is never refused: NaN and negative are unwalked queries)
    assert host(fake, params(8, 0, 16, -1.0), tris, 0, out, None) == 0
    assert dev(fake, params(), tris, 0, out, None, None) == 0
    assert cnt(fake, params(), tris, 0, out, counts, C.byref(tallies)) == 0 and tallies.samples == 0


def test_refusal_texts(pkg):
    """One refusal of each kind leaves its text in shray_last_error(), in the words of the triangle-intersection library's."""
    N = pkg._native
    lib = N.load_clearance()
    host, cnt, own = lib.shray_clearance_triangles, lib.shray_clearance_triangles_counters, lib.shray_clearance_self
    buf = np.zeros(4096, np.uint8)
    base = (buf.ctypes.data + 15) & ~15
    tris, out, counts = C.c_void_p(base), C.c_void_p(base + 96), C.c_void_p(base + 2048)
    fake = C.c_void_p(1)   # never read

    def params(k=8, flags=0, struct_size=16):
        op = N.ClearanceParams()
        op.struct_size, op.max_pairs, op.flags, op.max_dist2 = struct_size, k, flags, 1.0
        return C.byref(op)

    cases = {
        "negative triangle count -1": lambda: host(fake, params(), tris, -1, out, counts),
        "scene or triangles is NULL": lambda: host(fake, params(), None, 2, out, counts),
        "out is NULL with max_pairs 8": lambda: host(fake, params(), tris, 2, None, counts),
        "nothing is asked for: max_pairs is 0 and counts is NULL": lambda: host(fake, params(0), tris, 2, None, None),
        "clearance params out of range (max_pairs 65 of 0 .. 64, flags 0x0)": lambda: host(fake, params(65), tris, 2, out, counts),
        "clearance params out of range (max_pairs 8 of 0 .. 64, flags 0x4)": lambda: host(fake, params(8, 4), tris, 2, out, counts),
        "shray_clearance_params.struct_size is 12, this library expects 16": lambda: host(fake, params(struct_size=12), tris, 2, out, counts),
        "clearance params are NULL": lambda: host(fake, None, tris, 2, out, counts),
        # the library's own refusals keep their place: after the NULL triangles, before the NULL out
        "SHRAY_CLEARANCE_ANY needs max_pairs 0 (it is 8) and counts": lambda: host(fake, params(8, N.CLEARANCE_ANY), tris, 2, None, counts),
        "negative first triangle -3": lambda: own(fake, params(), -3, 2, None, counts),
        "the triangles and the records must be 16-byte aligned, the counts 4-byte aligned":
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
        return   # a GPU is present: the query runs (tests/test_gpu_clearance.py)
    hand = helpers.single_leaf_scene([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]])
    with pytest.raises(N.ShrayError) as err:
        pkg.Scene(hand.desc).triangle_distances(np.zeros((2, 9), np.float32))
    assert err.value.code in (-2, -3) and str(err.value)
