"""include/shader_ray_overlap.h against libshray_overlap.so and the ctypes mirror: exactly the declared functions are exported
and bound, shray_box and shray_overlap_params have the header's layout, the constants are the mirror's, and every argument
refusal the header lists returns SHRAY_ERR_INVALID_ARGUMENT before any scene or device is touched."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "shader_ray_overlap.h")
FUNCTIONS = {"shray_overlap_params_init", "shray_overlap_triangles_device", "shray_overlap_triangles", "shray_overlap_triangles_counters"}


def declared():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return set(re.findall(r"^\s*(?:int|void)\s+\**(shray_\w+)\s*\(", text, flags=re.M))


def test_header_symbols_are_exactly_the_exported_and_bound_ones(pkg):
    names = declared()
    assert names == FUNCTIONS
    assert names == {n for n, _, _ in pkg._native.OVERLAP_SYMBOLS}
    lib = pkg._native.load_overlap()
    out = subprocess.run(["nm", "-D", "--defined-only", pkg._native.OVERLAP_LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\b[TW] (shrayi?_\w+)", out))
    assert exported == names, exported ^ names
    for n in names:
        assert getattr(lib, n).argtypes is not None


def test_layouts_and_constants_match_the_header(pkg, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "shader_ray_overlap.h"\nint main(void) {\n'
                   '    printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d\\n", sizeof(shray_box), offsetof(shray_box, lo), offsetof(shray_box, pad0),\n'
                   '           offsetof(shray_box, hi), offsetof(shray_box, pad1), sizeof(shray_overlap_params),\n'
                   '           offsetof(shray_overlap_params, struct_size), offsetof(shray_overlap_params, max_triangles),\n'
                   '           offsetof(shray_overlap_params, flags), offsetof(shray_overlap_params, reserved), (int)SHRAY_OVERLAP_MAX,\n'
                   '           (int)SHRAY_OVERLAP_ANY);\n'
                   '    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    B, P = pkg._native.Box, pkg._native.OverlapParams
    assert got == [C.sizeof(B), B.lo.offset, B.pad0.offset, B.hi.offset, B.pad1.offset, C.sizeof(P), P.struct_size.offset,
                   P.max_triangles.offset, P.flags.offset, P.reserved.offset, pkg._native.OVERLAP_MAX, pkg._native.OVERLAP_ANY]
    assert got == [32, 0, 12, 16, 28, 16, 0, 4, 8, 12, 64, 1]
    assert pkg.tracer.BOX_DTYPE.itemsize == 32 and [pkg.tracer.BOX_DTYPE.fields[f][1] for f in ("lo", "pad0", "hi", "pad1")] == [0, 12, 16, 28]
    op = P()
    op.flags, op.reserved = 9, 9
    pkg._native.load_overlap().shray_overlap_params_init(C.byref(op))
    assert (op.struct_size, op.max_triangles, op.flags, op.reserved) == (16, 8, 0, 0)
    pkg._native.load_overlap().shray_overlap_params_init(None)   # a no-op
    assert pkg.tracer.overlap_params(5).max_triangles == 5 and pkg.tracer.overlap_params().max_triangles == 8
    assert pkg.tracer.overlap_params(0, True).flags == 1
    boxes = pkg.tracer.make_boxes([(0, 1, 2)], [(3, 4, 5)])
    assert boxes.view(np.float32).tolist() == [0, 1, 2, 0, 3, 4, 5, 0]


def test_argument_errors(pkg):
    """Each call below fails with SHRAY_ERR_INVALID_ARGUMENT before it reads the (fake) scene; count 0 with valid arguments
    is a no-op that needs no scene data or device."""
    N = pkg._native
    lib = N.load_overlap()
    host, dev, cnt = lib.shray_overlap_triangles, lib.shray_overlap_triangles_device, lib.shray_overlap_triangles_counters
    buf = np.zeros(1024, np.uint8)
    base = (buf.ctypes.data + 15) & ~15
    boxes, out, counts = C.c_void_p(base), C.c_void_p(base + 64), C.c_void_p(base + 640)
    tallies = N.Counters()
    fake = C.c_void_p(1)   # never read
    ANY = N.OVERLAP_ANY

    def params(k=8, flags=0, reserved=0, struct_size=16):
        op = N.OverlapParams()
        op.struct_size, op.max_triangles, op.flags, op.reserved = struct_size, k, flags, reserved
        return C.byref(op)

    cases = {}
    for name, call in (("host", lambda *a: host(*a)), ("device", lambda *a: dev(*a, None)), ("counters", lambda *a: cnt(*a, C.byref(tallies)))):
        cases.update({
            f"{name}, NULL scene": lambda call=call: call(None, params(), boxes, 2, out, counts),
            f"{name}, NULL params": lambda call=call: call(fake, None, boxes, 2, out, counts),
            f"{name}, NULL boxes": lambda call=call: call(fake, params(), None, 2, out, counts),
            f"{name}, NULL out with K > 0": lambda call=call: call(fake, params(), boxes, 2, None, counts),
            f"{name}, K == 0 and no counts": lambda call=call: call(fake, params(0), boxes, 2, None, None),
            f"{name}, K == 0, out given, no counts": lambda call=call: call(fake, params(0), boxes, 2, out, None),
            f"{name}, negative count": lambda call=call: call(fake, params(), boxes, -1, out, counts),
            f"{name}, K -1": lambda call=call: call(fake, params(-1), boxes, 2, out, counts),
            f"{name}, K 65": lambda call=call: call(fake, params(65), boxes, 2, out, counts),
            f"{name}, unknown flag": lambda call=call: call(fake, params(8, 2), boxes, 2, out, counts),
            f"{name}, unknown flag beside ANY": lambda call=call: call(fake, params(0, ANY | 0x80000000), boxes, 2, None, counts),
            f"{name}, reserved": lambda call=call: call(fake, params(8, 0, 1), boxes, 2, out, counts),
            f"{name}, struct_size 12": lambda call=call: call(fake, params(struct_size=12), boxes, 2, out, counts),
            f"{name}, struct_size 20": lambda call=call: call(fake, params(struct_size=20), boxes, 2, out, counts),
            f"{name}, ANY with K > 0": lambda call=call: call(fake, params(8, ANY), boxes, 2, out, counts),
            f"{name}, ANY without counts": lambda call=call: call(fake, params(0, ANY), boxes, 2, None, None),
            f"{name}, misaligned boxes": lambda call=call: call(fake, params(), C.c_void_p(base + 4), 2, out, counts),
            f"{name}, misaligned boxes by 8": lambda call=call: call(fake, params(), C.c_void_p(base + 8), 2, out, counts),
            f"{name}, misaligned out": lambda call=call: call(fake, params(), boxes, 2, C.c_void_p(base + 66), counts),
            f"{name}, misaligned counts": lambda call=call: call(fake, params(), boxes, 2, out, C.c_void_p(base + 641)),
            f"{name}, misaligned counts, K == 0": lambda call=call: call(fake, params(0), boxes, 2, None, C.c_void_p(base + 642)),
        })
    cases["counters, NULL counters"] = lambda: cnt(fake, params(), boxes, 2, out, counts, None)
    for what, call in cases.items():
        assert call() == -1, what
        assert N.load_hip().shray_last_error(), what
    assert host(fake, params(), boxes, 0, out, counts) == 0
    assert host(fake, params(0), boxes, 0, None, counts) == 0
    assert host(fake, params(0, ANY), boxes, 0, None, counts) == 0
    assert host(fake, params(64), boxes, 0, out, None) == 0
    assert dev(fake, params(), boxes, 0, out, None, None) == 0
    assert cnt(fake, params(), boxes, 0, out, counts, C.byref(tallies)) == 0 and tallies.samples == 0


def test_refusal_texts(pkg):
    """One refusal of each kind leaves in shray_last_error() the text this library has always given for it."""
    N = pkg._native
    lib = N.load_overlap()
    host, cnt = lib.shray_overlap_triangles, lib.shray_overlap_triangles_counters
    buf = np.zeros(1024, np.uint8)
    base = (buf.ctypes.data + 15) & ~15
    boxes, out, counts = C.c_void_p(base), C.c_void_p(base + 64), C.c_void_p(base + 640)
    fake = C.c_void_p(1)   # never read

    def params(k=8, flags=0, struct_size=16):
        op = N.OverlapParams()
        op.struct_size, op.max_triangles, op.flags, op.reserved = struct_size, k, flags, 0
        return C.byref(op)

    cases = {
        "negative box count -1": lambda: host(fake, params(), boxes, -1, out, counts),
        "scene or boxes is NULL": lambda: host(fake, params(), None, 2, out, counts),
        "out is NULL with max_triangles 8": lambda: host(fake, params(), boxes, 2, None, counts),
        "nothing is asked for: max_triangles is 0 and counts is NULL": lambda: host(fake, params(0), boxes, 2, None, None),
        "overlap params out of range (max_triangles 65 of 0 .. 64, flags 0x0, reserved 0)": lambda: host(fake, params(65), boxes, 2, out, counts),
        "shray_overlap_params.struct_size is 12, this library expects 16": lambda: host(fake, params(struct_size=12), boxes, 2, out, counts),
        "overlap params are NULL": lambda: host(fake, None, boxes, 2, out, counts),
        # the library's own refusal keeps its place: after the NULL boxes, before the NULL out
        "SHRAY_OVERLAP_ANY needs max_triangles 0 (it is 8) and counts": lambda: host(fake, params(8, N.OVERLAP_ANY), boxes, 2, None, counts),
        "the boxes must be 16-byte aligned, the indices and the counts 4-byte aligned":
            lambda: host(fake, params(), C.c_void_p(base + 4), 2, out, counts),
        "counters is NULL": lambda: cnt(fake, params(), boxes, 2, out, counts, None),
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
        pytest.skip("a GPU is present: the query runs (tests/test_gpu_overlap.py)")
    hand = helpers.single_leaf_scene([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]])
    with pytest.raises(N.ShrayError) as err:
        pkg.Scene(hand.desc).triangles_in_boxes(np.zeros((2, 6), np.float32))
    assert err.value.code in (-2, -3) and str(err.value)
