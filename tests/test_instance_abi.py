"""include/shader_ray_instance.h against libshray_instance.so and the ctypes mirror: every declared function is exported and
bound, shray_instance's layout matches the compiled header, and without a usable scene creating a set fails with an error."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "shader_ray_instance.h")


def declared():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return set(re.findall(r"^\s*(?:int|void)\s+\**(shray_\w+)\s*\(", text, flags=re.M))


def test_header_symbols_are_exported_and_bound(pkg):
    names = declared()
    assert names == {n for n, _, _ in pkg._native.INSTANCE_SYMBOLS}
    lib = pkg._native.load_instance()
    out = subprocess.run(["nm", "-D", "--defined-only", pkg._native.INSTANCE_LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (shray_\w+)", out))
    assert names <= exported, names - exported
    for n in names:
        assert getattr(lib, n) is not None


def test_instance_layout_matches_the_header(pkg, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "shader_ray_instance.h"\n'
                   'int main(void) { printf("%zu %zu %zu\\n", sizeof(shray_instance), offsetof(shray_instance, scene), '
                   'offsetof(shray_instance, object_to_world)); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    size, scene, m = map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split())
    I = pkg._native.Instance
    assert (size, scene, m) == (C.sizeof(I), I.scene.offset, I.object_to_world.offset)


def test_create_refuses_bad_arguments(pkg):
    N = pkg._native
    lib = N.load_instance()
    inst = (N.Instance * 1)()
    out = C.c_void_p()
    assert lib.shray_instance_set_create(None, 1, C.byref(out)) == -1 and not out.value
    assert lib.shray_instance_set_create(inst, 1, None) == -1
    assert lib.shray_instance_set_create(inst, 0, C.byref(out)) == -1
    assert lib.shray_instance_set_create(inst, N.INSTANCE_MAX + 1, C.byref(out)) == -1
    with pytest.raises(N.ShrayError):
        N.check(lib.shray_instance_set_update(None, None))


def test_create_without_a_gpu_fails_with_no_device(pkg):
    """Without a visible HIP device, creating a set fails with SHRAY_ERR_NO_DEVICE before any scene is read; with one, the
    same call is refused for its NULL scene."""
    N = pkg._native
    lib = N.load_instance()
    n = C.c_int()
    have_gpu = N.load_hip().shray_device_count(C.byref(n)) == 0 and n.value > 0
    inst = (N.Instance * 1)()
    inst[0].object_to_world[0] = inst[0].object_to_world[5] = inst[0].object_to_world[10] = 1.0
    out = C.c_void_p()
    rc = lib.shray_instance_set_create(inst, 1, C.byref(out))
    assert not out.value
    message = N.load_hip().shray_last_error()
    if have_gpu:
        assert rc == -1 and b"NULL" in message
    else:
        assert rc == -2 and b"no HIP device" in message
