"""The device update of an instance set (include/shader_ray_instance.h: shray_instance_set_update_device and
shray_instance_set_update_status) against libshray_instance.so and the ctypes mirror: both are declared, exported and bound,
the tests' accessor shrayi_instance_set_arrays is exported but stays out of the header, and a NULL set is refused at the call."""
import ctypes as C
import re
import subprocess

import pytest

from test_instance_abi import HEADER, declared

NEW = {"shray_instance_set_update_device", "shray_instance_set_update_status"}


def exported(pkg):
    out = subprocess.run(["nm", "-D", "--defined-only", pkg._native.INSTANCE_LIB], capture_output=True, text=True, check=True).stdout
    return set(re.findall(r"\bT (shray\w+)", out))


def test_update_device_is_declared_exported_and_bound(pkg):
    assert NEW <= declared()
    assert NEW <= {n for n, _, _ in pkg._native.INSTANCE_SYMBOLS}
    assert NEW <= exported(pkg)
    lib = pkg._native.load_instance()
    for n in NEW:
        assert getattr(lib, n).argtypes is not None


def test_the_arrays_accessor_is_internal(pkg):
    assert "shrayi_instance_set_arrays" in exported(pkg)
    assert "shrayi_instance_set_arrays" not in open(HEADER).read()
    assert getattr(pkg._native.load_instance(), "shrayi_instance_set_arrays").argtypes is not None


def test_a_null_set_is_refused(pkg):
    N = pkg._native
    lib = N.load_instance()
    assert lib.shray_instance_set_update_device(None, None, None) == -1
    assert b"NULL" in N.load_hip().shray_last_error()
    refused = C.c_int32(5)
    assert lib.shray_instance_set_update_status(None, C.byref(refused)) == -1
    assert lib.shray_instance_set_update_status(None, None) == -1
    count = C.c_int32()
    assert lib.shrayi_instance_set_arrays(None, None, None, C.byref(count)) == -1
    with pytest.raises(N.ShrayError):
        N.check(lib.shray_instance_set_update_device(None, None, None))
