"""Reader for the section dumps written by oracle/_ref/ref_host (oracle/ref_driver.cpp)."""
import hashlib
import struct

import numpy as np


def read_dump(path: str) -> dict:
    out = {}
    with open(path, "rb") as f:
        blob = f.read()
    assert blob[:4] == b"SHRD", "not a ref_host dump"
    pos = 4
    while pos < len(blob):
        (name_len,) = struct.unpack_from("<I", blob, pos)
        pos += 4
        name = blob[pos:pos + name_len].decode()
        pos += name_len
        (count,) = struct.unpack_from("<Q", blob, pos)
        pos += 8
        out[name] = np.frombuffer(blob, dtype="<f4", count=count, offset=pos).copy()
        pos += 4 * count
    return out


def bits_sha256(a) -> str:
    """SHA-256 of an array's float32 bit patterns (little-endian): equal digests = equal arrays, bit for bit."""
    return hashlib.sha256(np.ascontiguousarray(a, dtype="<f4").view("<u4").tobytes()).hexdigest()


def digest_large(dump: dict, above: int) -> dict:
    """The dump with every array of more than `above` floats replaced by `<name>.sha256` (bits_sha256) and `<name>.size`:
    a fixture of a large scene small enough to commit that still pins every bit."""
    out = {}
    for name, a in dump.items():
        a = np.asarray(a)
        if a.size > above:
            out[name + ".sha256"] = np.array(bits_sha256(a))
            out[name + ".size"] = np.array(a.size, dtype=np.int64)
        else:
            out[name] = a
    return out
