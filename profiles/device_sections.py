"""Digests of what a library's gfx950 code object executes: sha256 of its .text (the instructions), .rodata (the kernel
descriptors) and .note (per kernel: registers, spills, LDS, scratch).  A move of device code between files that leaves the
three as they were has changed neither behaviour nor speed.  buildhash.py's hash of the whole
.hip_fatbin also covers the symbol tables, where the compiler puts a name it derives from the unit's text.

    python profiles/device_sections.py shader-ray_amd/libshray_overlap.so [more libraries, or device-only objects of
                                                                          hipcc --cuda-device-only -c]"""
import hashlib
import os
import subprocess
import sys
import tempfile

from buildhash import _section

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
SECTIONS = (".text", ".rodata", ".note")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def _run(tool, *args):
    return subprocess.run([os.path.join(LLVM, tool), *args], check=True, capture_output=True, text=True).stdout


def _code_objects(path, tmp):
    """the gfx950 code objects of a library (one bundle per unit in its .hip_fatbin), or the device-only object itself"""
    blob = _section(path, ".hip_fatbin")
    if blob is None:
        return [path]
    found = []
    for k, bundle in enumerate(MAGIC + part for part in blob.split(MAGIC)[1:]):
        packed = os.path.join(tmp, f"bundle{k}")
        with open(packed, "wb") as f:
            f.write(bundle)
        # (the triple's prefix differs between -c and -shared builds: pick the target by its architecture)
        targets = [t for t in _run("clang-offload-bundler", "--list", "--type=o", f"--input={packed}").split() if t.endswith("gfx950")]
        if len(targets) != 1:
            raise RuntimeError(f"{path}: bundle {k} has gfx950 targets {targets}")
        found.append(packed + ".co")
        _run("clang-offload-bundler", "--unbundle", "--type=o", f"--input={packed}", f"--targets={targets[0]}", f"--output={found[-1]}")
    return found


def device_sections(path):
    """{section: sha256 over that section of every gfx950 code object of `path`, in the library's order}"""
    digests = {s: hashlib.sha256() for s in SECTIONS}
    with tempfile.TemporaryDirectory() as tmp:
        for obj in _code_objects(path, tmp):
            for s in SECTIONS:
                raw = os.path.join(tmp, "section.bin")
                _run("llvm-objcopy", "-O", "binary", f"--only-section={s}", obj, raw)
                with open(raw, "rb") as f:
                    digests[s].update(f.read())
    return {s: d.hexdigest() for s, d in digests.items()}


if __name__ == "__main__":
    for lib in sys.argv[1:]:
        print(os.path.basename(lib), *(f"{s} {d[:16]}" for s, d in device_sections(lib).items()))
