#!/usr/bin/env python3
"""Scratch memory and spilled registers of every kernel in the built library, read from the metadata notes of its gfx950 code objects.

usage: tools/kernel_resources.py [--write] [filter]
  prints  <scratch bytes> <spilled VGPRs> <kernel symbol>  per kernel; --write regenerates the table in force, GOLDEN below
  (the ceilings tests/test_kernel_resources.py holds every kernel to), from the library as built.

Tables: tests/golden/kernel_resources.json is the first table, frozen as committed; kernel_ceilings.json extended it by the kernels of
top-down inference on full frames and is the fixture of tests/test_kernel_ceilings.py; GOLDEN = kernel_ceilings_roi.json is the table
in force: kernel_ceilings.json, entry for entry, plus the oriented-ROI and One-Euro kernels (both earlier files are fixtures of tests
that stay as committed, so the new entries went into a file of their own).  The table in force only extends the earlier ones
(tests/test_kernel_ceilings.py, tests/test_roi_host.py): a kernel can gain an entry or earn a lower one, never a higher one.

The library carries one clang offload bundle per translation unit in its .hip_fatbin section; each bundle holds the gfx950 code object
whose NT_AMDGPU_METADATA note lists .private_segment_fixed_size and .vgpr_spill_count per kernel (llvm-readelf --notes prints it)."""
import json
import os
import re
import shutil
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "lighthand_amd", "liblighthand_hip.so")
FROZEN = os.path.join(ROOT, "tests", "golden", "kernel_resources.json")
GOLDEN = os.path.join(ROOT, "tests", "golden", "kernel_ceilings_roi.json")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def find_tool(name):
    """An LLVM tool of the ROCm installation (or of PATH); None when there is none."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for d in (os.path.join(rocm, "lib", "llvm", "bin"), os.path.join(rocm, "llvm", "bin")):
        p = os.path.join(d, name)
        if os.access(p, os.X_OK):
            return p
    return shutil.which(name)


def tools_present():
    return all(find_tool(t) for t in ("llvm-readelf", "llvm-objcopy"))


def code_objects(fatbin, arch="gfx950"):
    """The device code objects for `arch` inside the bytes of a .hip_fatbin section (uncompressed clang offload bundles)."""
    out, pos = [], fatbin.find(MAGIC)
    while pos >= 0:
        n, = struct.unpack_from("<Q", fatbin, pos + len(MAGIC))
        q = pos + len(MAGIC) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", fatbin, q)
            triple = fatbin[q + 24:q + 24 + tlen].decode()
            q += 24 + tlen
            if triple.startswith("hip") and triple.rstrip("-").endswith(arch) and size:
                out.append(fatbin[pos + off:pos + off + size])
        pos = fatbin.find(MAGIC, pos + 1)
    return out


def read_resources(lib=LIB):
    """{kernel symbol (mangled: the names are exact and need no demangler): [scratch bytes, spilled VGPRs]} of every kernel in the library."""
    readelf, objcopy = find_tool("llvm-readelf"), find_tool("llvm-objcopy")
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        fat = os.path.join(tmp, "fatbin")
        subprocess.run([objcopy, "--dump-section", ".hip_fatbin=" + fat, lib, os.path.join(tmp, "copy.so")], check=True, capture_output=True)
        with open(fat, "rb") as f:
            objs = code_objects(f.read())
        if not objs:
            raise RuntimeError(f"{lib}: no gfx950 code object in .hip_fatbin")
        for i, co in enumerate(objs):
            path = os.path.join(tmp, f"co{i}.elf")
            with open(path, "wb") as f:
                f.write(co)
            notes = subprocess.run([readelf, "--notes", path], check=True, capture_output=True, text=True).stdout
            # one "- .agpr_count: ..." item per kernel; keys are sorted, so walk the items and pick the three fields
            for item in re.split(r"\n\s+- \.agpr_count:", notes)[1:]:
                name = re.search(r"^\s+\.symbol:\s+(\S+)\.kd\s*$", item, re.M)      # (.name also labels kernel arguments)
                scratch = re.search(r"^\s+\.private_segment_fixed_size:\s+(\d+)", item, re.M)
                spill = re.search(r"^\s+\.vgpr_spill_count:\s+(\d+)", item, re.M)
                if not (name and scratch and spill):
                    raise RuntimeError("kernel metadata item without .name / .private_segment_fixed_size / .vgpr_spill_count")
                res[name.group(1)] = [int(scratch.group(1)), int(spill.group(1))]
    return res


def main():
    args = [a for a in sys.argv[1:] if a != "--write"]
    res = read_resources()
    if "--write" in sys.argv[1:]:
        with open(GOLDEN, "w") as f:
            f.write("{\n" + ",\n".join(f"  {json.dumps(k)}: {json.dumps(v)}" for k, v in sorted(res.items())) + "\n}\n")
        print(f"{len(res)} kernels -> {GOLDEN}")
        return
    for k, (scratch, spill) in sorted(res.items()):
        if not args or args[0] in k:
            print(f"{scratch:5d} {spill:4d}  {k}")


if __name__ == "__main__":
    main()
