#!/usr/bin/env python3
"""List every gfx950 kernel of a built library with the resources its code object records:

    python tools/kernel_meta.py vae_play_amd/libvaeplay_hip.so > new.txt

One line per kernel, sorted: demangled-as-stored symbol, VGPRs, AGPRs, SGPRs, LDS bytes, scratch bytes.  Two builds whose host code
differs and whose device code does not give identical listings (DESIGN.md section 24 compares a refactor with its parent this way).
Needs the ROCm LLVM tools (llvm-objcopy, llvm-readelf); no GPU."""
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM_BIN", "/opt/rocm/lib/llvm/bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
FIELDS = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")


def code_objects(lib, arch):
    """the device ELF images for `arch` of every translation unit: the .hip_fatbin section is a sequence of uncompressed offload bundles"""
    with tempfile.TemporaryDirectory() as d:
        raw = os.path.join(d, "fatbin")
        subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", f".hip_fatbin={raw}", lib, os.path.join(d, "copy")])
        blob = open(raw, "rb").read()
    assert b"CCOB" not in blob[:4], "compressed offload bundles are not handled: build without --offload-compress"
    at = blob.find(MAGIC)
    while at >= 0:
        (n,) = struct.unpack_from("<Q", blob, at + len(MAGIC))
        pos = at + len(MAGIC) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", blob, pos)
            triple = blob[pos + 24:pos + 24 + tlen].decode()
            pos += 24 + tlen
            if arch in triple and size:
                yield blob[at + off:at + off + size]
        at = blob.find(MAGIC, at + len(MAGIC))


def kernels(lib, arch="gfx950"):
    rows = []
    for image in code_objects(lib, arch):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(image)
            f.flush()
            notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", f.name], text=True)
        for entry in re.split(r"\n\s+- \.", notes)[1:]:      # one metadata map per kernel
            get = lambda key: re.search(rf"\.?{key}:\s*(\S+)", entry)
            if not get("symbol") or not get("vgpr_count"):
                continue
            rows.append(" ".join([get("symbol").group(1).strip("'")] + [f"{k.split('_')[0]}={get(k).group(1)}" for k in FIELDS if get(k)]))
    return sorted(rows)


if __name__ == "__main__":
    print("\n".join(kernels(sys.argv[1])))
