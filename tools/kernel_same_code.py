#!/usr/bin/env python3
"""kernel_same_code.py — do two builds of libcray_hip.so hold the same instructions in the kernels whose names contain one of the given substrings?

    python tools/kernel_same_code.py OLD.so NEW.so [k_pathtrace_roll k_aov ...]

Adding a kernel to csrc/cray_hip.hip lengthens .rodata in front of .text, which moves the PC-relative literals (`s_add_u32 / s_addc_u32 …, <offset>` behind
`s_getpc_b64`) of every kernel and with them bench.py's kernel_source_md5. This tool takes the gfx950 code object of that translation unit out of each library,
disassembles the named kernels (llvm-objdump), masks those literals and compares the listings line by line. Exit status 0: the same instructions."""
import os
import re
import struct
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"


def code_object(lib):
    """The gfx code object that holds the path-tracing kernels (bench.py: kernel_source_md5 reads the same one)."""
    import bench
    data = open(lib, "rb").read()
    secs, _ = bench._elf64_sections(data)
    _t, _a, off, size = secs[".hip_fatbin"][:4]
    fat = data[off:off + size]
    magic, pos = b"__CLANG_OFFLOAD_BUNDLE__", 0
    while True:
        p = fat.find(magic, pos)
        if p < 0:
            raise SystemExit(f"{lib}: no gfx code object with k_pathtrace in it")
        n, = struct.unpack_from("<Q", fat, p + 24)
        q = p + 32
        for _ in range(n):
            o, sz, ts = struct.unpack_from("<QQQ", fat, q)
            triple = fat[q + 24:q + 24 + ts]
            q += 24 + ts
            obj = fat[p + o:p + o + sz]
            if b"gfx" in triple and b"k_pathtrace" in obj:
                return obj
        pos = p + len(magic)


def listing(lib, names):
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(code_object(lib))
        f.flush()
        text = subprocess.check_output([OBJDUMP, "-d", "--no-show-raw-insn", "--no-leading-addr", f.name], stderr=subprocess.DEVNULL).decode(errors="replace")
    out, on = [], False
    for line in text.splitlines():
        m = re.match(r"^<([^>]*)>:", line)
        if m:
            on = any(n in m.group(1) for n in names)
        if on:
            line = re.sub(r"//.*$", "", line).rstrip()
            out.append(re.sub(r"(s_add_u32|s_addc_u32)( [^,]+,[^,]+,) *(0x[0-9a-f]+|-?[0-9]+)$", r"\1\2 LIT", line))
    return out


def main():
    if len(sys.argv) < 3:
        raise SystemExit(__doc__)
    names = sys.argv[3:] or ["k_pathtrace_roll", "k_aov"]
    a, b = listing(sys.argv[1], names), listing(sys.argv[2], names)
    differ = sum(1 for x, y in zip(a, b) if x != y) + abs(len(a) - len(b))
    print(f"{', '.join(names)}: {len(a)} / {len(b)} lines, {differ} differ (PC-relative literals masked)")
    sys.exit(1 if differ or not a else 0)


if __name__ == "__main__":
    main()
