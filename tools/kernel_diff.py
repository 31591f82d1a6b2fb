#!/usr/bin/env python3
"""Kernel-by-kernel comparison of two builds of libmvsv.so: for every gfx950
code object embedded in each library (.hip_fatbin -> clang offload bundles ->
ELF), the kernels by mangled name with their register counts, scratch and LDS
bytes (AMDGPU metadata notes) and the bytes of the kernel's symbol in .text.

    python tools/kernel_diff.py A.so B.so

Prints the kernels present on one side only, the kernels a library holds more
than once, and the kernels whose metadata or code bytes differ; exits non-zero
on any of them.  A source move that changes no kernel leaves nothing to print.
"""
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
FIELDS = (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def code_objects(lib):
    """The gfx950 code objects (ELF images, bytes) of every offload bundle in lib."""
    with tempfile.TemporaryDirectory() as td:
        fat = os.path.join(td, "fat.bin")
        subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", lib,
                        os.path.join(td, "x.so")], check=True, capture_output=True)
        b = open(fat, "rb").read()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    i = b.find(magic)
    while i >= 0:
        n = struct.unpack_from("<Q", b, i + len(magic))[0]
        p = i + len(magic) + 8
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", b, p)
            p += 24
            triple = b[p:p + tl].decode()
            p += tl
            if "gfx950" in triple and size:
                yield b[i + off:i + off + size]
        i = b.find(magic, i + 1)


def kernel_metadata(co):
    """[(mangled kernel name, {metadata field: int})] of one code object file."""
    notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], check=True, capture_output=True,
                           text=True).stdout
    out, cur = [], {}
    for line in notes.splitlines():
        m = re.match(r"\s+(?:- )?(\.\w+):\s+(\S+)", line)
        if not m:
            continue
        cur[m.group(1)] = m.group(2)
        # a kernel's keys are sorted: its own .name follows its arguments', .wavefront_size ends it
        if m.group(1) == ".wavefront_size":
            out.append((cur[".name"], {k: int(cur[k]) for k in FIELDS}))
            cur = {}
    return out


def kernel_code(co):
    """{symbol name: bytes in .text} for the function symbols of one code object file."""
    img = open(co, "rb").read()
    run = lambda *a: subprocess.run([f"{LLVM}/llvm-readelf", "--wide", *a, co], check=True,
                                    capture_output=True, text=True).stdout
    text = None
    for line in run("-S").splitlines():
        m = re.match(r"\s*\[\s*(\d+)\]\s+\.text\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", line)
        if m:
            text = (m.group(1), int(m.group(2), 16), int(m.group(3), 16))
    out = {}
    for line in run("-s").splitlines():
        f = line.split()
        if len(f) == 8 and f[3] == "FUNC" and text and f[6] == text[0]:
            a = text[2] + int(f[1], 16) - text[1]
            out[f[7]] = img[a:a + int(f[2])]
    return out


def kernels(lib):
    """({kernel: (metadata, code bytes)}, [kernels held more than once]) of a library."""
    out, twice = {}, []
    with tempfile.TemporaryDirectory() as td:
        co = os.path.join(td, "dev.co")
        for image in code_objects(lib):
            open(co, "wb").write(image)
            code = kernel_code(co)
            for name, meta in kernel_metadata(co):
                if name in out:
                    twice.append(name)
                out[name] = (meta, code.get(name))
    return out, twice


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    (a, a2), (b, b2) = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = 0
    for tag, only in (("only in A", sorted(set(a) - set(b))), ("only in B", sorted(set(b) - set(a))),
                      ("twice in A", a2), ("twice in B", b2)):
        for k in only:
            print(f"{tag}: {k}")
        bad += len(only)
    for k in sorted(set(a) & set(b)):
        (ma, ca), (mb, cb) = a[k], b[k]
        if ma != mb:
            print(f"metadata differs: {k}: {ma} vs {mb}")
        if ca is None or cb is None or ca != cb:
            la, lb = (len(c) if c is not None else None for c in (ca, cb))
            print(f"code differs: {k}: {la} vs {lb} bytes")
        bad += ma != mb or ca is None or ca != cb
    print(f"A: {len(a)} kernels, B: {len(b)} kernels, {bad} differences")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
