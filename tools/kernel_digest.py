"""Digest of every kernel a source file compiles to: are this tree's kernels the ones another commit's were?

  python tools/kernel_digest.py [--csrc DIR] [FILE.hip ...]        (no files: every file of build.py's SOURCES)

Each file is compiled for the device alone with build.py's FLAGS (-DSC_ABLATIONS with --ablations); for every kernel of
the resulting gfx950 code object one line is printed, sorted by name:  <file> <kernel symbol> <code bytes> <sha256>.
The hash covers the kernel's code bytes and its 64-byte descriptor (<symbol>.kd) with the descriptor's
kernel_code_entry_byte_offset (bytes 16 .. 23) zeroed: that field is the distance from the descriptor to the code, which
moves with every other kernel of the file.  Two listings — one made with --csrc pointing at another checkout's csrc — are
compared with --compare A B: kernels are matched by name across files (a kernel may have moved to another file), and the
exit status is 0 only if both hold the same names with the same digests.  Only hashes: no instruction is looked at.
Needs hipcc, no GPU.
"""
from __future__ import annotations

import argparse
import hashlib
import importlib.util
import os
import struct
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
BUILD_PY = os.path.join(HERE, "..", "sac-cot_amd", "build.py")


def _build_module():
    spec = importlib.util.spec_from_file_location("saccot_build", BUILD_PY)
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b


def elf_kernels(blob: bytes):
    """[(name, size, sha256)] of the FUNC symbols of a little-endian ELF64 that have a <name>.kd object beside them."""
    if blob[:6] != b"\x7fELF\x02\x01":
        raise ValueError("not a little-endian ELF64 (is the output still a bundle?)")
    shoff, = struct.unpack_from("<Q", blob, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", blob, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", blob, shoff + k * shentsize) for k in range(shnum)]  # name type flags addr off size link info align entsize

    def at(sec_index: int, addr: int, size: int) -> bytes:
        s = secs[sec_index]
        if s[1] == 8:  # SHT_NOBITS
            raise ValueError("symbol in a section without bytes")
        off = s[4] + (addr - s[3])
        return blob[off:off + size]

    funcs, objects = {}, {}
    for s in secs:
        if s[1] != 2:  # SHT_SYMTAB
            continue
        strtab = secs[s[6]]
        for k in range(s[5] // 24):
            name_off, info, _other, shndx, value, size = struct.unpack_from("<IBBHQQ", blob, s[4] + 24 * k)
            end = blob.index(b"\0", strtab[4] + name_off)
            name = blob[strtab[4] + name_off:end].decode()
            if shndx == 0 or shndx >= 0xFF00:
                continue
            if info & 0xF == 2:
                funcs[name] = (shndx, value, size)
            elif info & 0xF == 1:
                objects[name] = (shndx, value, size)
    out = []
    for name, (shndx, value, size) in funcs.items():
        kd = objects.get(name + ".kd")
        if kd is None or kd[2] != 64:
            raise ValueError(f"{name}: a function without a 64-byte kernel descriptor (an out-of-line device function?)")
        desc = bytearray(at(kd[0], kd[1], 64))
        desc[16:24] = bytes(8)  # kernel_code_entry_byte_offset
        out.append((name, size, hashlib.sha256(at(shndx, value, size) + bytes(desc)).hexdigest()))
    return sorted(out)


def digest_file(b, src: str, ablations: bool):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    flags = b.FLAGS + (["-DSC_ABLATIONS"] if ablations else [])
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "device.elf")
        subprocess.check_call([hipcc] + flags + ["--offload-device-only", "--no-gpu-bundle-output", "-c", src, "-o", out])
        with open(out, "rb") as f:
            return elf_kernels(f.read())


def read_listing(path: str):
    kernels = {}
    with open(path) as f:
        for line in f:
            parts = line.split()
            if len(parts) != 4:
                continue
            if parts[1] in kernels:
                raise SystemExit(f"{path}: {parts[1]} listed twice")
            kernels[parts[1]] = (parts[0], parts[2], parts[3])
    return kernels


def compare(path_a: str, path_b: str) -> int:
    a, b = read_listing(path_a), read_listing(path_b)
    bad = 0
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            print(f"only in {path_a if name in a else path_b}: {name}")
            bad += 1
        elif a[name][1:] != b[name][1:]:
            print(f"differs: {name}  ({a[name][0]} {a[name][1]} bytes -> {b[name][0]} {b[name][1]} bytes)")
            bad += 1
    moved = sum(1 for name in a if name in b and a[name][0] != b[name][0])
    if not bad:
        print(f"all {len(a)} kernels identical ({moved} of them in another file)")
    return 1 if bad else 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("files", nargs="*", help="source files (names relative to --csrc, or paths); default: build.py's SOURCES")
    ap.add_argument("--csrc", default=None, help="directory of the sources (default: this tree's sac-cot_amd/csrc)")
    ap.add_argument("--ablations", action="store_true")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"), help="compare two listings instead of making one")
    args = ap.parse_args()
    if args.compare:
        return compare(*args.compare)
    b = _build_module()
    csrc = args.csrc or b.CSRC
    files = args.files
    if not files:  # the SOURCES of the checkout the sources come from
        other = os.path.join(csrc, "..", "build.py")
        files = b.SOURCES
        if args.csrc and os.path.exists(other):
            spec = importlib.util.spec_from_file_location("saccot_build_other", other)
            ob = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(ob)
            files = ob.SOURCES
    for name in files:
        src = name if os.path.exists(name) else os.path.join(csrc, name)
        for kernel, size, sha in digest_file(b, src, args.ablations):
            print(os.path.basename(src), kernel, size, sha, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
