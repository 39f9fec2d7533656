"""The kernel instantiations the shipped library holds, read from feathercnn_amd/libfeather_hip.so itself.

hipcc places one `__CLANG_OFFLOAD_BUNDLE__` per translation unit in the host ELF's `.hip_fatbin` section.  Each bundle lists its entries
(offset, size, target triple); the `hipv4-amdgcn-amd-amdhsa--gfx950` entries are device ELFs whose symbol table holds one `<name>.kd` kernel
descriptor per instantiated `__global__` function.  This module walks those bytes with `struct` (no LLVM tool), demangles the names with
`c++filt` and normalises them to `ns::name<args>` -- no return type, no parameter list -- e.g. `fhip::stream_gemm_kernel<8, true, false, true>`.

`instances()` -> sorted list of names; `base(name)` -> the unqualified kernel name (`stream_gemm_kernel`), the name tests/test_guarded_cpu.py's
scan of `__global__` declarations finds.
"""
from __future__ import annotations

import functools
import os
import struct
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "feathercnn_amd", "libfeather_hip.so")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
TARGET = "gfx950"


def _sections(elf: bytes) -> dict:
    """name -> (file offset, size) of a little-endian ELF64."""
    assert elf[:4] == b"\x7fELF" and elf[4] == 2 and elf[5] == 1, "not a little-endian ELF64"
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", elf, 0x3A)
    hdrs = [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + i * shentsize) for i in range(shnum)]
    strtab = hdrs[shstrndx][4]
    out = {}
    for h in hdrs:
        name = elf[strtab + h[0]:elf.index(b"\0", strtab + h[0])].decode()
        out[name] = (h[4], h[5], h[1], h[6], h[9])  # offset, size, type, link, entsize
    return out


def _section_list(elf: bytes) -> list:
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum, _ = struct.unpack_from("<HHH", elf, 0x3A)
    return [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + i * shentsize) for i in range(shnum)]


def code_objects(path: str = LIB, target: str = TARGET) -> list:
    """-> [bytes] of every device ELF for `target` in the library's .hip_fatbin section, in bundle order."""
    data = open(path, "rb").read()
    off, size = _sections(data)[".hip_fatbin"][:2]
    fat = data[off:off + size]
    objs, pos = [], fat.find(MAGIC)
    while pos >= 0:
        n, = struct.unpack_from("<Q", fat, pos + len(MAGIC))
        q = pos + len(MAGIC) + 8
        for _ in range(n):
            eoff, esize, tlen = struct.unpack_from("<QQQ", fat, q)
            triple = fat[q + 24:q + 24 + tlen].decode()
            q += 24 + tlen
            if triple.startswith("hip") and triple.endswith("-" + target) and esize:
                objs.append(fat[pos + eoff:pos + eoff + esize])
        pos = fat.find(MAGIC, pos + len(MAGIC))
    return objs


def kd_symbols(obj: bytes) -> list:
    """-> the mangled names (without `.kd`) of the kernel descriptors in one device ELF's symbol table."""
    secs = _section_list(obj)
    out = []
    for s in secs:
        if s[1] != 2:  # SHT_SYMTAB
            continue
        stroff = secs[s[6]][4]
        for i in range(s[5] // 24):
            st_name, = struct.unpack_from("<I", obj, s[4] + 24 * i)
            name = obj[stroff + st_name:obj.index(b"\0", stroff + st_name)].decode()
            if name.endswith(".kd"):
                out.append(name[:-3])
    return out


def normalise(demangled: str) -> str:
    """`void fhip::k<8, true>(float const*, int)` -> `fhip::k<8, true>`: drop the return type and the parameter list."""
    s = demangled.strip()
    if s.startswith("void "):
        s = s[5:]
    depth = 0
    for i, ch in enumerate(s):  # the parameter list is the first '(' outside template brackets
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0:
            return s[:i]
    return s


def base(name: str) -> str:
    """`fhip::stream_gemm_kernel<8, true, false, true>` -> `stream_gemm_kernel`."""
    return name.split("<", 1)[0].rsplit("::", 1)[-1]


def _demangle(names: list) -> list:
    if not names:
        return []
    r = subprocess.run(["c++filt"], input="\n".join(names) + "\n", capture_output=True, text=True, check=True)
    out = r.stdout.splitlines()
    assert len(out) == len(names), "c++filt returned a different number of lines"
    return out


@functools.lru_cache(maxsize=None)
def _instances(path: str, mtime: float) -> tuple:
    mangled = sorted({m for obj in code_objects(path) for m in kd_symbols(obj)})
    return tuple(sorted({normalise(d) for d in _demangle(mangled)}))


def instances(path: str = LIB) -> list:
    """-> sorted normalised names of every kernel instantiation in the library's gfx950 code objects."""
    return list(_instances(path, os.path.getmtime(path)))


if __name__ == "__main__":
    names = instances()
    for n in names:
        print(n)
    print(f"{len(names)} instantiations of {len({base(n) for n in names})} kernels")
