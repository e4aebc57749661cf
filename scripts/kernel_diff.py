#!/usr/bin/env python3
"""kernel_diff.py A.so B.so [--hashes] — is the gfx950 device code of two builds of libsiren_fit.so the same?

The code object is taken out of each library in two steps (objcopy --only-section=.hip_fatbin, then
clang-offload-bundler --unbundle --targets=hipv4-amdgcn-amd-amdhsa--gfx950) and three of its ELF sections are compared
byte for byte: .text (instructions), .rodata (kernel descriptors) and .note (metadata: mangled names, argument layouts,
register and LDS counts).  The sha256 of the whole .hip_fatbin is too strict a test once a kernel source was edited:
the symbol and hash tables of the code object come out in another order while the three sections stay the same.

Exit status 0: the three sections are identical and both libraries define the same symbols.  Otherwise the kernels
whose byte range of .text differs are listed (ranges from the symbol table: address, size), and the symbols only one
library has.  Bytes only: nothing is disassembled and nothing is searched for.  --hashes prints the sha256 of the
three sections of both libraries.
"""
import hashlib
import os
import struct
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM_BIN", "/opt/rocm/lib/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
SECTIONS = (".text", ".rodata", ".note")


def code_object(lib, tmp):
    """bytes of the gfx950 code object bundled in `lib`"""
    tag = hashlib.sha256(os.path.abspath(lib).encode()).hexdigest()[:12]
    fat, co = os.path.join(tmp, tag + ".fatbin"), os.path.join(tmp, tag + ".co")
    objcopy = os.path.join(LLVM, "llvm-objcopy")
    subprocess.check_call([objcopy if os.path.exists(objcopy) else "objcopy", "-O", "binary",
                           "--only-section=.hip_fatbin", lib, fat])
    subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--unbundle", "--input=" + fat,
                           "--targets=" + TARGET, "--output=" + co])
    with open(co, "rb") as f:
        return f.read()


def parse_elf(b):
    """-> ({section name: (address, bytes)}, {symbol name: (section name, address, size)}) of a little-endian ELF64"""
    if b[:4] != b"\x7fELF" or b[4] != 2 or b[5] != 1:
        raise ValueError("not a little-endian ELF64 code object")
    shoff, = struct.unpack_from("<Q", b, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", b, 0x3A)
    hdr = [struct.unpack_from("<IIQQQQIIQQ", b, shoff + i * shentsize) for i in range(shnum)]

    def cstr(tab, off):
        return tab[off:tab.index(b"\0", off)].decode()

    def body(h):
        return b"" if h[1] == 8 else b[h[4]:h[4] + h[5]]   # SHT_NOBITS holds no bytes

    shstr = body(hdr[shstrndx])
    names = [cstr(shstr, h[0]) for h in hdr]
    sections = {n: (h[3], body(h)) for n, h in zip(names, hdr)}
    symbols = {}
    for h in hdr:
        if h[1] != 2:   # SHT_SYMTAB
            continue
        strtab, tab = body(hdr[h[6]]), body(h)
        for off in range(0, len(tab), 24):
            name, _info, _other, shndx, value, size = struct.unpack_from("<IBBHQQ", tab, off)
            if name and 0 < shndx < shnum:
                symbols[cstr(strtab, name)] = (names[shndx], value, size)
    return sections, symbols


def main(argv):
    args = [a for a in argv if not a.startswith("--")]
    if len(args) != 2:
        print(__doc__)
        return 2
    with tempfile.TemporaryDirectory() as tmp:
        (sec_a, sym_a), (sec_b, sym_b) = (parse_elf(code_object(lib, tmp)) for lib in args)
    if "--hashes" in argv:
        for lib, sec in zip(args, (sec_a, sec_b)):
            for s in SECTIONS:
                print("%s  %-8s %8d bytes  %s" % (hashlib.sha256(sec[s][1]).hexdigest(), s, len(sec[s][1]), lib))
    differing = [s for s in SECTIONS if sec_a[s][1] != sec_b[s][1]]
    only_a, only_b = sorted(set(sym_a) - set(sym_b)), sorted(set(sym_b) - set(sym_a))
    n_kernels = sum(1 for n in sym_a if n.endswith(".kd"))
    if not differing and not only_a and not only_b:
        print("identical: %s of %d kernels, %d symbols" % (", ".join(SECTIONS), n_kernels, len(sym_a)))
        return 0
    for s in differing:
        print("%s differs (%d and %d bytes)" % (s, len(sec_a[s][1]), len(sec_b[s][1])))
    # a function's bytes are compared range against range, so one that only moved is not listed
    (base_a, text_a), (base_b, text_b) = sec_a[".text"], sec_b[".text"]
    changed = [n for n in sorted(set(sym_a) & set(sym_b))
               if sym_a[n][0] == ".text" and sym_b[n][0] == ".text" and sym_a[n][2] and
               text_a[sym_a[n][1] - base_a:sym_a[n][1] - base_a + sym_a[n][2]] !=
               text_b[sym_b[n][1] - base_b:sym_b[n][1] - base_b + sym_b[n][2]]]
    print("%d of %d kernels differ in .text" % (len(changed), n_kernels))
    for n in changed:
        print("  %s  (%d -> %d bytes)" % (n, sym_a[n][2], sym_b[n][2]))
    for tag, names in (("first", only_a), ("second", only_b)):
        for n in names:
            print("  only in the %s library: %s" % (tag, n))
    return 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
