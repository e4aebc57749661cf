#!/usr/bin/env python3
"""kernel_diff.py A.so B.so [--hashes] [--by-address] — is the gfx950 device code of two builds of libsiren_fit.so the same?

The code object is taken out of each library in two steps (objcopy --only-section=.hip_fatbin, then
clang-offload-bundler --unbundle --targets=hipv4-amdgcn-amd-amdhsa--gfx950) and three of its ELF sections are compared
byte for byte: .text (instructions), .rodata (kernel descriptors) and .note (metadata: mangled names, argument layouts,
register and LDS counts).  The sha256 of the whole .hip_fatbin is too strict a test once a kernel source was edited:
the symbol and hash tables of the code object come out in another order while the three sections stay the same.

Exit status 0: the three sections are identical and both libraries define the same symbols.  Otherwise the kernels
whose byte range of .text differs are listed (ranges from the symbol table: address, size), and the symbols only one
library has.  Bytes only: nothing is disassembled and nothing is searched for.  --hashes prints the sha256 of the
three sections of both libraries.

--by-address is for a change that RENAMES kernels (other template arguments, the same instructions): the functions of
.text are paired by address order instead of by name, and the old -> new name of every renamed pair is printed (demangled
where llvm-cxxfilt or c++filt is at hand).  Exit status 0: both libraries hold the same number of functions, every pair has the same
offset in .text, the same size and the same bytes, and .text and .rodata are identical as a whole; .note then differs
only because it holds the mangled names, and is reported, not judged.
Other names have another length, so the name tables the linker lays out in front of .rodata and .text (.note, .dynstr)
change size, and the padding between the two sections (64- and 256-byte alignment) may change with them.  The words that
hold that distance then change by exactly its change d, and nothing else may: the entry offset of every kernel descriptor
(the 8 bytes at +16 of each `.kd` symbol: + d) and the 32-bit pc-relative offsets with which code reaches a constant table
in .rodata (- d).  Such words are counted and reported as "position words", with the functions that hold them; a differing
word of any other value, or anywhere else in .rodata, is a difference.  With d = 0 the comparison is exact.
"""
import hashlib
import os
import shutil
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


def functions(sections, symbols):
    """[(address, size, name)] of the functions of .text in address order (kernel descriptors, `.kd`, live in .rodata)"""
    return sorted((addr, size, n) for n, (sec, addr, size) in symbols.items() if sec == ".text" and size)


def demangled(names):
    filt = os.path.join(LLVM, "llvm-cxxfilt")
    filt = filt if os.path.exists(filt) else shutil.which("c++filt")
    if not names or not filt:
        return list(names)
    return subprocess.run([filt], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()


def by_address(sec_a, sym_a, sec_b, sym_b):
    fa, fb = functions(sec_a, sym_a), functions(sec_b, sym_b)
    (base_a, text_a), (base_b, text_b) = sec_a[".text"], sec_b[".text"]
    (ro_a, rodata_a), (ro_b, rodata_b) = sec_a[".rodata"], sec_b[".rodata"]
    d = (base_b - ro_b) - (base_a - ro_a)   # change of the distance from .rodata to .text
    print("%d and %d functions in .text; .text lies %d bytes behind .rodata in the first library, %d in the second"
          % (len(fa), len(fb), base_a - ro_a, base_b - ro_b))
    bad = len(fa) != len(fb) or len(text_a) != len(text_b) or len(rodata_a) != len(rodata_b)
    renamed, n_text_words = [], 0
    for (aa, sa, na), (ab, sb, nb) in zip(fa, fb):
        if na != nb:
            renamed.append((na, nb))
        oa, ob = aa - base_a, ab - base_b
        if (oa, sa) != (ob, sb):
            print("  differs: %s (at +%#x, %d bytes) and %s (at +%#x, %d bytes)" % (na, oa, sa, nb, ob, sb))
            bad = True
        elif text_a[oa:oa + sa] != text_b[ob:ob + sb]:
            words = [w for w in range(oa & ~3, oa + sa, 4) if text_a[w:w + 4] != text_b[w:w + 4]]
            moved = [w for w in words if struct.unpack_from("<i", text_b, w)[0] - struct.unpack_from("<i", text_a, w)[0] == -d]
            if d and moved == words:
                print("  %d position words (each %+d) in %s" % (len(words), -d, nb))
                n_text_words += len(words)
            else:
                print("  differs: %d words of %s and %s" % (len(words) - len(moved), na, nb))
                bad = True
    # between the functions (padding) nothing may differ either: every differing word of .text was counted above
    n_diff = sum(1 for w in range(0, min(len(text_a), len(text_b)), 4) if text_a[w:w + 4] != text_b[w:w + 4])
    if n_diff != n_text_words:
        print("  differs: %d words of .text outside the functions listed" % (n_diff - n_text_words))
        bad = True
    # .rodata: only the entry offsets of the kernel descriptors may change, each by d
    entry = {addr - ro_b + 16 for n, (sec, addr, _size) in sym_b.items() if sec == ".rodata" and n.endswith(".kd")}
    diff_ro = [o for o in range(0, min(len(rodata_a), len(rodata_b)), 8) if rodata_a[o:o + 8] != rodata_b[o:o + 8]]
    ok_ro = [o for o in diff_ro if o in entry and
             struct.unpack_from("<q", rodata_b, o)[0] - struct.unpack_from("<q", rodata_a, o)[0] == d]
    if diff_ro and (not d or ok_ro != diff_ro):
        print("  differs: %d words of .rodata that are no kernel entry offset moved by %+d" % (len(diff_ro) - len(ok_ro), d))
        bad = True
    for s, n in ((".text", n_text_words), (".rodata", len(ok_ro))):
        same = sec_a[s][1] == sec_b[s][1]
        print("%s %s (%d and %d bytes)" % (s, "identical" if same else "differs in %d position words" % n if not bad else "differs",
                                           len(sec_a[s][1]), len(sec_b[s][1])))
    print(".note %s (it holds the mangled names)" % ("identical" if sec_a[".note"][1] == sec_b[".note"][1] else "differs"))
    old, new = demangled([a for a, _ in renamed]), demangled([b for _, b in renamed])
    print("%d of %d functions renamed" % (len(renamed), len(fa)))
    for o, n in zip(old, new):
        print("  %s -> %s" % (o, n))
    if not bad:
        print("identical function for function: %d functions of %d kernels%s"
              % (len(fa), sum(1 for n in sym_a if n.endswith(".kd")),
                 "" if not d else ", apart from the position words (the distance from .rodata to .text changed by %+d)" % d))
    return 1 if bad else 0


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
    if "--by-address" in argv:
        return by_address(sec_a, sym_a, sec_b, sym_b)
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
