"""Do two builds of libtfft.so hold the same device code? CPU only: the gfx950 code objects of both (llvm-objdump --offloading, as
tools/kernel_resources.py) are compared as whole files, then function by function: symbol lists, the bytes of every function and
the vgpr / agpr / sgpr / scratch / lds notes of every kernel. Bytes and names only.
usage: python tools/compare_code_objects.py A.so B.so      (exit status 0: same device code)"""
import os
import shutil
import struct
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_resources import LLVM_BIN, resources  # noqa: E402


def code_object(so_path):
    tmp = tempfile.mkdtemp(prefix="tfft_co_")
    try:
        local = os.path.join(tmp, os.path.basename(so_path))
        shutil.copy(so_path, local)
        subprocess.check_call([os.path.join(LLVM_BIN, "llvm-objdump"), "--offloading", local], cwd=tmp,
                              stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        co = [f for f in os.listdir(tmp) if "amdgcn" in f and "gfx950" in f][0]
        with open(os.path.join(tmp, co), "rb") as f:
            return f.read()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def functions(elf):
    """{symbol: bytes} of every function symbol of a little-endian ELF64 image"""
    assert elf[:6] == b"\x7fELF\x02\x01", "not a little-endian ELF64 file"
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", elf, 0x3A)
    sections = [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + i * shentsize) for i in range(shnum)]
    out = {}
    for _, sh_type, _, _, offset, size, link, _, _, entsize in sections:
        if sh_type != 2:        # SHT_SYMTAB
            continue
        strtab = sections[link]
        for i in range(size // entsize):
            name, info, _, shndx, value, fsize = struct.unpack_from("<IBBHQQ", elf, offset + i * entsize)
            if (info & 15) != 2 or shndx == 0 or shndx >= shnum:        # STT_FUNC, defined
                continue
            end = elf.index(b"\0", strtab[4] + name)
            sec = sections[shndx]
            start = sec[4] + value - sec[3]
            out[elf[strtab[4] + name:end].decode()] = elf[start:start + fsize]
    return out


def main(a_path, b_path):
    a, b = code_object(a_path), code_object(b_path)
    if a == b:
        print(f"the gfx950 code objects are byte-identical ({len(a)} bytes)")
        return 0
    fa, fb = functions(a), functions(b)
    ra, rb = resources(a_path), resources(b_path)
    only = sorted(set(fa) ^ set(fb))
    differ = sorted(k for k in set(fa) & set(fb) if fa[k] != fb[k])
    notes = sorted(k for k in set(ra) | set(rb) if ra.get(k) != rb.get(k))
    print(f"code objects differ as files ({len(a)} / {len(b)} bytes); {len(fa)} / {len(fb)} functions, {len(ra)} / {len(rb)} kernels")
    for title, names in (("only in one build", only), ("code bytes differ", differ), ("resource notes differ", notes)):
        print(f"{title}: {len(names)}")
        for k in names:
            print("   ", k)
    if not (only or differ or notes):
        same_order = list(fa) == list(fb)
        print("every function has the same bytes and every kernel the same notes; " +
              ("the symbol order is the same too" if same_order else "only the order of the functions differs"))
        return 0
    return 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
