"""Device code of a built libmonocon_hip.so, per kernel: prints "<sha256 of the kernel's machine code> <symbol>" for every
gfx950 kernel of every code object in the library's fat binary, sorted by symbol.  Two builds with the same device code
print the same lines (`diff` of the two outputs); needs the ROCm LLVM tools, no GPU.

    python scratch/kernel_symbols.py monocon-pytorch_amd/hipmonocon/libmonocon_hip.so > new.txt
"""
import hashlib, os, struct, subprocess, sys, tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def code_objects(fatbin):
    at = fatbin.find(MAGIC)
    while at >= 0:
        (n,) = struct.unpack_from("<Q", fatbin, at + len(MAGIC))
        p = at + len(MAGIC) + 8
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", fatbin, p)
            triple = fatbin[p + 24:p + 24 + tl].decode()
            p += 24 + tl
            if "gfx950" in triple and size:
                yield fatbin[at + off:at + off + size]
        at = fatbin.find(MAGIC, at + len(MAGIC))


def kernels(elf_bytes, tmp):
    path = os.path.join(tmp, "co.elf")
    open(path, "wb").write(elf_bytes)
    secs = subprocess.run([LLVM + "/llvm-readelf", "-S", "-W", path], capture_output=True, text=True, check=True).stdout
    text = [l.replace("[", " ").replace("]", " ").split() for l in secs.splitlines() if " .text " in l][0]
    t_addr, t_off = int(text[3], 16), int(text[4], 16)
    syms = subprocess.run([LLVM + "/llvm-readelf", "-s", "-W", path], capture_output=True, text=True, check=True).stdout
    funcs, kds = {}, set()
    for l in syms.splitlines():
        f = l.split()
        if len(f) < 8 or not f[0].endswith(":"):
            continue
        if f[3] == "FUNC":
            funcs[f[7]] = (int(f[1], 16), int(f[2]))
        elif f[3] == "OBJECT" and f[7].endswith(".kd"):
            kds.add(f[7][:-3])
    for name in kds:
        addr, size = funcs[name]
        o = t_off + addr - t_addr
        yield name, hashlib.sha256(elf_bytes[o:o + size]).hexdigest()


with tempfile.TemporaryDirectory() as tmp:
    fb = os.path.join(tmp, "fatbin")
    subprocess.run([LLVM + "/llvm-objcopy", "--dump-section", ".hip_fatbin=" + fb, sys.argv[1], os.path.join(tmp, "copy.so")], check=True)
    out = [k for co in code_objects(open(fb, "rb").read()) for k in kernels(co, tmp)]
for name, digest in sorted(out):
    print(digest, name)
