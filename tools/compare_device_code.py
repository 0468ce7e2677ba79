"""Device code of two builds of liblmm_hip.so, kernel by kernel: extracts the gfx950 code objects of both from the offload bundles in .hip_fatbin, reads every
function symbol's bytes out of .text (llvm-readelf -sW / -SW) and reports, per kernel name, whether the two builds hold the same bytes.
Usage: python tools/compare_device_code.py OLD.so NEW.so   (host only; needs ROCm's object tools)"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def code_objects(so, tmp, tag):
    """The gfx950 entries of the clang offload bundles in the library's .hip_fatbin section (one bundle per translation unit)"""
    readelf = os.path.join(ROCM, "lib", "llvm", "bin", "llvm-readelf")
    sec = re.search(r"\.hip_fatbin\s+PROGBITS\s+[0-9a-f]+\s+([0-9a-f]+)\s+([0-9a-f]+)", subprocess.run([readelf, "-SW", so], capture_output=True, text=True, check=True).stdout)
    data = open(so, "rb").read()[int(sec.group(1), 16):][:int(sec.group(2), 16)]
    magic, paths, at = b"__CLANG_OFFLOAD_BUNDLE__", [], 0
    assert data.startswith(magic), "not an uncompressed offload bundle"
    while (at := data.find(magic, at)) >= 0:
        n, q = int.from_bytes(data[at + 24: at + 32], "little"), at + 32
        for _ in range(n):
            off, size, tl = (int.from_bytes(data[q + 8 * i: q + 8 * i + 8], "little") for i in range(3))
            triple = data[q + 24: q + 24 + tl].decode()
            q += 24 + tl
            if "gfx950" in triple and size:
                path = os.path.join(tmp, f"{tag}_{len(paths)}.co")
                with open(path, "wb") as oh:
                    oh.write(data[at + off: at + off + size])
                paths.append(path)
        at += 24
    return paths


def kernels(co):
    """{symbol: sha1 of its bytes} for the FUNC symbols of .text, + the kernel descriptors (.rodata objects named *.kd)"""
    readelf = os.path.join(ROCM, "lib", "llvm", "bin", "llvm-readelf")
    secs = {}
    for line in subprocess.run([readelf, "-SW", co], capture_output=True, text=True, check=True).stdout.splitlines():
        m = re.match(r"\s*\[\s*(\d+)\]\s+(\S+)\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", line)
        if m:
            secs[int(m.group(1))] = (int(m.group(3), 16), int(m.group(4), 16))      # address, file offset
    data = open(co, "rb").read()
    res = {}
    for line in subprocess.run([readelf, "-sW", co], capture_output=True, text=True, check=True).stdout.splitlines():
        f = line.split()
        if len(f) == 8 and f[3] in ("FUNC", "OBJECT") and f[6].isdigit():
            addr, size, sec = int(f[1], 16), int(f[2]), secs[int(f[6])]
            if f[3] == "OBJECT" and not f[7].endswith(".kd"):
                continue
            res[f[7]] = hashlib.sha1(data[sec[1] + addr - sec[0]: sec[1] + addr - sec[0] + size]).hexdigest() + f" {size}"
    return res


def main(old, new):
    with tempfile.TemporaryDirectory() as tmp:
        a, b = {}, {}
        for so, tag, into in ((old, "old", a), (new, "new", b)):
            cos = code_objects(so, tmp, tag)
            print(f"{tag}: {so}: {len(cos)} gfx950 code objects")
            for co in cos:
                into.update(kernels(co))
    same = [k for k in a if k in b and a[k] == b[k]]
    differ = [k for k in a if k in b and a[k] != b[k]]
    print(f"{len(a)} symbols in old, {len(b)} in new: {len(same)} byte-identical, {len(differ)} differ, "
          f"{len(set(a) - set(b))} only in old, {len(set(b) - set(a))} only in new")
    for k in differ:
        print("DIFFERS", k, a[k], "->", b[k])
    for k in sorted(set(a) - set(b)):
        print("ONLY OLD", k)
    for k in sorted(set(b) - set(a)):
        print("ONLY NEW", k)
    return 1 if differ or set(a) != set(b) else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
