"""Device code of two builds of liblmm_hip.so, kernel by kernel: extracts the gfx950 code objects of both from the offload bundles in .hip_fatbin, reads every
function symbol's bytes out of .text (llvm-readelf -sW / -SW) and reports, per kernel name, whether the two builds hold the same bytes.
A kernel descriptor (*.kd) is compared without its kernel_code_entry_byte_offset (bytes 16 .. 23), which only says where in .text the code landed.
--pair REGEX=REPL (repeatable): a kernel of OLD whose name matches REGEX is compared with the kernel of NEW named re.sub(REGEX, REPL, name): for kernels
that were renamed or merged.  Where the code of a kernel differs, its VGPR / AGPR / SGPR counts, spills, scratch and LDS bytes of both builds (the code
objects' metadata notes) are printed.  Exit status: 0 when every kernel has a partner with the same bytes, 1 when some bytes differ or a kernel has no
partner, 2 when a resource figure differs as well.
Usage: python tools/compare_device_code.py OLD.so NEW.so [--pair REGEX=REPL ...]   (host only; needs ROCm's object tools)"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
READELF = os.path.join(ROCM, "lib", "llvm", "bin", "llvm-readelf")
RESOURCES = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")


def code_objects(so, tmp, tag):
    """The gfx950 entries of the clang offload bundles in the library's .hip_fatbin section (one bundle per translation unit)"""
    sec = re.search(r"\.hip_fatbin\s+PROGBITS\s+[0-9a-f]+\s+([0-9a-f]+)\s+([0-9a-f]+)", subprocess.run([READELF, "-SW", so], capture_output=True, text=True, check=True).stdout)
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
    secs = {}
    for line in subprocess.run([READELF, "-SW", co], capture_output=True, text=True, check=True).stdout.splitlines():
        m = re.match(r"\s*\[\s*(\d+)\]\s+(\S+)\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", line)
        if m:
            secs[int(m.group(1))] = (int(m.group(3), 16), int(m.group(4), 16))      # address, file offset
    data = open(co, "rb").read()
    res = {}
    for line in subprocess.run([READELF, "-sW", co], capture_output=True, text=True, check=True).stdout.splitlines():
        f = line.split()
        if len(f) == 8 and f[3] in ("FUNC", "OBJECT") and f[6].isdigit():
            addr, size, sec = int(f[1], 16), int(f[2]), secs[int(f[6])]
            if f[3] == "OBJECT" and not f[7].endswith(".kd"):
                continue
            raw = data[sec[1] + addr - sec[0]: sec[1] + addr - sec[0] + size]
            if f[3] == "OBJECT":
                raw = raw[:16] + bytes(8) + raw[24:]
            res[f[7]] = hashlib.sha1(raw).hexdigest() + f" {size}"
    return res


def resources(co):
    """{kernel name: {resource: value}} from the code object's metadata notes"""
    res, cur = {}, None
    for line in subprocess.run([READELF, "--notes", co], capture_output=True, text=True, check=True).stdout.splitlines():
        m = re.match(r"\s+(- )?\.(\w+):\s*(\S*)", line)
        if not m:
            continue
        if m.group(1) and m.group(2) == "agpr_count":
            cur = {}
        if cur is not None and m.group(2) in RESOURCES:
            cur[m.group(2)] = int(m.group(3))
        if cur is not None and m.group(2) == "name":
            res[m.group(3)] = cur
    return res


def main(old, new, pairs):
    with tempfile.TemporaryDirectory() as tmp:
        a, b, ra, rb = {}, {}, {}, {}
        for so, tag, into, rinto in ((old, "old", a, ra), (new, "new", b, rb)):
            cos = code_objects(so, tmp, tag)
            print(f"{tag}: {so}: {len(cos)} gfx950 code objects")
            for co in cos:
                into.update(kernels(co))
                rinto.update(resources(co))
    partner = {}
    for k in a:
        for rx, repl in pairs:
            if k not in b and re.search(rx, k) and re.sub(rx, repl, k) in b:
                partner[k] = re.sub(rx, repl, k)
    both = [(k, k) for k in a if k in b] + sorted(partner.items())
    same = [k for k, k2 in both if a[k] == b[k2]]
    differ = [(k, k2) for k, k2 in both if a[k] != b[k2]]
    only_old, only_new = sorted(set(a) - set(b) - set(partner)), sorted(set(b) - set(a) - set(partner.values()))
    print(f"{len(a)} symbols in old, {len(b)} in new: {len(same)} byte-identical ({sum(k in partner for k in same)} of them paired by --pair), "
          f"{len(differ)} differ, {len(only_old)} only in old, {len(only_new)} only in new")
    for k, k2 in sorted(partner.items()):
        print("PAIRED", k, "->", k2, "identical" if a[k] == b[k2] else "DIFFERS")
    bad = 0
    for k, k2 in differ:
        print("DIFFERS", k, a[k], "->", k2 if k2 != k else "", b[k2])
        o, n = ra.get(k.removesuffix(".kd"), {}), rb.get(k2.removesuffix(".kd"), {})
        moved = [r for r in RESOURCES if o.get(r) != n.get(r)]
        print("   ", " ".join(f"{r}={o.get(r)}" + ("" if r not in moved else f"->{n.get(r)}") for r in RESOURCES), "RESOURCES DIFFER" if moved else "resources equal")
        bad = 2 if moved else bad
    for k in only_old:
        print("ONLY OLD", k)
    for k in only_new:
        print("ONLY NEW", k)
    return bad or (1 if differ or only_old or only_new else 0)


if __name__ == "__main__":
    args, pairs = [], []
    it = iter(sys.argv[1:])
    for x in it:
        if x == "--pair":
            pairs.append(tuple(next(it).split("=", 1)))
        else:
            args.append(x)
    sys.exit(main(args[0], args[1], pairs))
