"""Resource figures of every gfx950 kernel of a build of liblmm_hip.so (or of any shared library holding offload bundles), one line per kernel,
sorted by demangled name: VGPRs, AGPRs, SGPRs, spills, scratch (private segment) and LDS (group segment) bytes, read from the code objects'
metadata notes with the helpers of tools/compare_device_code.py.  --match REGEX keeps the kernels whose demangled name matches.
Usage: python tools/device_code_resources.py LIB.so [--match REGEX]   (host only; needs ROCm's object tools)"""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from compare_device_code import RESOURCES, ROCM, code_objects, resources  # noqa: E402

CXXFILT = shutil.which("llvm-cxxfilt", path=os.path.join(ROCM, "lib", "llvm", "bin")) or shutil.which("c++filt") or "cat"      # cat: mangled names


def main(so, match):
    with tempfile.TemporaryDirectory() as tmp:
        res = {}
        for co in code_objects(so, tmp, "lib"):
            res.update(resources(co))
    names = sorted(res)
    plain = subprocess.run([CXXFILT], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    for name, full in sorted(zip(plain, names)):
        name = re.sub(r"^void \(anonymous namespace\)::", "", name)
        if match and not re.search(match, name):
            continue
        print(" ".join(f"{r}={res[full].get(r)}" for r in RESOURCES), name)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description="resource figures of the gfx950 kernels of a shared library")
    ap.add_argument("library")
    ap.add_argument("--match", default=None, help="keep the kernels whose demangled name matches this regular expression")
    a = ap.parse_args()
    main(a.library, a.match)
