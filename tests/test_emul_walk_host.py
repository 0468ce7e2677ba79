"""Host-only check of two index helpers of the int8 emulation (csrc/lmm_emul.h): the work-id ranges of the GEMM's
walk tile [0, nids) exactly for every grid, and the words of the unwritten-piece bitmap ("dead blocks are never written") stay inside
the bytes set aside for them beside the live masks.  tests/c/emul_walk_check.cpp is the check; this builds and runs it.  No GPU."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_stand_alone_program(tmp_path):
    exe = str(tmp_path / "emul_walk_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "linearmixingmodels.jl_amd", "csrc"),
                           os.path.join(HERE, "c", "emul_walk_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout.strip())
    assert out.returncode == 0 and out.stdout.strip().endswith(" 0 failures"), out.stdout[-500:] + out.stderr[-3000:]
    assert int(out.stdout.split()[0]) > 1000000
