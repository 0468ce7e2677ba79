"""Host-only check of the index arithmetic behind the int8 emulation's screen (csrc/lmm_emul.h, DESIGN.md 4.17 "negligible tiles"):
the ordered compaction of the GEMM's work ids into the live id list, the layout of the screen's block, and the GEMM's ranges over a
list of any length, the empty one included.  tests/c/emul_screen_check.cpp is the check; this builds and runs it.  No GPU."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_stand_alone_program(tmp_path):
    exe = str(tmp_path / "emul_screen_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "linearmixingmodels.jl_amd", "csrc"),
                           os.path.join(HERE, "c", "emul_screen_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout.strip())
    assert out.returncode == 0 and out.stdout.strip().endswith(" 0 failures"), out.stdout[-500:] + out.stderr[-3000:]
    assert int(out.stdout.split()[0]) > 1000000
