"""Host-only check of emul_amax_cover (csrc/lmm_potrf_plan.h): which kept row-maximum arrays an emulated update of a
factorisation reads instead of scanning its panel again.  The function is plain C++ over the plan's step list, so the check is the
stand-alone tests/c/emul_cover_check.cpp (the header compiles without HIP): for shapes with even and uneven halves and several switch
settings the kept ranges plus the scanned range tile every emulated panel exactly, every kept array comes from an earlier emulated step
inside the panel, and C2's chains are the documented ones.  No GPU, no lmm_init."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_kept_ranges_tile_every_emulated_panel(tmp_path):
    exe = str(tmp_path / "emul_cover_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "linearmixingmodels.jl_amd", "csrc"),
                           os.path.join(HERE, "c", "emul_cover_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout.strip())
    assert out.returncode == 0 and out.stdout.strip().endswith(" 0 failures"), out.stdout[-500:] + out.stderr[-3000:]
    words = out.stdout.split()
    assert int(words[0]) > 1000 and int(words[3]) > 500      # emulated updates seen, and those that read kept maxima
