"""Host-only checks of plan_potrf (csrc/lmm_potrf_plan.h) through lmm_dev_potrf_plan and lmm_dev_emul_plan: no GPU,
no lmm_init.

* tests/golden/emul_plan_parent.json holds every word lmm_dev_emul_plan gave before the planner existed (the recursive driver's second
  walk); the planner reproduces it.
* The step list of a grid of shapes, batch sizes, in-flight counts, dtypes and progress modes is replayed on a model of the 64 x 64
  blocks of the matrix (check_replay): every block is factored / solved once, with exactly its updates applied before.
* The decision table of DESIGN.md 4.19, the place of the ragged last 64 rows included; the odd leading dimension, which the hook has
  no argument for, through the stand-alone tests/c/potrf_plan_check.cpp.
* The steps the profile names are the launches tests/golden/potrf_launches_parent.json recorded from the recursive driver on a GPU.

The environment switches are read once per process, so everything that depends on them runs in a child process per setting
(`python tests/test_potrf_plan_host.py <setting>`); the settings are those of tests/test_gpu_parity_r2.py::test_update_kernel_variants_agree
and of tests/test_gpu_potrf_plan.py."""
import ctypes as C
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER, STEP, CAP = 8, 14, 1024
KINDS = ["diag64", "solve64", "update", "leaf128", "bulk", "update_leaf", "emul_update_leaf", "region"]
EMUL_SHAPES = [(16448, 16384), (8256, 8192), (4160, 4096), (2112, 2048), (2368, 2304), (1216, 1152), (2304, 2304)]
GRID_SHAPES = EMUL_SHAPES + [(320, 256), (1088, 1024), (1280, 1216), (192, 192)]
SETTINGS = {
    "default": {}, "round2_path": {"LMM_PANEL128": "0"}, "deterministic": {"LMM_DETERMINISTIC": "1"},
    "round2_deterministic": {"LMM_PANEL128": "0", "LMM_DETERMINISTIC": "1"}, "no_fused_bulk": {"LMM_FUSE_BULK": "0"},
    "region_base_512": {"LMM_REGION_ALL": "1", "LMM_REGION": "512"}, "region_no_assistants": {"LMM_REGION_ASST": "0"},
    "region_occ2": {"LMM_REGION_OCC": "2"}, "panel_recursion": {"LMM_REGION_ALL": "0"},
    "panel_recursion_deterministic": {"LMM_REGION_ALL": "0", "LMM_DETERMINISTIC": "1"},
    "panel_recursion_lax": {"LMM_REGION_ALL": "0", "LMM_STRICT_PROGRESS": "0"},      # strict progress is an argument of the plan, not a switch it reads
    "strip_separate": {"LMM_STRIP_ITEMS": "0"}, "strip_in_launch": {"LMM_STRIP_ITEMS": "2"},
}


def load():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import lmm_amd
    lib = lmm_amd.load()
    lib.lmm_dev_potrf_plan.argtypes = [C.c_int] * 8 + [C.POINTER(C.c_longlong), C.c_int]
    lib.lmm_dev_potrf_plan.restype = C.c_int
    lib.lmm_dev_emul_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_longlong), C.c_int]
    lib.lmm_dev_emul_plan.restype = C.c_int
    lib.lmm_dev_set_f64_emul_rule.argtypes = [C.c_int, C.c_int, C.c_double]
    return lib


def reset(lib):
    assert lib.lmm_dev_set_f64_emul(-1, 0, 0) == 0 and lib.lmm_dev_set_f64_emul_rule(-1, 0, 0.0) == 0 and lib.lmm_dev_set_emul_group(0) == 0


def as_double(word):
    return struct.unpack("<d", struct.pack("<q", word))[0]


def plan(lib, NR, NC, nb, rows_real=-1, in_flight=1, cus=256, f32=0, strict=1):
    """(header dict, [step dict, ...]) of lmm_dev_potrf_plan (layout: include/lmm_hip.h)"""
    out = (C.c_longlong * (HEADER + STEP * CAP))()
    n = lib.lmm_dev_potrf_plan(NR, NC, nb, rows_real, in_flight, cus, f32, strict, out, CAP)
    assert 0 <= n <= CAP, (n, lib.lmm_last_error_string())
    head = dict(zip(["panel128", "region_cols", "w2", "node_flags", "asst", "emul_bytes", "emul_G", "nmod"], out[:HEADER]))
    steps = []
    for i in range(n):
        r = out[HEADER + STEP * i: HEADER + STEP * (i + 1)]
        steps.append(dict(kind=KINDS[r[0]], j0=r[1], h=r[2], N=r[3], M=r[4], cls=r[5], named=r[6], work=as_double(r[7]), bytes=as_double(r[8]),
                          first_done=r[9], fused_bulk=r[10], strip=r[11], group=r[12], scratch=r[13]))
    return head, steps


def split(w):
    if w >= 256:
        return (w // 2 + 127) // 128 * 128
    return 128 if w == 192 else 64


def recursion_updates(NR, j0, w, panel128, region_cols, out):
    """(j0, K, N, M) of the trailing updates of the split() recursion over [j0, j0 + w) that are launches of their own: on the panel
    path a 128-column panel is a leaf, and so is a block column the region kernel takes"""
    if w <= 64 or (panel128 and (w == 128 or (w <= region_cols and w % 128 == 0))):
        return out
    h = split(w)
    recursion_updates(NR, j0, h, panel128, region_cols, out)
    out.append((j0, h, w - h, NR - j0 - h))
    return recursion_updates(NR, j0 + h, w - h, panel128, region_cols, out)


def check_replay(NR, NC, head, steps):
    """The steps on the 64 x 64 blocks (r, c), r >= c, of an NR x NC matrix.  done[r, c]: source block columns applied to the block so
    far -- updates reach a block in increasing order of their sources, so a count says which; a block is final when done == c and it
    is factored (r == c) or solved (r > c)."""
    R, Cb = NR // 64, NC // 64
    low = np.tril(np.ones((R, Cb), dtype=bool))
    done = np.zeros((R, Cb), dtype=np.int64)
    final = np.zeros((R, Cb), dtype=bool)      # factored (diagonal) / solved (below it)

    def square(c0, c1):          # factor the diagonal square of the block columns [c0, c1): nothing of it final, all outer updates in
        sq = (slice(c0, c1), slice(c0, c1))
        assert not final[sq][low[sq]].any() and (done[sq][low[sq]] == c0).all()
        done[sq] = np.arange(c0, c1)[None, :]
        final[sq] = low[sq]

    def below(c0, c1):           # solve the rows below that square
        assert final[c0:c1, c0:c1][low[c0:c1, c0:c1]].all()
        assert not final[c1:, c0:c1].any() and (done[c1:, c0:c1] == c0).all()
        done[c1:, c0:c1] = np.arange(c0, c1)[None, :]
        final[c1:, c0:c1] = True

    def update(s):
        k0, k1, c0 = s["j0"] // 64, (s["j0"] + s["h"]) // 64, (s["j0"] + s["h"]) // 64
        c1 = c0 + s["N"] // 64
        assert s["M"] == NR - 64 * c0 and s["M"] >= s["N"]
        assert final[k0:, k0:k1][low[k0:, k0:k1]].all()                    # its operands are final
        tgt = (slice(c0, R), slice(c0, c1))
        assert not final[tgt].any() and (done[tgt][low[tgt]] == k0).all()   # applied before the block is factored or solved, once, in order
        done[tgt] = np.where(low[tgt], k1, done[tgt])

    for s in steps:
        c, k = s["j0"] // 64, s["kind"]
        if k == "diag64":
            square(c, c + 1)
        elif k == "solve64":
            assert s["M"] == NR - s["j0"] - 64
            below(c, c + 1)
        elif k == "update":
            update(s)
        elif k == "leaf128":
            square(c, c + 2)
        elif k == "bulk":
            assert s["M"] == NR - s["j0"] - 128
            below(c, c + 2)
        elif k in ("update_leaf", "emul_update_leaf"):
            update(s)
            c1 = (s["j0"] + s["h"]) // 64
            square(c1, c1 + 2)
            if s["fused_bulk"]:
                assert k == "update_leaf" and head["node_flags"] > 0 and R > c1 + 2
                below(c1, c1 + 2)
            if k == "emul_update_leaf":
                assert 1 <= s["group"] and 0 < s["scratch"] <= head["emul_bytes"]
        elif k == "region":      # its whole block column
            assert head["region_cols"] >= s["N"] and s["N"] % 128 == 0 and s["M"] == NR - s["j0"]
            c1 = c + s["N"] // 64
            if s["first_done"]:
                assert final[c:c + 2, c:c + 2][low[:2, :2]].all() and not final[c + 2:, c:c + 2].any()
                final[c:c + 2, c:c + 2] = False
                done[c:c + 2, c:c + 2] = c
            square(c, c1)
            below(c, c1)
    assert final[low].all() and (done[low] == np.broadcast_to(np.arange(Cb), (R, Cb))[low]).all()
    got = [(s["j0"], s["h"], s["N"], s["M"]) for s in steps if "update" in s["kind"]]
    assert got == recursion_updates(NR, 0, NC, head["panel128"], head["region_cols"], [])


def check_grid(lib, setting):
    for NR, NC in GRID_SHAPES:
        for nb in (1, 3, 16, 32):
            for in_flight in (1, 2, 4):
                for f32 in (0, 1):
                    for strict in (0, 1):
                        head, steps = plan(lib, NR, NC, nb, NC + 1 if NR > NC else -1, in_flight, 256, f32, strict)
                        try:
                            check_replay(NR, NC, head, steps)
                        except AssertionError:
                            print("replay failed:", setting, (NR, NC, nb, in_flight, f32, strict), head, file=sys.stderr)
                            raise
                        if strict:
                            assert not any(s["fused_bulk"] for s in steps)


def named(steps):
    return [[s["cls"], s["M"], s["N"], s["h"]] for s in steps if s["named"]]


def check_fixture(lib, setting):
    """The launches the recursive driver made on a GPU (recorded CU count and in-flight counts) are the plan's named steps, and the
    work / bytes / launch totals of the factorisation's profile classes are the steps' sums."""
    with open(os.path.join(HERE, "golden", "potrf_launches_parent.json")) as fh:
        fx = json.load(fh)
    if setting not in fx["envs"]:
        return
    env, strict = fx["envs"][setting], 0 if setting == "panel_recursion_lax" else 1
    for name, rec in env["scenarios"].items():
        emul = name.startswith("potrf_emul")
        if emul:
            assert lib.lmm_dev_set_f64_emul(1, 256, 16) == 0
        steps = []
        for NR, NC, nb, rows_real in fx["plans"][name]:
            steps += plan(lib, NR, NC, nb, rows_real, fx["in_flight"][name], env["cus"], 0, strict)[1]
        reset(lib)
        assert named(steps) == [r for r in rec["launches"] if 1 <= r[0] <= 6], (setting, name)
        for cls in range(1, 7):
            mine = [s for s in steps if s["cls"] == cls]
            work = bytes_ = 0.0
            for s in mine:      # in launch order, as lmm_profile_end adds them: equality is exact
                work += s["work"]; bytes_ += s["bytes"]
            assert [len(mine), work, bytes_] == rec["totals"][cls], (setting, name, cls)


def check_decision_table(lib, setting):
    """DESIGN.md 4.19, default switches, 256 CUs."""
    def kinds(steps):
        return [s["kind"] for s in steps]
    # The ragged last 64 rows of (2368, 2304)'s K = 1152 update (M = 1216 = 9.5 row tiles): items of the launch while the batch runs
    # alone, a launch of their own beside another batch; LMM_STRIP_ITEMS=0: always their own launch, 2: always items.  No other step has any.
    strip_want = {"default": (1, 2), "strip_separate": (2, 2), "strip_in_launch": (1, 1)}
    if setting in strip_want:
        for in_flight, want in zip((1, 2), strip_want[setting]):
            head, steps = plan(lib, 2368, 2304, 1, 2305, in_flight)
            assert [(s["kind"], s["h"], s["N"], s["M"], s["strip"]) for s in steps if s["strip"]] == [("update_leaf", 1152, 1152, 1216, want)], (setting, in_flight)
        head, steps = plan(lib, 2304, 2304, 1)       # M = 1152: whole tiles
        assert not any(s["strip"] for s in steps)
    if setting == "default":
        # the 64-column path: Float32, or fewer than 128 columns (LMM_PANEL128=0: round2_path below; an odd leading dimension is not an
        # argument of the hook: test_plan_check_program pins it on plan_potrf itself)
        for args in [(4160, 4096, 8, -1, 1, 256, 1, 1), (64, 64, 8, -1, 1, 256, 0, 1), (16448, 16384, 16, -1, 1, 256, 1, 1)]:
            head, steps = plan(lib, *args)
            assert head["panel128"] == 0 and head["region_cols"] == 0 and head["emul_bytes"] == 0 and head["w2"] == 0
            assert set(kinds(steps)) <= {"diag64", "solve64", "update"}
        for nb in (1, 3, 16, 32):
            head, steps = plan(lib, 1088, 1024, nb)
            assert kinds(steps) == ["region"] and steps[0]["first_done"] == 0 and (steps[0]["j0"], steps[0]["N"]) == (0, 1024)
        head, steps = plan(lib, 1216, 1152, 3, 1153, 1)
        assert [(s["kind"], s["j0"], s["N"], s["first_done"]) for s in steps] == [("region", 0, 640, 0), ("update_leaf", 0, 512, 0), ("region", 640, 512, 1)]
        assert (steps[1]["h"], steps[1]["fused_bulk"]) == (640, 0)
        assert plan(lib, 1216, 1152, 32, 1153, 2)[0]["region_cols"] == 512
        head, steps = plan(lib, 1280, 1216, 1)
        assert head["region_cols"] == 0 and "region" not in kinds(steps) and kinds(steps)[-3:] == ["update", "diag64", "solve64"]
        head, steps = plan(lib, 16448, 16384, 16, 16385, 2)
        assert head["region_cols"] == 512
        ups = [s for s in steps if "update" in s["kind"]]
        assert [s["h"] for s in ups if s["h"] >= 4096] == [4096, 8192, 4096]
        for s in ups:
            assert (s["kind"] == "emul_update_leaf") == (s["h"] >= 4096 or (s["h"] == 2048 and s["M"] >= 6208)), s
        assert plan(lib, 16448, 16384, 4, 16385, 1)[0]["region_cols"] == 1024
    if setting in ("round2_path", "round2_deterministic"):
        head, steps = plan(lib, 4160, 4096, 8)
        assert head["panel128"] == 0 and head["region_cols"] == 0 and set(kinds(steps)) <= {"diag64", "solve64", "update"}
    if setting == "panel_recursion_lax":      # region "never" at NC > 1024
        for NR, NC, nb in [(2368, 2304, 2), (4160, 4096, 8), (8256, 8192, 4)]:
            for strict in (0, 1):
                head, steps = plan(lib, NR, NC, nb, NC + 1, 1, 256, 0, strict)
                assert head["region_cols"] == 0
                ups = [s for s in steps if s["kind"] == "update_leaf"]
                assert ups
                for s in ups:
                    want = strict == 0 and 512 <= s["h"] <= 2048 and s["N"] >= 128 and (s["M"] + 127) // 128 > 1
                    assert s["fused_bulk"] == int(want), s


def child(setting):
    lib = load()
    reset(lib)
    check_decision_table(lib, setting)
    check_fixture(lib, setting)
    check_grid(lib, setting)
    print("ok")


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_plan_in_a_fresh_process(setting):
    """Decision table, GPU fixture and block-state replay of the grid under one setting of the environment switches."""
    drop = {k for v in SETTINGS.values() for k in v} | {"LMM_REGION_SMALL", "LMM_STRIP_ITEMS", "LMM_REGION_TH", "LMM_REGION_TRACE", "LMM_F64_EMUL", "LMM_F64_EMUL_MINK"}
    env = {k: v for k, v in os.environ.items() if k not in drop}
    out = subprocess.run([sys.executable, os.path.abspath(__file__), setting], env=dict(env, **SETTINGS[setting]), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr[-3000:]


def test_emul_plan_is_the_recursive_drivers():
    lib = load()
    with open(os.path.join(HERE, "golden", "emul_plan_parent.json")) as fh:
        golden = json.load(fh)
    count = 0
    try:
        for setting in ("default", "rule_512_256_2e5", "mink_256"):
            reset(lib)
            if setting == "rule_512_256_2e5":
                assert lib.lmm_dev_set_f64_emul_rule(512, 256, 2.0e5) == 0
            if setting == "mink_256":
                assert lib.lmm_dev_set_f64_emul(1, 256, 16) == 0
            for NR, NC in EMUL_SHAPES:
                for nb in (1, 3, 4, 16, 32):
                    out = (C.c_longlong * (2 + 6 * 512))()
                    n = lib.lmm_dev_emul_plan(NR, NC, nb, out, 512)
                    assert 0 <= n <= 512
                    assert list(out[:2 + 6 * n]) == golden[f"{setting}/{NR}x{NC}/{nb}"], (setting, NR, NC, nb)
                    count += 1
    finally:
        reset(lib)
    assert count == len(golden) == 105


def test_bad_arguments():
    lib = load()
    out = (C.c_longlong * (HEADER + STEP))()
    from lmm_amd import _lib as L
    assert lib.lmm_dev_potrf_plan(4160, 4096, 0, -1, 1, 256, 0, 1, out, 1) == -L.LMM_ERR_ARG
    assert lib.lmm_dev_potrf_plan(4000, 4096, 8, -1, 1, 256, 0, 1, out, 1) == -L.LMM_ERR_ARG
    assert lib.lmm_dev_potrf_plan(4160, 4096, 8, -1, 0, 256, 0, 1, out, 1) == -L.LMM_ERR_ARG
    for rows_real in (-2, 0, 4095, 4161):       # rows that hold data: -1 (all), or NC .. NR
        assert lib.lmm_dev_potrf_plan(4160, 4096, 8, rows_real, 1, 256, 0, 1, out, 1) == -L.LMM_ERR_ARG
    assert lib.lmm_dev_potrf_plan(4160, 4096, 8, 4096, 1, 256, 0, 1, out, 1) > 1
    assert lib.lmm_dev_potrf_plan(4160, 4096, 8, -1, 1, 256, 0, 1, out, 1) > 1      # counted beyond cap, not written


def test_plan_check_program(tmp_path):
    """tests/c/potrf_plan_check.cpp calls plan_potrf itself (the header compiles without HIP), so it also reaches the one input the
    hook does not pass on: an odd leading dimension gives the 64-column path, no region, no scratch and nothing emulated."""
    exe = str(tmp_path / "potrf_plan_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "linearmixingmodels.jl_amd", "csrc"),
                           os.path.join(HERE, "c", "potrf_plan_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith(" 0 failures"), out.stdout[-500:] + out.stderr[-3000:]


def test_scratch_check_program(tmp_path):
    """tests/c/potrf_scratch_check.cpp: the plan's scratch sizes, covers, vote and listeners equal what the executor derived from the
    step list while it sized its own scratch, on the whole grid; batch_plan's per-stream term is its former expression; and each of
    the seven extent invariants of plan_potrf_check fails, naming its step, on a plan edited to violate exactly that one."""
    exe = str(tmp_path / "potrf_scratch_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "linearmixingmodels.jl_amd", "csrc"),
                           os.path.join(HERE, "c", "potrf_scratch_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith(" 0 failures"), out.stdout[-500:] + out.stderr[-3000:]


if __name__ == "__main__":
    child(sys.argv[1])
