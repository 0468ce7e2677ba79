"""The factorisation driver (plan_potrf + its executor, DESIGN.md "what is launched for a shape") launches what the recursive driver
it replaced launched: tests/golden/potrf_launches_parent.json holds, per environment and scenario, the ordered (class, M, N, K) of the
profiled launches and the per-class launch counts, work and bytes of lmm_profile_end, recorded from that driver with this file's
child mode (`python tests/test_gpu_potrf_plan.py > fixture-part.json` under each environment of ENVS).  work and bytes are host
arithmetic, so the comparison is exact.  The scenarios run in a fresh child process per environment: the switches are read once."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIXTURE = os.path.join(HERE, "golden", "potrf_launches_parent.json")
ENVS = {
    "default": {},
    "panel_recursion_lax": {"LMM_REGION_ALL": "0", "LMM_STRICT_PROGRESS": "0"},
    "round2_path": {"LMM_PANEL128": "0"},
    "deterministic": {"LMM_DETERMINISTIC": "1"},
}
POTRF_SHAPES = [(320, 256), (1088, 1024), (1216, 1152), (1280, 1216)]      # (NR, NC): one 64-row block of riders
EMUL_SHAPE = (2368, 2304)
SWITCHES = ["LMM_PANEL128", "LMM_REGION", "LMM_REGION_ALL", "LMM_REGION_SMALL", "LMM_FUSE_BULK", "LMM_STRIP_ITEMS", "LMM_DETERMINISTIC",
            "LMM_REGION_ASST", "LMM_REGION_OCC", "LMM_REGION_TH", "LMM_REGION_TRACE", "LMM_F64_EMUL", "LMM_F64_EMUL_MINK",
            "LMM_STRICT_PROGRESS", "LMM_BATCH", "LMM_NSTREAMS"]


def spd_problem(NR, NC):
    """(Kmat, rhs, column-major device matrix with ld = NR + 2): NC columns of an SPD matrix and NR - NC rider rows."""
    import torch
    rng = np.random.default_rng(NC)
    G = rng.standard_normal((NC, NC + 8))
    Kmat = G @ G.T / NC + 0.5 * np.eye(NC)
    rhs = rng.standard_normal((NR - NC, NC))
    full = np.zeros((NR, NC))
    full[:NC] = np.tril(Kmat)
    full[NC:] = rhs
    A = torch.zeros(NC, NR + 2, dtype=torch.float64, device="cuda")
    A[:, :NR] = torch.from_numpy(full.T.copy()).cuda()
    return Kmat, rhs, A


def dev_potrf(lib, A, NR, NC):
    import torch
    W = torch.zeros(NC // 64 * 4096, dtype=torch.float64, device="cuda")
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()      # raw pointers cross the ABI: torch's asynchronous producers of these tensors must be done
    rc = lib.lmm_dev_potrf(C.c_void_p(A.data_ptr()), NR, NC, NR + 2, C.c_void_p(W.data_ptr()), NC, C.c_void_p(info.data_ptr()))
    assert rc == 0, lib.lmm_last_error_string()
    assert int(info.item()) == 0


def child():
    """Runs every scenario between lmm_profile_begin(0) and lmm_profile_end; the library writes its [prof] lines to stderr, this
    function a [scenario] line ahead of each, and the per-class totals as one JSON line to stdout."""
    sys.path.insert(0, ROOT)
    import torch
    import lmm_amd
    from lmm_amd import _lib as L
    from lmm_amd.workloads import synthetic_problem
    lib = lmm_amd.load()
    lmm_amd.init(0)
    totals = {}

    def profiled(name, fn):
        sys.stderr.write(f"[scenario] {name}\n"); sys.stderr.flush()
        L.check(lib.lmm_profile_begin(0))
        fn()
        ent = (L.ProfEntryT * len(L.PROF_CLASSES))()
        L.check(lib.lmm_profile_end(ent))
        totals[name] = [[int(e.launches), e.work, e.bytes] for e in ent]

    for NR, NC in POTRF_SHAPES:
        A = spd_problem(NR, NC)[2]
        profiled(f"potrf_{NR}x{NC}", lambda: dev_potrf(lib, A, NR, NC))
    A = spd_problem(*EMUL_SHAPE)[2]
    assert lib.lmm_dev_set_f64_emul(1, 256, 16) == 0
    profiled("potrf_emul_%dx%d" % EMUL_SHAPE, lambda: dev_potrf(lib, A, *EMUL_SHAPE))
    assert lib.lmm_dev_set_f64_emul(-1, 0, 0) == 0
    for m in (3, 34):
        P = synthetic_problem(m, 40, 1152, "matern52", True, seed=2)
        f = lmm_amd.ILMM(lmm_amd.independent_mogp([lmm_amd.GP(lmm_amd.Matern52Kernel()) for _ in range(m)]), lmm_amd.Orthogonal(P["U"], P["S"]))
        fx = f(lmm_amd.MOInputIsotopicByOutputs(P["x"], 40), 0.1)
        profiled(f"logpdf_1152_m{m}", lambda: lmm_amd.logpdf(fx, P["y"]))
    print(json.dumps({"cus": torch.cuda.get_device_properties(0).multi_processor_count, "totals": totals}))


def run_child(env):
    """{"cus", "scenarios": {name: {"launches": [[cls, M, N, K], ...], "totals": [[launches, work, bytes] per class]}}}"""
    base = {k: v for k, v in os.environ.items() if k not in SWITCHES and k != "LMM_PROF_DUMP"}
    out = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(base, LMM_PROF_DUMP="1", **env), capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stderr[-3000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    seqs, cur = {}, None
    for line in out.stderr.splitlines():
        if line.startswith("[scenario] "):
            cur = seqs.setdefault(line.split()[1], [])
        m = re.match(r"\[prof\] cls=(\d+) M=(\d+) N=(\d+) K=(\d+) ", line)
        if m:
            cur.append([int(v) for v in m.groups()])
    return {"cus": res["cus"], "scenarios": {k: {"launches": seqs[k], "totals": res["totals"][k]} for k in res["totals"]}}


@pytest.mark.gpu
@pytest.mark.parametrize("env", list(ENVS))
def test_launch_sequence_equals_the_recursive_drivers(env):
    with open(FIXTURE) as fh:
        want = json.load(fh)["envs"][env]
    got = run_child(ENVS[env])
    assert got["cus"] == want["cus"], "the fixture was recorded on a device with another CU count: the region rule depends on it"
    assert sorted(got["scenarios"]) == sorted(want["scenarios"])
    for name, w in want["scenarios"].items():
        g = got["scenarios"][name]
        assert g["launches"] == w["launches"], (env, name)
        assert g["totals"] == w["totals"], (env, name)      # launches, work, bytes per class: exact


@pytest.mark.gpu
@pytest.mark.parametrize("NR,NC", POTRF_SHAPES + [EMUL_SHAPE])
def test_factors_agree_with_lapack(NR, NC):
    """Every shape of the scenarios, in the default environment (which emulates nothing at these sizes); the tolerances of tests/test_gpu_parity.py::test_potrf_vs_lapack."""
    import scipy.linalg as sla
    import lmm_amd
    lib = lmm_amd.load()
    lmm_amd.init(0)
    Kmat, rhs, A = spd_problem(NR, NC)
    dev_potrf(lib, A, NR, NC)
    got = A[:, :NR].T.cpu().numpy()
    Lref = np.linalg.cholesky(Kmat)
    np.testing.assert_allclose(np.tril(got[:NC]), Lref, rtol=1e-9, atol=1e-11)
    zref = sla.solve_triangular(Lref, rhs.T, lower=True).T
    np.testing.assert_allclose(got[NC:], zref, rtol=1e-8, atol=1e-10)


if __name__ == "__main__":
    child()
