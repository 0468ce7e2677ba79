"""Host side of tests/test_gpu_solve_chain.py (no GPU): the float64 references of the back substitution alpha = L^-T z and of the
inverse K^-1 = L^-T L^-1, and their floors -- how far two host routes to the same quantity disagree on the inputs the GPU tests use
(tests/test_gpu_parity.py::test_potrf_vs_lapack: K = G G' / n + I / 2, condition number about 9).

    DELTA_backsolve: SciPy's solve_triangular (LAPACK dtrtrs) against a longdouble back substitution, relative to max|alpha|
    DELTA_inverse:   (L^-1)' L^-1 from a triangular solve against numpy.linalg.inv(K), relative to max|K^-1|

The GPU tests hold max(1e-10, 100 DELTA); measured at n = 65 / 333 / 1088 / 2112: DELTA_backsolve = 5.9e-16, DELTA_inverse = 2.3e-15,
so they hold 1e-10.  The floors are asserted here at 1e-13, where that rule would begin to move."""
import numpy as np

FLOOR_N = (65, 333, 1088, 2112)


def spd(n, j=0):
    """Matrix j of size n: test_potrf_vs_lapack's K for j = 0 (the same generator), further draws of the same family for j > 0."""
    rng = np.random.default_rng(n if j == 0 else [n, j])
    G = rng.standard_normal((n, n + 8))
    return G @ G.T / n + 0.5 * np.eye(n)


def backsolve_ref(L, Z):
    """alpha = L^-T z for the columns z of Z (n x k), L lower triangular."""
    import scipy.linalg as sla
    return sla.solve_triangular(L.T, Z, lower=False)


def backsolve_longdouble(L, Z):
    Ll, Zl = L.astype(np.longdouble), Z.astype(np.longdouble)
    out = np.zeros_like(Zl)
    for i in range(L.shape[0] - 1, -1, -1):
        out[i] = (Zl[i] - Ll[i + 1:, i] @ out[i + 1:]) / Ll[i, i]
    return out


def inverse_ref(L):
    """(L^-T, (L L')^-1) from one triangular solve."""
    import scipy.linalg as sla
    X = sla.solve_triangular(L, np.eye(L.shape[0]), lower=True)
    return X.T, X.T @ X


_DELTA = {}


def deltas():
    """(DELTA_backsolve, DELTA_inverse), the largest over FLOOR_N."""
    if not _DELTA:
        db = di = 0.0
        for n in FLOOR_N:
            K = spd(n)
            L = np.linalg.cholesky(K)
            Z = np.random.default_rng([n, 3]).standard_normal((n, 3))
            ref = backsolve_longdouble(L, Z)
            db = max(db, float(np.abs(backsolve_ref(L, Z) - ref).max() / np.abs(ref).max()))
            Ki = np.linalg.inv(K)
            di = max(di, float(np.abs(inverse_ref(L)[1] - Ki).max() / np.abs(Ki).max()))
        _DELTA["v"] = (db, di)
    return _DELTA["v"]


def tolerance():
    """The project's rule, max(1e-10, 100 DELTA), for (the back substitution, the inverse)."""
    db, di = deltas()
    return max(1e-10, 100.0 * db), max(1e-10, 100.0 * di)


def test_host_floors():
    db, di = deltas()
    print(f"DELTA_backsolve = {db:.3e}, DELTA_inverse = {di:.3e}")
    assert db <= 1e-13 and di <= 1e-13, (db, di)


def test_references_solve_their_equations():
    """The references themselves: L' alpha = z and K K^-1 = I, to rounding (a reference with lower / upper swapped passes neither)."""
    n = 333
    K = spd(n, 1)
    L = np.linalg.cholesky(K)
    Z = np.random.default_rng(5).standard_normal((n, 2))
    assert np.abs(L.T @ backsolve_ref(L, Z) - Z).max() <= 1e-13 * np.abs(Z).max()
    R, Ki = inverse_ref(L)
    assert np.abs(np.tril(R, -1)).max() == 0.0
    assert np.abs(K @ Ki - np.eye(n)).max() <= 1e-13
