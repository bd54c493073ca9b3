"""CPU suite of bsm_svds (no GPU): the one-sided Jacobi SVD of the projected matrix (csrc/bsm_svds.h, hook
bsm_debug_svds_jacobi) against numpy.linalg.svd; the selection and keep rules and the restart bookkeeping (hooks
bsm_debug_svds_select / _keep / _cycles) against the twin's own copies; the premises of the 600 x 400 problem; the numpy twin
of the solve (tests/_svds.py) against svd of the matrix as stored, for A and adjoint(A), both `which`, every type and the
cases test_gpu_svds.py runs, with the twin's cycle counts pinned -- and the library's bookkeeping and Jacobi SVD on the
bidiagonal matrix every one of these runs produces in its first cycle, against LAPACK --; the stand-alone host check
(tools/svds_host_check.cpp) built and run under AddressSanitizer / UBSan; the exported constants and struct layouts; the
refusals that need no device.  Every test but test_the_problem_meets_its_premises, which is about the test problem alone,
calls the library's new entry points or builds the new host check, and fails without the feature."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from _eigsh import keep_of
from _svds import (CASES, DTYPES, HIGH, LM, LOW, M600, MAX_NCV, N400, SIDES, SM, check_triplets, raw_cycles, raw_keep, raw_select,
                   raw_svd_jacobi, select, stored_singular_values, svd_dense, svd_rtol, svds_twin, twin_of)
from _lsqr import Dense

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = float(np.finfo(np.float64).eps)
name = lambda d: np.dtype(d).name  # noqa: E731


def arrow_bidiagonal(m, rng, keep=None):
    """the shape of Bp after a restart: diag(sigma) with the arrow in column `keep`, upper bidiagonal behind it"""
    keep = m // 3 if keep is None else keep
    B = np.zeros((m, m))
    B[np.arange(m), np.arange(m)] = rng.uniform(0.1, 6, m)
    for i in range(keep):
        B[i, keep] = rng.uniform(-1, 1) * 10.0 ** rng.integers(-12, 1)
    for j in range(keep, m - 1):
        B[j, j + 1] = rng.uniform(0.1, 2)
    return B


def check_jacobi(B, what):
    """|sigma - ref| <= m eps sigma_max against LAPACK; X, Y orthonormal to 4 x 2 m^1.5 eps (the bound of tests/_eigh.py on the
    Jacobi eigenvectors, the margin 4 of its acceptance); B Y = X diag(sigma) to m eps sigma_max per entry; the same bytes twice"""
    m = len(B)
    sigma, X, Y, sweeps = raw_svd_jacobi(B)
    ref = np.linalg.svd(B, compute_uv=False)
    smax = max(ref[0], np.finfo(np.float64).tiny)
    orth = max(np.linalg.norm(X.T @ X - np.eye(m)), np.linalg.norm(Y.T @ Y - np.eye(m)))
    print(f"SVDSTAT jacobi {what} m {m}: {sweeps} sweeps, max |sigma - ref| / (m eps smax) {np.max(np.abs(sigma - ref)) / (m * EPS * smax):.3f}, "
          f"orth / (2 m^1.5 eps) {orth / (2 * m ** 1.5 * EPS):.3f}, max |B Y - X sigma| / (m eps smax) {np.max(np.abs(B @ Y - X * sigma)) / (m * EPS * smax):.3f}")
    assert 0 <= sweeps < 60
    assert np.all(np.diff(sigma) <= 0) and np.all(sigma >= 0)
    assert np.max(np.abs(sigma - ref)) <= m * EPS * smax
    assert orth <= 4 * 2 * m ** 1.5 * EPS
    assert np.max(np.abs(B @ Y - X * sigma)) <= m * EPS * smax
    again = raw_svd_jacobi(B)
    assert all(a.tobytes() == b.tobytes() for a, b in zip((sigma, X, Y), again[:3]))
    return sigma, X, Y


@pytest.mark.parametrize("m", [1, 2, 3, 12, 128])
def test_jacobi_hook_against_lapack(bsm, m):
    check_jacobi(arrow_bidiagonal(m, np.random.default_rng(700 + m)), "arrow")
    check_jacobi(arrow_bidiagonal(m, np.random.default_rng(800 + m), keep=0), "bidiagonal")


def test_jacobi_hook_on_a_zero_column_and_a_double_singular_value(bsm):
    B = arrow_bidiagonal(12, np.random.default_rng(5))
    B[:, 7] = 0  # an exactly zero column: sigma_min = 0, the X column is completed
    sigma, X, Y = check_jacobi(B, "zero column")
    assert sigma[-1] == 0.0 and np.max(np.abs(B @ Y[:, -1])) <= 12 * EPS * sigma[0]
    B = arrow_bidiagonal(12, np.random.default_rng(6), keep=0)
    B[11, 11] = 0  # what an alpha_j that is exactly zero leaves: the last ROW is zero, the left null vector is e_11
    sigma, X, Y = check_jacobi(B, "zero alpha")
    assert sigma[-1] <= 12 * EPS * sigma[0] and abs(abs(X[11, -1]) - 1) <= 12 * EPS
    B = np.diag([3.0, 2.0, 2.0, 1.0])  # a double singular value
    B[0, 3] = 0.5
    sigma, X, Y = check_jacobi(B, "double value")
    assert abs(sigma[1] - 2) <= 4 * EPS * sigma[0] and abs(sigma[2] - 2) <= 4 * EPS * sigma[0]
    sigma, X, Y = check_jacobi(np.zeros((3, 3)), "zero matrix")
    assert np.all(sigma == 0) and np.array_equal(X, np.eye(3)) and np.array_equal(Y, np.eye(3))
    sigma, X, Y = check_jacobi(np.diag([1.0, 3.0, 2.0]), "diagonal")
    assert sigma.tolist() == [3.0, 2.0, 1.0] and np.array_equal(np.abs(Y), np.eye(3)[:, [1, 2, 0]])


def test_selection_and_keep_rules(bsm):
    assert select(LM, 5, 2) == [0, 1] == raw_select(LM, 5, 2)
    assert select(SM, 5, 3) == [4, 3, 2] == raw_select(SM, 5, 3)
    for d in range(0, 9):
        for count in range(0, d + 1):
            for which in (LM, SM):
                assert raw_select(which, d, count) == select(which, d, count)
    hand = {(4, 20): 12, (5, 12): 8, (1, 3): 2, (4, 128): 66, (17, 24): 20, (6, 8): 7, (126, 128): 127}
    for (nsv, ncv), keep in hand.items():
        assert keep_of(nsv, ncv) == keep == raw_keep(nsv, ncv) and nsv <= keep <= ncv - 1


@pytest.mark.parametrize("which", [LM, SM], ids=["LM", "SM"])
def test_restart_bookkeeping_against_lapack(bsm, which):
    """two cycles of made-up alpha / beta through the library's SvdProjected: the kept values are the selected sigma of the first
    cycle in the order of the selection, the arrow is beta_m X[m - 1, i] up to the sign of the column (checked as |arrow|, and
    through the second cycle's sigma, which do not depend on the signs), the estimates are |beta_m X[m - 1, i]|"""
    rng = np.random.default_rng(90 + which)
    nsv, ncv = 3, 9
    keep = keep_of(nsv, ncv)
    alpha, beta = rng.uniform(0.5, 3, (2, ncv)), rng.uniform(0.1, 1, (2, ncv))
    B1 = np.diag(alpha[0]) + np.diag(beta[0][:-1], 1)
    X1, s1, _ = np.linalg.svd(B1)
    d, sigma, est, _, _ = raw_cycles(which, nsv, ncv, alpha[:1], beta[:1])
    assert d == ncv and np.max(np.abs(sigma - s1)) <= ncv * EPS * s1[0]
    assert np.max(np.abs(est - np.abs(beta[0][-1] * X1[-1]))) <= 8 * ncv * EPS * s1[0]
    idx = select(which, ncv, keep)
    d, sigma, est, kept, arrow = raw_cycles(which, nsv, ncv, alpha, beta)
    assert d == ncv and np.max(np.abs(kept - s1[idx])) <= ncv * EPS * s1[0]
    assert np.max(np.abs(np.abs(arrow) - np.abs(beta[0][-1] * X1[-1, idx]))) <= 8 * ncv * EPS * s1[0]
    B2 = np.zeros((ncv, ncv))
    B2[np.arange(keep), np.arange(keep)] = s1[idx]
    B2[:keep, keep] = beta[0][-1] * X1[-1, idx]
    for j in range(keep, ncv):
        B2[j, j] = alpha[1][j]
        if j + 1 < ncv:
            B2[j, j + 1] = beta[1][j]
    X2, s2, _ = np.linalg.svd(B2)
    assert np.max(np.abs(sigma - s2)) <= 8 * ncv * EPS * s2[0]
    assert np.max(np.abs(est - np.abs(beta[1][-1] * X2[-1]))) <= 64 * ncv * EPS * s2[0]
    # a beta that is exactly zero ends the space there
    beta0 = beta[:1].copy()
    beta0[0, 4] = 0
    d, sigma, est, _, _ = raw_cycles(which, nsv, ncv, alpha[:1], beta0)
    assert d == 5 and np.all(est == 0)
    assert np.max(np.abs(sigma - np.linalg.svd(B1[:5, :5], compute_uv=False))) <= ncv * EPS * s1[0]
    alpha_nan = alpha[:1].copy()
    alpha_nan[0, 2] = np.nan
    assert raw_cycles(which, nsv, ncv, alpha_nan, beta[:1])[0] == -1


def test_the_problem_meets_its_premises():
    """(about the test problem alone: the one test of this module that does not touch the library)"""
    for dt in DTYPES:
        A, rsets, csets, s, v0 = svd_dense(dt)
        assert A.dtype == np.dtype(dt) and A.shape == (M600, N400) and len(v0) == N400
        assert sum(len(r) for r in rsets) == M600 and sum(len(c) for c in csets) == N400
        assert np.array_equal(s[:5], LOW) and np.array_equal(s[-5:], HIGH) and s[5:-5].min() >= 2 and s[5:-5].max() <= 3
        ref = stored_singular_values(Dense(A))
        # the stored matrix has the designed spectrum to the precision of its type
        assert np.max(np.abs(ref[::-1] - s)) <= M600 * np.finfo(dt).eps * HIGH[-1]


# cycles of the twin on the 600 x 400 problem at svd_rtol from the problem's v0 (the same for A and adjoint(A): the recurrence
# runs on the tall orientation either way): what test_gpu_svds.py compares the device's counts with (<= twin + 1)
TWIN_CYCLES = {
    "float32": {"LM": (1, 2, 12, 1), "SM": (2, 9, 1)},
    "float64": {"LM": (1, 4, 26, 1), "SM": (4, 16, 1)},
    "complex64": {"LM": (1, 2, 13, 1), "SM": (2, 9, 1)},
    "complex128": {"LM": (1, 4, 27, 1), "SM": (4, 17, 1)},
}


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("which", ["LM", "SM"])
def test_twin_against_svd_of_the_stored_matrix(which, side, dtype):
    A = svd_dense(dtype)[0]
    ref = stored_singular_values(Dense(A))
    shape = (M600, N400) if side == "A" else (N400, M600)
    eps = float(np.finfo(dtype).eps)
    which_code = {"LM": LM, "SM": SM}
    cycles = []
    for nsv, ncv in CASES[which]:
        r = twin_of(dtype, side, nsv, ncv, which)
        assert r.status == 0 and r.nconv == nsv and r.U.shape == (shape[0], nsv) and r.V.shape == (shape[1], nsv)
        assert np.all(r.estimate <= svd_rtol(dtype) * r.anorm)
        assert r.anorm <= ref[0] * (1 + M600 * eps)
        check_triplets(r.value, r.estimate, r.residual_av, r.residual_ahu, r.anorm, ref, which, shape, ncv, dtype,
                       f"twin {name(dtype)} {side} {which} {nsv, ncv}")
        assert r.orth <= 27 * eps, (r.orth / eps)  # (what the acceptance's margin of 8 multiplies)
        # the library's bookkeeping and Jacobi SVD on the bidiagonal matrix this run's first cycle produced, against LAPACK:
        # |sigma - ref| <= ncv eps sigma_max (the bound of the Jacobi hook's own test)
        a1, b1 = r.first
        d, sigma, _, _, _ = raw_cycles(which_code[which], nsv, ncv, a1[None], b1[None])
        s1 = np.linalg.svd(np.diag(a1) + np.diag(b1[:-1], 1), compute_uv=False)
        assert d == ncv and np.max(np.abs(sigma - s1)) <= ncv * EPS * s1[0], (d, np.max(np.abs(sigma - s1)) / (ncv * EPS * s1[0]))
        if r.cycles == 1:  # converged in that cycle: the values the twin returns are those of this matrix
            assert np.max(np.abs(sigma[select(which, ncv, nsv)] - r.value)) <= ncv * EPS * s1[0]
        print(f"SVDSTAT twin {name(dtype)} {side} {which} {nsv, ncv}: cycles {r.cycles} steps {r.steps} orth / eps {r.orth / eps:.1f}")
        cycles.append(r.cycles)
    assert tuple(cycles) == TWIN_CYCLES[name(dtype)][which], cycles
    assert max(cycles) <= (27 if which == "LM" else 17)


def test_twin_statuses():
    A, _, _, _, v0 = svd_dense(np.float64)
    r = svds_twin(A, v0, 1, 3, "SM", 1e-10, maxcycles=5)  # (SM with (1, 3) does not converge in 300 cycles either)
    assert r.status == 1 and r.nconv == 1 and r.cycles == 5
    r = svds_twin(A, np.zeros(N400), 4, 20, "LM", 1e-10)
    assert r.status == 3 and r.nconv == 0
    D = np.diag(np.arange(12.0, 0.0, -1.0))
    e1 = np.zeros(12)
    e1[0] = 1
    r = svds_twin(D, e1, 1, 3, "LM", 1e-10)
    assert r.status == 0 and r.nconv == 1 and r.value[0] == 12.0 and np.all(r.estimate == 0)
    r = svds_twin(D, e1, 2, 4, "LM", 1e-10)
    assert r.status == 3 and r.nconv == 1 and r.value[0] == 12.0
    # the library's bookkeeping ends the space at the same place from the same alpha / beta
    d, sigma, est, _, _ = raw_cycles(LM, 2, 4, r.first[0][None], r.first[1][None])
    assert d == 1 and sigma.tolist() == [12.0] and est.tolist() == [0.0]
    An = A.copy()
    An[7, 9] = np.nan
    r = svds_twin(An, v0, 4, 20, "LM", 1e-10)
    assert r.status == 2 and r.nconv == 0
    assert raw_cycles(LM, 4, 20, r.first[0][None], r.first[1][None])[0] == -1  # not finite: what the solve reports as status 2
    # a start vector in the null space of a square operator: alpha_0 = 0, q_0 = 0, beta_0 = 0 -- the triplet (0, 0, e_12)
    Z = np.zeros((12, 12))
    Z[:11, :11] = np.diag(np.arange(1.0, 12.0))
    e12 = np.zeros(12)
    e12[11] = 1
    r = svds_twin(Z, e12, 1, 3, "SM", 1e-10)
    assert r.status == 0 and r.nconv == 1 and r.value[0] == 0 and not r.U.any() and abs(r.V[11, 0]) == 1
    assert r.residual_av[0] == 0 and r.residual_ahu[0] == 0


def compiler():
    for c in (os.environ.get("CXX"), "/opt/rocm/lib/llvm/bin/clang++", "clang++", "c++", "g++"):
        if c and shutil.which(c):
            return shutil.which(c)
    return None


def test_host_check_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """tools/svds_host_check.cpp: a stand-alone program (its own main, the standard library only) over csrc/bsm_svds.h"""
    cxx = compiler()
    assert cxx, "no C++ compiler found"
    exe = str(tmp_path / "svds_host_check")
    # (the sanitizer runtimes linked statically: the program needs nothing from its environment)
    static = ["-static-libsan"] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static + [
        "-I", os.path.join(ROOT, "blocksparsematrices.jl_amd", "csrc"), os.path.join(ROOT, "tools", "svds_host_check.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout[-4000:])
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert "all checks passed" in run.stdout


def test_constants_exports_and_struct_layouts(bsm):
    from bsm_amd import _lib as L
    lib = L.lib()
    for fn in ("bsm_svds_create", "bsm_svds_solve", "bsm_svds_destroy"):
        assert fn in L.EXPORTS and hasattr(lib, fn) and getattr(lib, fn).restype is C.c_int
    assert (L.BSM_SVDS_LM, L.BSM_SVDS_SM) == (LM, SM)
    assert C.sizeof(L.BsmSvdsParams) == 32 and C.sizeof(L.BsmSvdsInfo) == 48 and C.sizeof(L.BsmSvdsTriplet) == 32
    assert L.BsmSvdsParams.rtol.offset == 8 and L.BsmSvdsParams.maxcycles.offset == 24 and L.BsmSvdsInfo.a_products.offset == 16
    assert MAX_NCV == L.BSM_GMRES_MAX_RESTART
    for name_ in ("Svds", "SvdsInfo", "svds"):
        assert hasattr(bsm, name_)


def test_refusals_that_need_no_device(bsm):
    """an analysis-only handle, null arguments and the order of the checks in front of it"""
    from _common import NODEV
    from _svds import ERR_DEVICE, ERR_INVALID, raw_svds_create, raw_svds_destroy
    A = bsm.BlockSparseMatrix([np.ones((6, 9))], [np.arange(1, 7)], [np.arange(1, 10)], (6, 9), device=NODEV)
    assert raw_svds_create(None, 0, 1, 1, 3)[0] == ERR_INVALID
    assert raw_svds_create(A, 0, 1, 1, 3, null_out=True)[0] == ERR_INVALID
    assert raw_svds_create(A, 3, 1, 1, 3)[0] == ERR_INVALID
    assert raw_svds_create(A, 0, 4, 1, 3)[0] == ERR_INVALID
    assert raw_svds_create(A, 0, 3, 1, 3)[0] == ERR_INVALID  # a real handle under a complex vdtype
    rc, out = raw_svds_create(A, 0, 1, 1, 3)  # not square: no refusal of its own
    assert rc == ERR_DEVICE and not out.value
    assert raw_svds_destroy(None) == 0
