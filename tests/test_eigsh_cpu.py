"""CPU suite of bsm_eigsh (no GPU): the Jacobi eigensolver of the projected matrix (csrc/bsm_eig.h, hook bsm_debug_eig_jacobi)
against numpy.linalg.eigvalsh; the selection and keep rules (hooks bsm_debug_eig_select / _keep and the twin's own copies) on
hand cases; the premises of the order-400 problem; the numpy twin of the solve (tests/_eigsh.py) against eigvalsh of the
matrix as stored, for every `which` and type; the twin's cycle counts for the cases test_gpu_eigsh.py runs; the exported
constants.  The hook tests fail without the feature: the entry points do not exist there."""
import ctypes as C

import numpy as np
import pytest

from _eigsh import (BE, CASES, DTYPES, HIGH, LA, LM, LOW, MAX_NCV, NEIG, SA, WHICH, check_pairs, eig_dense, eig_rtol, eigsh_twin,
                    keep_of, raw_jacobi, raw_keep, raw_select, select, stored_eigenvalues, tridiagonal_block, twin_of)

name = lambda d: np.dtype(d).name  # noqa: E731


def arrow_tridiagonal(m, rng):
    """the shape of T after a restart: diag(theta) with an arrow row at `keep`, tridiagonal behind it"""
    keep = m // 3
    T = np.zeros((m, m))
    T[np.arange(m), np.arange(m)] = rng.uniform(-3, 6, m)
    for i in range(keep):
        T[i, keep] = T[keep, i] = rng.uniform(-1, 1) * 10.0 ** rng.integers(-12, 1)
    for j in range(keep, m - 1):
        T[j, j + 1] = T[j + 1, j] = rng.uniform(0.1, 2)
    return T


@pytest.mark.parametrize("m", [1, 2, 3, 20, 128])
def test_jacobi_hook_against_eigvalsh(bsm, m):
    rng = np.random.default_rng(500 + m)
    T = arrow_tridiagonal(m, rng)
    theta, S = raw_jacobi(T)
    ref = np.linalg.eigvalsh(T)
    scale = m * np.finfo(np.float64).eps * np.linalg.norm(T, 2)
    print(f"EIGSTAT jacobi m {m}: max |theta - ref| / scale {np.max(np.abs(theta - ref)) / scale:.3f}, ||T S - S diag|| / scale "
          f"{np.linalg.norm(T @ S - S * theta, 2) / scale:.3f}, ||S^T S - I|| / (m eps) {np.linalg.norm(S.T @ S - np.eye(m), 2) / (m * 2.2e-16):.3f}")
    assert np.all(np.diff(theta) >= 0)
    assert np.max(np.abs(theta - ref)) <= scale
    assert np.linalg.norm(T @ S - S * theta, 2) <= scale
    assert np.linalg.norm(S.T @ S - np.eye(m), 2) <= m * np.finfo(np.float64).eps * max(1.0, np.linalg.norm(T, 2))
    theta2, S2 = raw_jacobi(T)
    assert theta.tobytes() == theta2.tobytes() and S.tobytes() == S2.tobytes()


def test_jacobi_hook_on_a_diagonal_and_a_repeated_eigenvalue(bsm):
    theta, S = raw_jacobi(np.diag([3.0, -1.0, 2.0]))
    assert theta.tolist() == [-1.0, 2.0, 3.0] and np.array_equal(np.abs(S), np.eye(3)[:, [1, 2, 0]])
    T = np.full((4, 4), 1.0)  # eigenvalues 0, 0, 0, 4
    theta, S = raw_jacobi(T)
    assert np.allclose(theta, [0, 0, 0, 4], atol=1e-15) and np.linalg.norm(T @ S - S * theta) <= 1e-14


HAND = [
    # which, theta ascending, count, wanted indices in the order of the report
    (LA, [-2, -1, 0, 1, 5], 2, [4, 3]),
    (SA, [-2, -1, 0, 1, 5], 3, [0, 1, 2]),
    (BE, [-2, -1, 0, 1, 5], 3, [4, 3, 0]),  # odd count: two from the top, one from the bottom
    (BE, [-2, -1, 0, 1, 5], 4, [4, 3, 0, 1]),
    (BE, [-2, -1, 0, 1, 5], 1, [4]),
    (LM, [-6, -1, 0, 1, 5], 3, [0, 4, 3]),  # |-1| == |1|: the positive one first
    (LM, [-6, -1, 0, 1, 5], 4, [0, 4, 3, 1]),
    (LM, [-3, -2, 4], 3, [2, 0, 1]),
    (LA, [1.0], 1, [0]),
]


@pytest.mark.parametrize("which,theta,count,want", HAND)
def test_selection_rules_on_hand_cases(bsm, which, theta, count, want):
    assert select(which, np.array(theta, float), count) == want
    assert raw_select(which, theta, count) == want


def test_selection_of_library_and_twin_agree_on_random_spectra(bsm):
    rng = np.random.default_rng(9)
    for _ in range(50):
        m = int(rng.integers(1, 40))
        theta = np.sort(rng.uniform(-3, 3, m).round(1))  # (rounded: equal magnitudes and equal values occur)
        for which in WHICH.values():
            count = int(rng.integers(0, m + 1))
            assert raw_select(which, theta, count) == select(which, theta, count)


def test_keep_rule(bsm):
    hand = {(4, 20): 12, (5, 12): 8, (1, 3): 2, (4, 128): 66, (6, 8): 7, (3, 5): 4, (126, 128): 127}
    for (nev, ncv), keep in hand.items():
        assert keep_of(nev, ncv) == keep == raw_keep(nev, ncv) and nev <= keep <= ncv - 1


def test_the_problem_meets_its_premises():
    for dt in DTYPES:
        D, sets, lam, v0 = eig_dense(dt)
        assert D.dtype == np.dtype(dt) and D.shape == (NEIG, NEIG) and np.array_equal(D, D.conj().T)
        assert np.array_equal(lam[:5], LOW) and np.array_equal(lam[-5:], HIGH) and lam[5:-5].min() >= 1 and lam[5:-5].max() <= 2
        out = np.concatenate([LOW, HIGH])
        assert np.min(np.diff(LOW)) >= 0.4 - 1e-12 and np.min(np.diff(HIGH)) >= 0.4 - 1e-12
        assert 1 - LOW[-1] >= 0.6 and HIGH[0] - 2 >= 0.6
        mags = np.sort(np.abs(out))
        assert np.min(np.diff(mags)) >= 0.1 - 1e-12
        ref = stored_eigenvalues(D)
        # the stored matrix has the designed spectrum to the precision of its type
        assert np.max(np.abs(ref - np.sort(lam))) <= NEIG * np.finfo(dt).eps * 6


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("which", list(WHICH))
def test_twin_against_eigvalsh_of_the_stored_matrix(which, dtype):
    D = eig_dense(dtype)[0]
    ref = stored_eigenvalues(D)
    eps = float(np.finfo(dtype).eps)
    worst = 0.0
    for nev, ncv in CASES + [(4, 400)]:
        r = twin_of(dtype, nev, ncv, which)
        assert r.status == 0 and r.nconv == nev and r.X.shape == (NEIG, nev)
        tol = eig_rtol(dtype) * r.anorm
        assert np.all(r.estimate <= tol)
        assert r.anorm <= np.max(np.abs(ref)) * (1 + NEIG * eps)  # a lower bound of ||A||_2, up to the error of both sides
        worst = max(worst, check_pairs(r.value, r.estimate, r.residual, r.anorm, ref, which, tol, dtype, f"twin {name(dtype)} {which} {nev, ncv}"))
        print(f"EIGSTAT twin {name(dtype)} {which} {nev, ncv}: cycles {r.cycles} steps {r.steps} orth / eps {r.orth / eps:.1f}")
    # the gap between the true residual and the estimate is rounding: forming X = V S ((ncv + 1) eps |V| |S|, times ||A||), the
    # product (n eps ||A||) and the loss of orthogonality the two Gram-Schmidt passes leave.  Measured: docs/experiments_r36.md
    assert worst <= NEIG + MAX_NCV + 2, worst


# cycles of the twin on the order-400 problem at eig_rtol from the problem's v0: what test_gpu_eigsh.py compares the device's
# counts with (<= twin + 1).  Rows: (nev, ncv); columns: LA, SA, BE, LM.
TWIN_CYCLES = {
    "float32": {(4, 20): (1, 1, 1, 1), (5, 12): (3, 4, 3, 3), (1, 3): (26, 26, 38, 38), (4, 128): (1, 1, 1, 1), (4, 400): (1, 1, 1, 1)},
    "float64": {(4, 20): (2, 2, 2, 2), (5, 12): (7, 7, 5, 6), (1, 3): (58, 57, 93, 93), (4, 128): (1, 1, 1, 1), (4, 400): (1, 1, 1, 1)},
    "complex64": {(4, 20): (1, 1, 1, 1), (5, 12): (4, 4, 3, 4), (1, 3): (27, 26, 43, 43), (4, 128): (1, 1, 1, 1), (4, 400): (1, 1, 1, 1)},
    "complex128": {(4, 20): (2, 2, 1, 2), (5, 12): (8, 7, 4, 6), (1, 3): (59, 57, 97, 97), (4, 128): (1, 1, 1, 1), (4, 400): (1, 1, 1, 1)},
}


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
def test_twin_cycle_counts_are_pinned(dtype):
    for case, counts in TWIN_CYCLES[name(dtype)].items():
        got = tuple(twin_of(dtype, *case, w).cycles for w in ("LA", "SA", "BE", "LM"))
        assert got == counts, (name(dtype), case, got)
        # the design's own figures: (4, 20) at most 2 cycles, (5, 12) at most 8, (1, 3) 25 .. 99, (4, 400) one
        lo, hi = {(4, 20): (1, 2), (5, 12): (1, 8), (1, 3): (25, 99), (4, 128): (1, 1), (4, 400): (1, 1)}[case]
        assert all(lo <= c <= hi for c in got)


def test_twin_statuses():
    D, _, _, v0 = eig_dense(np.float64)
    r = eigsh_twin(D, v0, 5, 12, "SA", 1e-10, maxcycles=1)
    assert r.status == 1 and r.nconv == 5 and r.cycles == 1
    r = eigsh_twin(D, np.zeros(NEIG), 4, 20, "LA", 1e-10)
    assert r.status == 3 and r.nconv == 0
    for dt in DTYPES:
        _, T, e1 = tridiagonal_block(dt)
        r = eigsh_twin(T, e1, 4, 8, "LA", 1e-10)
        want = np.linalg.eigvalsh(T[:3, :3].astype(np.float64))[::-1]
        assert r.status == 3 and r.nconv == 3 and np.max(np.abs(r.value - want)) <= 8 * np.finfo(np.float64).eps * 4
        assert np.all(r.estimate == 0) and np.all(r.X[3:] == 0)
        r = eigsh_twin(T, e1, 3, 8, "SA", 1e-10)  # the space ends with as many pairs as are wanted: convergence
        assert r.status == 0 and r.nconv == 3
    Dn = D.copy()
    Dn[7, 9] = Dn[9, 7] = np.nan
    r = eigsh_twin(Dn, v0, 4, 20, "LA", 1e-10)
    assert r.status == 2 and r.nconv == 0


def test_constants_exports_and_struct_layouts(bsm):
    from bsm_amd import _lib as L
    lib = L.lib()
    for fn in ("bsm_krylov_combine_tile", "bsm_krylov_combine", "bsm_eigsh_create", "bsm_eigsh_solve", "bsm_eigsh_destroy"):
        assert fn in L.EXPORTS and hasattr(lib, fn)
    assert (L.BSM_EIGSH_LA, L.BSM_EIGSH_SA, L.BSM_EIGSH_BE, L.BSM_EIGSH_LM) == (LA, SA, BE, LM)
    assert C.sizeof(L.BsmEigshParams) == 32 and C.sizeof(L.BsmEigshInfo) == 48 and C.sizeof(L.BsmEigshPair) == 24
    assert MAX_NCV == L.BSM_GMRES_MAX_RESTART
    # the documented tile: whole waves of real rows in 128 KiB of LDS, at most 1024; half as many complex elements
    for code, rs, nc in ((0, 4, 1), (1, 8, 1), (2, 4, 2), (3, 8, 2)):
        for m in (1, 2, 3, 20, 33, 127, 128):
            assert lib.bsm_krylov_combine_tile(code, m) == min(1024, 131072 // (m * rs) // 64 * 64) // nc
    assert lib.bsm_krylov_combine_tile(4, 8) < 0 and lib.bsm_krylov_combine_tile(1, 0) < 0 and lib.bsm_krylov_combine_tile(1, 129) < 0
    for name_ in ("Eigsh", "EigshInfo", "eigsh", "krylov_combine"):
        assert hasattr(bsm, name_)


def test_refusals_that_need_no_device(bsm):
    """an analysis-only handle, null arguments and the ranges of nev / ncv are refused before anything touches a device"""
    from _common import NODEV
    from _eigsh import ERR_DEVICE, ERR_INVALID, raw_combine, raw_eigsh_create, raw_eigsh_destroy
    A = bsm.BlockSparseMatrix([np.eye(6)], [np.arange(1, 7)], [np.arange(1, 7)], (6, 6), device=NODEV)
    assert raw_eigsh_create(None, 0, 1, 1, 3)[0] == ERR_INVALID
    assert raw_eigsh_create(A, 0, 1, 1, 3, null_out=True)[0] == ERR_INVALID
    assert raw_eigsh_create(A, 3, 1, 1, 3)[0] == ERR_INVALID
    assert raw_eigsh_create(A, 0, 4, 1, 3)[0] == ERR_INVALID
    assert raw_eigsh_create(A, 0, 3, 1, 3)[0] == ERR_INVALID  # a real handle under a complex vdtype
    rc, out = raw_eigsh_create(A, 0, 1, 1, 3)
    assert rc == ERR_DEVICE and not out.value
    assert raw_eigsh_destroy(None) == 0
    R = np.zeros((4, 4), order="F")
    p = R.ctypes.data
    assert raw_combine(7, 4, 2, 1, p, 4, p, 2, p, 4, -1) == ERR_INVALID
    assert raw_combine(1, -1, 2, 1, p, 4, p, 2, p, 4, -1) == ERR_INVALID
    assert raw_combine(1, 4, 0, 0, p, 4, p, 2, p, 4, -1) == ERR_INVALID
    assert raw_combine(1, 4, 129, 1, p, 4, p, 129, p, 4, -1) == ERR_INVALID
