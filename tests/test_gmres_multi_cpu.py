"""CPU suite of what test_gpu_gmres_multi.py relies on (tests/_gmres_multi.py): the numpy twin of one column of
bsm_gmres_multi_solve against _krylov.gmres_twin, why its least-squares solve is a QR factorisation, its pinned counts on
the problems the GPU file runs to convergence, the Python mirror of the workspace carve, and the sharpness of the iterate
check: a twin whose dots lose the last workgroup's rows lies far outside the bound the GPU file uses.  No GPU: the library
is loaded for its host-side test hook only.  Figures are printed in LOCKSTAT lines before they are asserted."""
import numpy as np
import pytest

from _cg import MAX_RHS
from _gmres_multi import (GRID_ITS, GRID_RESTART, MARGIN, STATE_BYTES, gmres_multi_twin, reference, spread, workspace_bytes)
from _jacobi import uniform
from _krylov import exact_minv, gmres_twin, krylov_problem, raw_lsq, rtol_of
from _lockstep import (RANGE_BYTES, TABLE, TABLE_IDS, block_solve, deviation, grid_case, half_sets, krylov_grid, last_range_rows,
                       path_rtol, staggered6)
from _submat import Truth

DENSE = [(np.float64, 1025), (np.complex128, 513), (np.float32, 2049), (np.complex64, 1025)]  # the G = 2 rows of the table


def name(dtype):
    return np.dtype(dtype).name


# ---- the twin against _krylov.gmres_twin ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype, n", DENSE, ids=[f"{name(d)}-n{n}" for d, n in DENSE])
def test_the_twin_is_the_method_of_gmres_twin(dtype, n):
    """on the dense form of the grid problem, with the least-squares solve of gmres_twin (lsq="lstsq"): statuses, counts and
    cycles equal after GMRES(3) x 5 and to path_rtol at restart 5; iterate and history within the twin's own spread under
    permuted sums -- gmres_twin forms its dots as one BLAS matrix-vector product, which is one more summation order
    (measured: 1.0 .. 2.0 eps max|x| and 0 .. 0.65 eps ||b|| against spreads of 1.5 .. 3.8 and 0.3 .. 1.5; the history of
    column 15 in the two single types sits ON its spread, 0.60 and 0.61: both are one unit in the last place of the same
    entry)"""
    _, Dop, B = grid_case("bicgstab", n, dtype)
    D = Dop.dense()
    for c in (0, MAX_RHS - 1):
        old = gmres_twin(D, B[:, c], None, GRID_RESTART, 0.0, GRID_ITS, dtype)
        new = gmres_multi_twin(Dop, B[:, c], None, GRID_RESTART, 0.0, GRID_ITS, dtype, lsq="lstsq")
        assert (new.status, new.iterations, new.cycles) == (old.status, old.iterations, old.cycles) == (1, GRID_ITS, 2)
        assert len(new.iterates) == GRID_ITS and np.array_equal(new.iterates[-1], new.x)
        dx = float(np.max(np.abs(new.x - old.x)) / (np.finfo(dtype).eps * np.max(np.abs(old.x))))
        dh = float(np.max(np.abs(new.history - old.history)) / (np.finfo(dtype).eps * old.bnorm))
        sx, sh = spread(Dop, B[:, c], GRID_ITS, dtype, lsq="lstsq")
        print(f"LOCKSTAT gmres twins {name(dtype)} n={n} column {c}: iterate {dx:.2f} eps max|x| (spread {sx:.2f}), history {dh:.2f} eps |b| "
              f"(spread {sh:.2f}), estimate after {GRID_ITS}: {new.history[-1] / new.bnorm:.3f} |b|")
        assert dx <= sx and dh <= sh
        assert 0.1 <= new.history[-1] / new.bnorm <= 0.25
        rtol = path_rtol(dtype)
        old = gmres_twin(D, B[:, c], None, 5, rtol, 200, dtype)
        for lsq in ("lstsq", "qr"):
            new = gmres_multi_twin(Dop, B[:, c], None, 5, rtol, 200, dtype, lsq=lsq)
            assert (new.status, new.iterations, new.cycles) == (old.status, old.iterations, old.cycles), lsq
            assert new.status == 0 and new.residual == new.history[-1] <= rtol * new.bnorm


@pytest.mark.parametrize("kind, dtype", [("vbcrs", np.float32), ("blocksparse", np.complex128), ("symmetric", np.float64)])
def test_the_twin_with_a_preconditioner_and_an_initial_guess(kind, dtype):
    """order 400 with the exact block-Jacobi inverse, restart 20 and restart 1, from zero and from a guess: the counts,
    cycles and statuses of gmres_twin, converged or not"""
    p, sets, b = krylov_problem(kind, dtype)
    D = Truth(p).D
    Minv = exact_minv(D, sets)
    x0 = uniform(np.random.default_rng(9300), (len(b),), dtype)
    for restart, guess in ((20, None), (20, x0), (1, None)):
        old = gmres_twin(D, b, Minv, restart, rtol_of(dtype), 400, dtype, x0=guess)
        new = gmres_multi_twin(D, b, Minv, restart, rtol_of(dtype), 400, dtype, x0=guess)
        assert (new.status, new.iterations, new.cycles) == (old.status, old.iterations, old.cycles), (restart, guess is None)
        assert old.status == 0 or restart == 1  # (GMRES(1) stalls on the symmetric operator: 400 cycles of one iteration)
        assert np.allclose(new.history, old.history, rtol=1e3 * np.finfo(dtype).eps, atol=1e3 * np.finfo(dtype).eps * old.bnorm)
    # maxiter = 0, a zero right-hand side, a NaN
    z = gmres_multi_twin(D, b, Minv, 20, rtol_of(dtype), 0, dtype)
    assert (z.status, z.iterations, z.cycles) == (1, 0, 0) and not np.any(z.x)
    z = gmres_multi_twin(D, np.zeros_like(b), Minv, 20, 0.0, 50, dtype)
    assert (z.status, z.iterations, z.residual) == (0, 0, 0.0)
    bad = b.copy()
    bad[-1] = np.nan
    z = gmres_multi_twin(D, bad, Minv, 20, rtol_of(dtype), 50, dtype)
    assert (z.status, z.iterations) == (2, 0) and not np.any(z.x)


def solve3_wide(H, e):
    """the least-squares solution of the 4 x 3 system by the normal equations in extended precision (condition number 5,
    so its square costs nothing that matters at 64 mantissa bits): Gaussian elimination by hand, numpy.linalg has no
    longdouble"""
    Hl, el = H.astype(np.longdouble), e.astype(np.longdouble)
    A, r = Hl.T @ Hl, Hl.T @ el
    k = len(r)
    for i in range(k):
        for j in range(i + 1, k):
            f = A[j, i] / A[i, i]
            A[j] -= f * A[i]
            r[j] -= f * r[i]
    y = np.zeros(k, np.longdouble)
    for i in range(k - 1, -1, -1):
        y[i] = (r[i] - A[i, i + 1:] @ y[i + 1:]) / A[i, i]
    return y


@pytest.mark.skipif(np.finfo(np.longdouble).eps > 1e-18, reason="needs an extended-precision long double for the reference solution")
def test_why_the_twin_solves_its_least_squares_problem_by_qr(bsm):
    """float64, n = 1025, column 0 of the grid problem, three iterations: numpy.linalg.lstsq returns y tens of eps off the
    extended-precision solution of a system of condition number 4.9, Householder QR and the library's rotations (the host
    form of the one-wave kernels' arithmetic, bsm_debug_krylov_lsq_host) stay within a few eps.  With lstsq the twin's third
    iterate lies outside the bound of the iterate check although its sums are formed like the honest twin's: the error
    is the same under every summation order, so no spread shows it"""
    dtype, n = np.float64, 1025
    _, Dop, B = grid_case("bicgstab", n, dtype)
    qr = gmres_multi_twin(Dop, B[:, 0], None, GRID_RESTART, 0.0, 3, dtype)
    ls = gmres_multi_twin(Dop, B[:, 0], None, GRID_RESTART, 0.0, 3, dtype, lsq="lstsq")
    H, beta = qr.hessenberg, qr.beta
    assert H.shape == (4, 3) and np.array_equal(H, ls.hessenberg) and np.linalg.cond(H) < 5
    e = np.zeros(4)
    e[0] = beta
    yw = solve3_wide(H, e)
    eps = np.finfo(dtype).eps

    def off(y):
        return float(np.max(np.abs((y.astype(np.longdouble) - yw) / yw)) / eps)
    Q, R = np.linalg.qr(H)
    rc, yg, _, _ = raw_lsq(H, beta)
    errs = dict(lstsq=off(np.linalg.lstsq(H, e, rcond=None)[0]), qr=off(np.linalg.solve(R, Q.T @ e)), rotations=off(yg))
    sx, _ = spread(Dop, B[:, 0], 3, dtype)
    dx = float(np.max(np.abs(ls.x - qr.x)) / (eps * np.max(np.abs(qr.x))))
    print(f"LOCKSTAT gmres least squares: y off the extended-precision solution by {errs} eps; third iterate of the lstsq twin off the "
          f"QR twin's by {dx:.1f} eps max|x|, spread {sx:.2f}")
    assert rc == 0 and errs["qr"] <= 8 and errs["rotations"] <= 8
    if errs["lstsq"] > 8:  # (what another LAPACK does is not this project's to pin; where it errs, the iterate shows it)
        assert dx > MARGIN * sx


# ---- the pinned counts --------------------------------------------------------------------------------------------------------
PATHS = {2: ([58, 60, 58], [43, 42, 42], [41, 40, 41], [39, 39, 40]),  # complex128 n = 513: plain, M, x0, float64 A; restart 5, rtol 1e-6
         3: ([62, 64, 62], [39, 39, 39], [45, 44, 45], [44, 44, 44])}  # n = 1027
STAGGERED = {"complex128": [131, 86, 44, 8, 0, 0], "float32": [31, 22, 13, 7, 0, 0]}  # n = 32769 / 131073, restart 5


@pytest.mark.parametrize("G", [2, 3])
def test_counts_on_the_selected_paths(G):
    """complex128 at G = 2, 3, restart 5 to path_rtol: plain, with the half-block preconditioner, from the initial guess and
    with the float64 operator -- 39 .. 64 iterations over 8 .. 13 cycles, the same counts under a permuted summation order
    (the GPU file allows the device +-1)"""
    dtype, n = np.complex128, {2: 513, 3: 1027}[G]
    _, Dop, B = grid_case("bicgstab", n, dtype)
    Minv = exact_minv(Dop.dense(), half_sets(n))
    sol = block_solve(Dop, B[:, :3])
    X0 = (sol + 1e-2 * np.max(np.abs(sol)) * uniform(np.random.default_rng(8900 + n), sol.shape, dtype)).astype(dtype)
    Dr = grid_case("bicgstab", n, np.float64)[1].astype(dtype)
    cases = [(Dop, {}), (Dop, dict(Minv=Minv)), (Dop, dict(x0=X0)), (Dr, {})]
    order = np.random.default_rng(0).permutation(n)
    for (D, kw), want in zip(cases, PATHS[G]):
        for o in (None, order):
            runs = [gmres_multi_twin(D, B[:, c], kw.get("Minv"), 5, path_rtol(dtype), 200, dtype, order=o,
                                     x0=kw["x0"][:, c] if "x0" in kw else None) for c in range(3)]
            assert [r.status for r in runs] == [0, 0, 0] and [r.iterations for r in runs] == want, (list(kw), o is None)
            assert all(r.cycles == -(-r.iterations // 5) for r in runs)
    assert all(m < p for m, p in zip(PATHS[G][1], PATHS[G][0])) and min(PATHS[G][1]) > GRID_ITS


@pytest.mark.parametrize("dtype", [np.complex128, np.float32], ids=["complex128", "float32"])
def test_counts_on_the_staggered_columns(dtype):
    """G = 65, restart 5, one absolute tolerance: four columns end at four counts in four different cycles, the zero column
    and the NaN column (the NaN in the LAST workgroup's range) at the start; the same counts under a permuted order, the
    estimates that end a column 1.5 .. 30 % under the tolerance"""
    n = 64 * (RANGE_BYTES // np.dtype(dtype).itemsize) + 1
    _, Dop, B = grid_case("bicgstab", n, dtype)
    tau, step = (1e-4, 10.0) if dtype == np.float32 else (1e-10, 1000.0)
    Bs, atol = staggered6(B, dtype, tau, step)
    assert last_range_rows(n, np.dtype(dtype).itemsize) >= 1 and np.isnan(Bs[n - 1, 5])
    for o in (None, np.random.default_rng(1).permutation(n)):
        runs = [gmres_multi_twin(Dop, Bs[:, c], None, 5, 0.0, 300, dtype, atol=atol, order=o) for c in range(6)]
        assert [r.status for r in runs] == [0, 0, 0, 0, 0, 2] and [r.iterations for r in runs] == STAGGERED[name(dtype)]
        assert all(r.residual <= 0.995 * atol for r in runs[:4])
    assert len({-(-k // 5) for k in STAGGERED[name(dtype)][:4]}) == 4


# ---- the mirror of the workspace carve ------------------------------------------------------------------------------------------
def test_the_mirror_of_the_workspace_carve():
    """the sizes the library reported on the device (info.workspace_bytes; the GPU file compares every solve's), the state's
    size, and that the size tells G, M and the restart"""
    assert STATE_BYTES == 1408
    # what the library reported on the device when this was written
    assert workspace_bytes(1025, np.float64, 3) == 794112 and workspace_bytes(1027, np.complex128, 3) == 1588480
    assert workspace_bytes(131073, np.float32, 3) == 50353088
    for dt, n, G in TABLE:
        es = np.dtype(dt).itemsize
        ld = (n * es + 15) // 16 * 16 // es
        assert krylov_grid(n, es) == G
        assert all(workspace_bytes(n, dt, GRID_RESTART, G=g) != workspace_bytes(n, dt, GRID_RESTART) for g in (1, G - 1, G + 1)), "the size does not tell G"
        assert workspace_bytes(n, dt, GRID_RESTART, has_m=True) - workspace_bytes(n, dt, GRID_RESTART) == (ld * es * MAX_RHS + 63) // 64 * 64
        assert workspace_bytes(n, dt, 4) - workspace_bytes(n, dt, 3) >= ld * es * MAX_RHS  # restart + 3 matrices


# ---- the check is sharp ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype, n, G", TABLE, ids=TABLE_IDS)
def test_a_lost_share_is_rejected_by_the_iterate_check(dtype, n, G):
    """the twin IN dtype whose dots lose (1) the last 1 / G of their terms, (2) exactly the rows of the last workgroup's range,
    against the reference and the bound of test_iterate_and_history_after_a_restart: out by more than 10 times the bound in
    the iterate or in the history, while the honest twin in dtype (the device's stand-in) is inside"""
    _, Dop, B = grid_case("bicgstab", n, dtype)
    b = B[:, 0]
    ref = reference(Dop, b, GRID_ITS, dtype)
    sx, sh = spread(Dop, b, GRID_ITS, dtype)
    honest = gmres_multi_twin(Dop, b, None, GRID_RESTART, 0.0, GRID_ITS, dtype)
    hx, hh = deviation(honest.x, honest.history, ref, GRID_ITS, dtype)
    assert 0 < sx <= 64 and hx <= MARGIN * sx and hh <= MARGIN * sh, (hx, sx, hh, sh)
    for keep in (n - n // G, n - last_range_rows(n, np.dtype(dtype).itemsize)):
        mut = gmres_multi_twin(Dop, b, None, GRID_RESTART, 0.0, GRID_ITS, dtype, keep=keep)
        mx, mh = deviation(mut.x, mut.history, ref, GRID_ITS, dtype)
        print(f"LOCKSTAT gmres sharp {name(dtype)} n={n} G={G}: {n - keep} terms lost: iterate {mx:.3g} eps max|x| against a bound of "
              f"{MARGIN * sx:.2f}, history {mh:.3g} against {MARGIN * sh:.3g}; honest {hx:.2f}, {hh:.3g}; spread {sx:.2f}, {sh:.3g}")
        assert mx > 10 * MARGIN * sx or mh > 10 * MARGIN * sh, (keep, mx, sx, mh, sh)
