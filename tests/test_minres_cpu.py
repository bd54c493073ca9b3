"""CPU suite of the MINRES twin (tests/_minres.py) that test_gpu_minres.py measures bsm_minres_solve against: that it solves
the indefinite problems, that the residual it carries IS b - A x, that its counts do not depend on the order of its sums,
its four statuses, and that the spread bound of the GPU suite would catch a lost share.  No GPU."""
import numpy as np
import pytest

from _cg import NB, NCG, cg_twin, column_tol
from _krylov import exact_minv, rtol_of, true_residual
from _lockstep import ITS, MARGIN, deviation, half_sets, path_rtol
from _minres import BROKEN_COUNTS, COUNTS, indef_case, minres_problem, minres_twin

DTYPES = [np.float32, np.float64, np.complex64, np.complex128]
IDS = [np.dtype(d).name for d in DTYPES]
# Bound of the residual checks, in eps times the scale of the start (||b||, or its M-norm): every iteration adds a few
# roundings of that scale to a recursively updated vector, the runs take at most 65 iterations, roundings accumulate like
# sqrt(65) ~ 8, and MARGIN = 4 of _lockstep.py on top: 32.
CARRIED_EPS = 32
_runs = {}


def runs_of(dtype):
    """(D, B, Minv, [twin run per column]) of the order-400 problem, computed once per type"""
    key = np.dtype(dtype).name
    if key not in _runs:
        _, _, sets, D, P, B = minres_problem("vbcrs", dtype)
        Minv = exact_minv(P, sets)
        _runs[key] = (D, B, Minv, [minres_twin(D, B[:, c], Minv, rtol_of(dtype), 0.0, 200, dtype) for c in range(NB)])
    return _runs[key]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_the_problem_is_indefinite_and_the_twin_solves_it(dtype):
    D, B, _, runs = runs_of(dtype)
    wide = np.complex128 if np.dtype(dtype).kind == "c" else np.float64
    ev = np.linalg.eigvalsh(D.astype(wide))
    assert np.array_equal(D, D.conj().T) and int(np.sum(ev < 0)) == 190
    lmin = float(np.min(np.abs(ev)))
    assert abs(lmin - (0.51 if np.dtype(dtype).kind == "c" else 0.34)) < 0.01
    sol = np.linalg.solve(D.astype(wide), B.astype(wide))
    assert [r.iterations for r in runs] == COUNTS[np.dtype(dtype).name]
    for c, run in enumerate(runs):
        tol = column_tol(B[:, c], rtol_of(dtype))
        true = true_residual(D, run.x, B[:, c])
        print(f"MRTWIN {np.dtype(dtype).name} column {c}: {run.iterations} iterations, true residual / tol {true / tol:.3f}")
        assert run.status == 0 and run.residual <= tol
        assert true <= tol * (1 + 1e-2), (c, true, tol)
        # x - x* = D^-1 (D x - b): within the true residual over the smallest |eigenvalue|
        assert np.linalg.norm(run.x.astype(wide) - sol[:, c]) <= 1.01 * true / lmin


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_the_carried_residual_is_the_true_one(dtype):
    """after EVERY iteration ||r|| of the recurrence against || b - D x || in complex128, to CARRIED_EPS eps of ||b|| -- the
    scale the rounding of a recursively updated residual lives on (_lockstep.deviation); relative to itself a residual
    reduced to 1e-10 ||b|| cannot be known to any multiple of eps (measured: 9e3 eps single, 1.3e10 eps double).  With M the
    Lanczos vectors are orthogonal in the M-form, not in the 2-norm, so this distinguishes the sign of the v_new term of the
    recurrence, which the norm without M does not"""
    D, B, _, runs = runs_of(dtype)
    eps = np.finfo(dtype).eps
    worst = 0.0
    for c, run in enumerate(runs):
        for j, x in enumerate(run.iterates):
            worst = max(worst, abs(run.history[j] - true_residual(D, x, B[:, c])) / (eps * run.bnorm))
    print(f"MRTWIN {np.dtype(dtype).name}: carried against true residual, worst {worst:.2f} eps ||b||")
    assert worst <= CARRIED_EPS


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_with_m_the_m_norm_of_the_residual_is_eta_and_does_not_grow(dtype):
    """what MINRES minimises with M is sqrt<r, M r>: of the TRUE residual b - D x in complex128 it does not grow from one
    iteration to the next, and |eta| of the recurrence is that norm, both to CARRIED_EPS eps of its starting value (the
    2-norm history with M has no such shape: test_grid_problems_and_monotone_history)"""
    D, B, Minv, runs = runs_of(dtype)
    eps = np.finfo(dtype).eps
    Dw, Mw = D.astype(np.complex128), Minv.astype(np.complex128)
    off = rise = 0.0
    for c, run in enumerate(runs):
        bw = B[:, c].astype(np.complex128)
        res = [bw] + [bw - Dw @ x.astype(np.complex128) for x in run.iterates]
        mn = np.array([np.sqrt((t.conj() @ (Mw @ t)).real) for t in res])
        assert len(run.etas) == run.iterations
        off = max(off, float(np.max(np.abs(mn[1:] - run.etas))) / (eps * mn[0]))
        rise = max(rise, float(np.max(np.diff(mn))) / (eps * mn[0]))
    print(f"MRTWIN {np.dtype(dtype).name}: |eta| against the M-norm of the true residual, worst {off:.2f} eps of the start; largest rise {rise:.2f}")
    assert off <= CARRIED_EPS and rise <= CARRIED_EPS


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_counts_do_not_depend_on_the_order_of_the_sums(dtype):
    D, B, Minv, runs = runs_of(dtype)
    for c, run in enumerate(runs):
        counts = [minres_twin(D, B[:, c], Minv, rtol_of(dtype), 0.0, 200, dtype, order=np.random.default_rng(seed).permutation(NCG)).iterations
                  for seed in range(8)]
        print(f"MRTWIN {np.dtype(dtype).name} column {c}: {run.iterations} iterations, {sorted(set(counts))} under 8 permuted orders")
        assert max(abs(k - run.iterations) for k in counts) <= 1


@pytest.mark.parametrize("dtype, n", [(np.float64, 1025), (np.float32, 2049), (np.complex128, 515), (np.complex64, 1025)],
                         ids=["float64", "float32", "complex128", "complex64"])
def test_grid_problems_and_monotone_history(dtype, n):
    """the block diagonal problems of the GPU suite at path_rtol: the pinned counts, the residual after ITS iterations is not
    made of rounding, and WITHOUT M the history does not grow (MINRES minimises the 2-norm of the residual then; with M it
    minimises the M-norm, and the 2-norm after the first iteration is 1.17 .. 1.65 ||b|| on the order-400 problems)"""
    _, Dop, _, Dsib, B = indef_case(n, dtype)
    Minv = exact_minv(Dsib.dense(), half_sets(n))
    plain = {"float64": 33, "float32": 22, "complex128": 47, "complex64": 33}[np.dtype(dtype).name]
    with_m = {"float64": (29, 31), "float32": (19, 20), "complex128": (40, 40), "complex64": (26, 27)}[np.dtype(dtype).name]
    for c in range(3):
        run = minres_twin(Dop, B[:, c], None, path_rtol(dtype), 0.0, 200, dtype)
        assert run.status == 0 and abs(run.iterations - plain) <= 1, (c, run.iterations)
        assert 0.1 <= run.history[ITS - 1] / run.bnorm <= 0.4
        assert np.all(np.diff(run.history) <= CARRIED_EPS * np.finfo(dtype).eps * run.bnorm), "the residual norm grew without M"
        assert true_residual(Dop.dense(), run.x, B[:, c]) <= 1.01 * column_tol(B[:, c], path_rtol(dtype))
        run = minres_twin(Dop, B[:, c], Minv, path_rtol(dtype), 0.0, 200, dtype)
        assert run.status == 0 and with_m[0] <= run.iterations <= with_m[1], (c, run.iterations)
        assert true_residual(Dop.dense(), run.x, B[:, c]) <= 1.01 * column_tol(B[:, c], path_rtol(dtype))


def test_without_m_the_scaled_problem_stagnates():
    D, B, _, _ = runs_of(np.float64)
    run = minres_twin(D, B[:, 0], None, 1e-10, 0.0, 400, np.float64)
    print(f"MRTWIN unpreconditioned order-400 float64: status {run.status}, residual / ||b|| {run.residual / run.bnorm:.2e} after 400 iterations")
    assert run.status == 1 and run.iterations == 400 and run.residual > 1e-4 * run.bnorm


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_status_3_from_an_indefinite_preconditioner(dtype):
    """M = the block inverse of D itself: <v, z> is negative at the start (0 iterations) or after the first Lanczos step"""
    _, _, sets, D, _, B = minres_problem("vbcrs", dtype)
    Minv = exact_minv(D, sets)
    runs = [minres_twin(D, B[:, c], Minv, rtol_of(dtype), 0.0, 200, dtype) for c in range(NB)]
    assert [r.status for r in runs] == [3] * NB
    assert [r.iterations for r in runs] == BROKEN_COUNTS[np.dtype(dtype).name]
    assert all(np.all(np.isfinite(r.x)) for r in runs)


def test_the_other_statuses():
    dtype = np.float64
    D, B, Minv, _ = runs_of(dtype)
    zero = minres_twin(D, np.zeros(NCG), Minv, 1e-10, 0.0, 200, dtype)
    assert (zero.status, zero.iterations, zero.bnorm) == (0, 0, 0.0) and np.all(zero.x == 0)
    bn = B[:, 0].copy()
    bn[17] = np.nan
    nan = minres_twin(D, bn, Minv, 1e-10, 0.0, 200, dtype)
    assert (nan.status, nan.iterations) == (2, 0) and np.all(nan.x == 0)
    cut_short = minres_twin(D, B[:, 0], Minv, 1e-10, 0.0, 5, dtype)
    assert (cut_short.status, cut_short.iterations) == (1, 5)
    # [[0, 1], [1, 0]] with b = e1 breaks CG down (<p, A p> = 0); MINRES solves it in two iterations: delta = 0, but
    # gamma_new = 1, so a1 = 1
    swap = np.array([[0.0, 1.0], [1.0, 0.0]])
    run = minres_twin(swap, np.array([1.0, 0.0]), None, 1e-6, 0.0, 10, dtype)
    assert (run.status, run.iterations) == (0, 2) and run.x.tolist() == [0.0, 1.0] and run.history.tolist() == [1.0, 0.0]
    assert cg_twin(swap, np.array([1.0, 0.0]), None, True, 1e-6, 0.0, 10, dtype).status == 3
    # a1 == 0 needs delta == 0 AND gamma_new == 0: b in the null space of a singular operator
    for order in (1, 2):
        b = np.zeros(order)
        b[0] = 1
        null = minres_twin(np.zeros((order, order)), b, None, 1e-6, 0.0, 10, dtype)
        assert (null.status, null.iterations) == (3, 0) and np.all(null.x == 0) and null.residual == 1.0


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_lost_share_is_beyond_the_spread_bound(dtype):
    """the forms summed without their last tenth (keep): the fourth iterate moves by far more than MARGIN x what permuted
    sums move it by, so the iterate check of test_gpu_minres.py would see a kernel that loses a workgroup's share"""
    D, B, Minv, _ = runs_of(dtype)
    a = minres_twin(D, B[:, 0], Minv, 0.0, 0.0, ITS, dtype)
    sx = 0.0
    for seed in range(8):
        p = minres_twin(D, B[:, 0], Minv, 0.0, 0.0, ITS, dtype, order=np.random.default_rng(seed).permutation(NCG))
        sx = max(sx, deviation(p.x, p.history, a, ITS, dtype)[0])
    lost = minres_twin(D, B[:, 0], Minv, 0.0, 0.0, ITS, dtype, keep=NCG - 40)
    dx = deviation(lost.x, lost.history, a, ITS, dtype)[0]
    print(f"MRTWIN {np.dtype(dtype).name}: spread {sx:.2f} eps max|x|, a lost share {dx:.3g}")
    assert 0 < sx and dx > 100 * MARGIN * sx


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_what_cg_does_on_the_indefinite_problem(dtype):
    """RECORDED, not argued from: on the order-400 indefinite D with the definite sibling's M the twin of CG neither breaks
    down nor stalls -- it reaches the tolerance in MINRES's count (+2 in the complex types).  CG carries no guarantee on an
    indefinite operator (its <p, A p> changes sign; the 2 x 2 case of test_the_other_statuses is a breakdown) and its
    residual norm is not monotone: the largest rise from one iteration to the next is printed"""
    D, B, Minv, runs = runs_of(dtype)
    cg = [cg_twin(D, B[:, c], Minv, True, rtol_of(dtype), 0.0, 100, dtype) for c in range(NB)]
    rise = max(float(np.max(r.history[1:] / r.history[:-1])) for r in cg)
    print(f"MRTWIN cg on the indefinite {np.dtype(dtype).name} problem: statuses {[r.status for r in cg]}, counts {[r.iterations for r in cg]}, "
          f"minres {[r.iterations for r in runs]}, largest rise of ||r|| x{rise:.2f}")
    assert [r.status for r in cg] == [0] * NB
    assert all(0 <= a.iterations - b.iterations <= 2 for a, b in zip(cg, runs))
