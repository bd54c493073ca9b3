"""CPU suite of the LSQR tests' own tools (tests/_lsqr.py) and of what bsm_lsqr_* decides without a device: the twin against
numpy's least-squares / pseudo-inverse solutions, scipy's lsqr and the closed form of the damped problem; the margins the
GPU suite (test_gpu_lsqr.py) relies on -- counts stable to +-1 under permuted sums, true criteria within 1 x their threshold,
so that the GPU suite's factor 2 is one the reference stays inside; a lost share moves the iterate beyond the grid test's
bound; the scalar step of csrc/bsm_lsqr.h (hook bsm_debug_lsqr_step) against the twin's scalars; the refusals of
bsm_lsqr_create that are decided before any device call; the refusals of the Python layer.

The pinned counts.  Consistent, inconsistent and real damped legs reproduce the ranges of the prototype the feature was
specified with (76-79 / 71-73 / 58-60 double, 35-37 / 30-33 / 25-27 single).  The under-determined leg needs 80-84 / 40-44
where that prototype needed 74-78 / 35-38: its right-hand side Bu is this module's own draw (uniform, taken from the
generator after A, Xtrue and Bi), not the prototype's.  The complex damped counts (64; 28-29) have no earlier figure.
rnorm against the true residual norm: 1e-4 relative is asserted for the double types; in single precision the estimate at
convergence sits at the rounding of the recurrences, 1e-4 ||b||, so there 1e-3 ||b|| is allowed on top."""
import numpy as np
import pytest

from _common import NODEV
from _cg import ERR_DEVICE, ERR_INVALID, MAX_RHS
from _jacobi import CODE
from _lockstep import MARGIN, deviation
from _lsqr import (LSQR_ITS, M600, N400, NB, history_unit, lsqr_problem, lsqr_rtol, lsqr_spread, lsqr_twin, orders, raw_lsqr_create, raw_lsqr_step,
                   singular_symmetric, tall_case, true_criteria)

DTYPES = [np.float32, np.float64, np.complex64, np.complex128]
IDS = [np.dtype(d).name for d in DTYPES]
# the twin's iterations on the five columns, rtol = ntol = lsqr_rtol(dtype), maxiter 400
COUNTS = {
    ("float64", "consistent"): [77, 78, 78, 78, 76], ("float64", "inconsistent"): [71, 72, 71, 72, 73],
    ("float64", "under"): [80, 81, 83, 82, 83], ("float64", "damped"): [59, 58, 58, 58, 60],
    ("float32", "consistent"): [35, 36, 37, 35, 37], ("float32", "inconsistent"): [32, 31, 31, 31, 33],
    ("float32", "under"): [44, 40, 43, 41, 41], ("float32", "damped"): [26, 26, 26, 26, 27],
    ("complex128", "consistent"): [78, 79, 79, 77, 77], ("complex128", "inconsistent"): [71, 71, 71, 72, 72],
    ("complex128", "under"): [82, 81, 84, 84, 83], ("complex128", "damped"): [64, 64, 64, 64, 64],
    ("complex64", "consistent"): [37, 37, 38, 36, 37], ("complex64", "inconsistent"): [32, 32, 32, 32, 32],
    ("complex64", "under"): [40, 42, 42, 42, 41], ("complex64", "damped"): [29, 29, 29, 29, 28],
}
LEGS = ["consistent", "inconsistent", "under", "damped"]
_runs = {}


def leg(dtype, which):
    """(operator, B, damp, rule) of one leg of the order-600 x 400 problems"""
    _, A, _, Bc, Bi, Bu = lsqr_problem("vbcrs", dtype)
    return {"consistent": (A, Bc, 0.0, 1), "inconsistent": (A, Bi, 0.0, 2), "under": (A.conj().T, Bu, 0.0, 1), "damped": (A, Bi, 2.0, 2)}[which]


def runs(dtype, which):
    key = (np.dtype(dtype).name, which)
    if key not in _runs:
        A, B, damp, _ = leg(dtype, which)
        r = lsqr_rtol(dtype)
        _runs[key] = [lsqr_twin(A, B[:, c], r, 0.0, r, damp, 400, dtype) for c in range(NB)]
    return _runs[key]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("which", LEGS)
def test_the_twin_solves_the_problems_within_its_thresholds(dtype, which):
    """counts as pinned; the true criterion of the rule the leg ends by, in complex128 with the twin's own anorm, <= 1 x its
    threshold; the solution against numpy's: lstsq (minimum norm for the under-determined leg), the closed form with damp"""
    A, B, damp, rule = leg(dtype, which)
    r = lsqr_rtol(dtype)
    got = runs(dtype, which)
    assert [t.iterations for t in got] == COUNTS[np.dtype(dtype).name, which]
    Aw = A.astype(np.complex128)
    if damp:
        ref = np.linalg.solve(Aw.conj().T @ Aw + damp * damp * np.eye(Aw.shape[1]), Aw.conj().T @ B.astype(np.complex128))
    else:
        ref = np.linalg.pinv(Aw) @ B.astype(np.complex128)
    for c, t in enumerate(got):
        assert t.status == 0
        crit = true_criteria(A, t.x, B[:, c], t.tol, r, t.anorm, damp)
        print(f"LSSTAT {np.dtype(dtype).name} {which} column {c}: criteria / thresholds {crit[0]:.3f} {crit[1]:.3f}")
        assert crit[rule - 1] <= 1.0, (c, crit)
        # rnorm is an estimate of the (damped) residual norm
        rbar = crit[0] * t.tol
        assert abs(t.rnorm - rbar) <= 1e-4 * rbar + (0 if np.finfo(dtype).eps < 1e-10 else 1e-3 * t.bnorm)
        # the distance to the exact solution: the stopping rules bound the residuals, cond(A) ~ 10 carries them to x
        err = np.linalg.norm(t.x - ref[:, c]) / np.linalg.norm(ref[:, c])
        assert err <= 1e3 * r, (c, err)


def test_the_twin_agrees_with_scipy_on_the_real_double_problems():
    sla = pytest.importorskip("scipy.sparse.linalg")
    for which in ("consistent", "inconsistent", "damped"):
        A, B, damp, _ = leg(np.float64, which)
        for c, t in enumerate(runs(np.float64, which)):
            # scipy's first rule is rnorm <= btol ||b|| + atol anorm ||x||: with atol = 0 it is this solver's first rule (and
            # scipy's second rule is off); its second rule with atol in the place of ntol is this solver's second one
            atol = 0.0 if which == "consistent" else 1e-8
            x, istop, itn, r1norm, r2norm, anorm, *_ = sla.lsqr(A, B[:, c], damp=damp, atol=atol, btol=1e-8, conlim=0, iter_lim=400)
            assert abs(t.iterations - itn) <= 1 and istop == (1 if which == "consistent" else 2), (which, c, t.iterations, itn, istop)
            assert np.linalg.norm(t.x - x) <= 1e-6 * np.linalg.norm(x)
        # the estimates after 10 iterations, before two runs that round differently have drifted apart (at the end 2e-3 in
        # anorm and 1e-3 in a residual estimate eight digits below ||b|| were seen)
        t = lsqr_twin(A, B[:, 0], 0.0, 0.0, 0.0, damp, 10, np.float64)
        _, istop, itn, _, r2norm, anorm, _, arnorm, *_ = sla.lsqr(A, B[:, 0], damp=damp, atol=0, btol=0, conlim=0, iter_lim=10)
        assert (istop, itn, t.status, t.iterations) == (7, 10, 1, 10)
        assert abs(anorm - t.anorm) <= 1e-12 * anorm and abs(r2norm - t.rnorm) <= 1e-10 * r2norm and abs(arnorm - t.arnorm) <= 1e-10 * arnorm


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_counts_move_by_at_most_one_under_permuted_sums(dtype):
    r = lsqr_rtol(dtype)
    for which in LEGS:
        A, B, damp, _ = leg(dtype, which)
        base = runs(dtype, which)
        for seed in range(4):
            o = orders(seed, *A.shape)
            for c in (0, 4):
                t = lsqr_twin(A, B[:, c], r, 0.0, r, damp, 400, dtype, order=o)
                assert t.status == 0 and abs(t.iterations - base[c].iterations) <= 1, (which, seed, c, t.iterations, base[c].iterations)


GRID_PINS = [(np.float64, 1025, 40, False, [12, 12, 12]), (np.float64, 1025, 40, True, [14, 14, 14]),
             (np.float32, 4099, 2049, False, [36, 35, 35])]


@pytest.mark.parametrize("dtype, m, n, flip, counts", GRID_PINS, ids=[f"{np.dtype(d).name}-{m}x{n}{'-adjoint' if f else ''}" for d, m, n, f, _ in GRID_PINS])
def test_grid_problems_counts_spread_and_a_lost_share(dtype, m, n, flip, counts):
    """the block-built operators of the grid test: the twin's counts; the spread after LSQR_ITS iterations is small; a twin that
    loses the last 16-byte groups' share of a norm (m side, then n side) leaves MARGIN x spread"""
    _, op, B, Bt = tall_case(m, n, dtype)
    op, B = (op.H, Bt) if flip else (op, B)
    r = lsqr_rtol(dtype)
    assert [lsqr_twin(op, B[:, c], r, 0.0, r, 0.0, 200, dtype).iterations for c in range(3)] == counts
    sx, sh = lsqr_spread(op, B[:, 0], LSQR_ITS, dtype)
    ref = lsqr_twin(op, B[:, 0], 0.0, 0.0, 0.0, 0.0, LSQR_ITS, dtype)
    print(f"LSSTAT grid {np.dtype(dtype).name} {op.shape}: spread {sx:.2f} eps max|x|, {sh:.2e} eps ||b||")
    assert 0 < sx < 200
    rows, cols = op.shape
    for keep in ((rows - rows // 8, None), (None, cols - max(cols // 8, 1))):
        lost = lsqr_twin(op, B[:, 0], 0.0, 0.0, 0.0, 0.0, LSQR_ITS, dtype, keep=keep)
        dx, dh = deviation(lost.x, lost.history, ref, LSQR_ITS, dtype)
        assert dx > MARGIN * sx or dh > MARGIN * history_unit(sh), (keep, dx, sx, dh, sh)  # the bound the GPU suite uses


def test_the_singular_symmetric_problem_keeps_its_counts():
    D, B = singular_symmetric()
    assert np.linalg.matrix_rank(D) == 30
    for seed in [None, 0, 1, 2, 3]:
        o = None if seed is None else orders(seed, 40, 40)
        runs = [lsqr_twin(D, B[:, c], 1e-8, 0.0, 1e-8, 0.0, 100, np.float64, order=o) for c in range(3)]
        assert [t.iterations for t in runs] == [24, 23, 23] and all(t.status == 0 for t in runs)
        assert all(true_criteria(D, t.x, B[:, c], t.tol, 1e-8, t.anorm)[0] <= 1 for c, t in enumerate(runs))


# ---- the scalar step (csrc/bsm_lsqr.h: lsqr_step, compiled for host and device) ---------------------------------------------
def test_the_scalar_step_follows_the_twin_on_a_recorded_run():
    for which in ("consistent", "inconsistent", "damped"):
        _, _, damp, _ = leg(np.float64, which)
        t = runs(np.float64, which)[0]
        assert len(t.steps) == t.iterations
        for before, bn, an, after, status in t.steps:
            out, st = raw_lsqr_step(before, bn, an, damp, t.tol, lsqr_rtol(np.float64))
            assert st == status
            assert np.all(np.abs(out - np.array(after)) <= 4 * np.finfo(np.float64).eps * np.abs(after))


def test_the_scalar_step_at_its_edges():
    s = [2.0, 3.0, 3.0, 2.0, 0.0, 1.0]  # alpha, beta, phibar, rhobar, res2, anorm
    # beta' = 0 (and with it alpha' = 0): the Krylov space ended -- status 0, phibar = 0, no NaN
    out, st = raw_lsqr_step(s, 0.0, 0.0, 0.0, 1e-30, 0.0)
    assert st == 0 and np.all(np.isfinite(out)) and out[2] == 0 and out[6] == 3.0 / 2.0 and out[7] == 0 and out[8] == 0
    # alpha' = 0 with beta' > 0: status 0 by the second rule's arnorm = 0 even with ntol = 0, x still takes its step
    out, st = raw_lsqr_step(s, 1.0, 0.0, 0.0, 1e-30, 0.0)
    rho = np.sqrt(5.0)
    assert st == 0 and out[9] == 0 and abs(out[6] - (2 / rho) * 3 / rho) < 1e-15 and out[7] == 0 and abs(out[8] - 3 / rho) < 1e-15
    # everything zero: no division by zero is executed
    out, st = raw_lsqr_step([0.0] * 6, 0.0, 0.0, 0.0, 0.0, 0.0)
    assert st == 0 and np.all(out == 0)
    # damp > 0: the first rotation leaves psi in res2, rnorm^2 = phibar^2 + res2, anorm takes damp^2
    out, st = raw_lsqr_step(s, 1.0, 1.5, 2.0, 1e-30, 0.0)
    rb1 = np.sqrt(8.0)
    psi, pb1 = (2 / rb1) * 3, (2 / rb1) * 3
    rho = np.sqrt(9.0)
    assert st == -1 and abs(out[4] - psi * psi) < 1e-14 and abs(out[2] - (1 / rho) * pb1) < 1e-15
    assert abs(out[5] - np.sqrt(1 + 4 + 1 + 4)) < 1e-15 and abs(out[8] - np.sqrt(out[2] ** 2 + out[4])) < 1e-15
    assert abs(out[3] + (rb1 / rho) * 1.5) < 1e-15
    # the rules in their order: within tol -> 0;  the second rule -> 0
    assert raw_lsqr_step(s, 1.0, 1.5, 0.0, 10.0, 0.0)[1] == 0
    assert raw_lsqr_step(s, 1.0, 1.5, 0.0, 0.0, 1e3)[1] == 0 and raw_lsqr_step(s, 1.0, 1.5, 0.0, 0.0, 1e-3)[1] == -1
    # a NaN or an infinity anywhere: status 2
    assert raw_lsqr_step(s, float("nan"), 1.0, 0.0, 10.0, 10.0)[1] == 2
    assert raw_lsqr_step(s, 1.0, float("nan"), 0.0, 10.0, 10.0)[1] == 2
    assert raw_lsqr_step(s, float("inf"), 1.0, 0.0, 10.0, 10.0)[1] == 2


# ---- refusals decided before any device call -----------------------------------------------------------------------------------
def test_create_refusals_without_a_device(bsm):
    p, *_ = lsqr_problem("vbcrs", np.float64)
    A = bsm.synthetic.build(p, device=NODEV)
    from bsm_amd import _lib as L
    cases = [((None, 0, CODE[np.dtype(np.float64)], 1), ERR_INVALID, "null handle"), ((A, 3, CODE[np.dtype(np.float64)], 1), ERR_INVALID, "bad op"),
             ((A, 0, 4, 1), ERR_INVALID, "vdtype"), ((A, 0, CODE[np.dtype(np.float64)], 0), ERR_INVALID, "nrhs_max"),
             ((A, 0, CODE[np.dtype(np.float64)], MAX_RHS + 1), ERR_INVALID, "nrhs_max"),
             ((A, 0, CODE[np.dtype(np.float32)], 1), ERR_INVALID, "vector type"), ((A, 0, CODE[np.dtype(np.float64)], 1), ERR_DEVICE, "no device image")]
    for args, code, word in cases:
        rc, out = raw_lsqr_create(*args)
        assert rc == code and not out.value, (args[1:], rc, out.value)
        assert word in L.lib().bsm_last_error().decode(), (word, L.lib().bsm_last_error())
    assert L.lib().bsm_lsqr_create(A._h.ptr, 0, 1, 1, None) == ERR_INVALID
    # op T on a complex handle: conj(A) is offered by no product
    pc, *_ = lsqr_problem("vbcrs", np.complex128)
    rc, out = raw_lsqr_create(bsm.synthetic.build(pc, device=NODEV), 1, CODE[np.dtype(np.complex128)], 1)
    assert rc == -2 and not out.value and "conj(A)" in L.lib().bsm_last_error().decode()


def test_python_refusals_without_a_device(bsm):
    p, A, _, Bc, _, Bu = lsqr_problem("vbcrs", np.float64)
    H = bsm.synthetic.build(p, device=NODEV)
    with pytest.raises(RuntimeError, match="no device image"):
        bsm.Lsqr(H, nrhs=2)
    with pytest.raises(TypeError, match="not a supported vector type"):
        bsm.Lsqr(H, dtype=np.int32)
    assert "Lsqr" not in bsm.solvers.__all__ and bsm.Lsqr is bsm.solvers.Lsqr and bsm.lsqr is bsm.solvers.lsqr


class _Shape(object):
    """a solver object as far as _prelude needs one: the Python-side checks of solve() run before any library call"""


def test_solve_checks_the_two_lengths(bsm):
    S = bsm.Lsqr.__new__(bsm.Lsqr)
    S.dtype, S.nb, S.n, S.nrhs, S._base, S._ptr = np.dtype(np.float64), M600, N400, 3, None, None
    B = np.zeros((M600, 2), order="F")
    with pytest.raises(ValueError, match="DimensionMismatch"):
        S.solve(np.zeros((N400, 2), order="F"))  # B with the rows of X
    with pytest.raises(ValueError, match="DimensionMismatch"):
        S.solve(B, X=np.zeros((M600, 2), order="F"))  # X with the rows of B
    with pytest.raises(ValueError, match="columns"):
        S.solve(np.zeros((M600, 4), order="F"))  # more columns than nrhs
    with pytest.raises(ValueError, match="different numbers of columns"):
        S.solve(B, X=np.zeros((N400, 1), order="F"))
    with pytest.raises(TypeError):
        S.solve(B.astype(np.float32))
    with pytest.raises(TypeError, match="X0 must have the shape"):
        S.solve(B, X0=np.zeros((M600, 2), order="F"))
    with pytest.raises(TypeError, match="X0 must have the shape"):
        S.solve(B, X0=np.zeros((N400, 2), dtype=np.float32, order="F"))
