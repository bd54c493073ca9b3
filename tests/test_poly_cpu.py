"""CPU suite of the polynomial preconditioners (bsm_poly_create, PolynomialPreconditioner): the Chebyshev coefficients against
the same recurrence in exact rational arithmetic, the residual-polynomial identity that pins the recurrence itself, the numpy
twin of tests/_poly.py on dense examples, the twin together with the CG twin (the iteration counts the GPU suite then asks of
the device), the core of lanczos_bounds on numpy, every refusal of create that is decided before a device is touched, the
refusals of the Python constructors and the ctypes prototypes."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from _cg import cg_problem, cg_twin, exact_minv
from _common import NODEV
from _jacobi import CODE, uniform
from _poly import (ERR_DEVICE, ERR_INVALID, MAX_STEPS, chebyshev_exact, chebyshev_t, dense_poly, neumann_coefficients, poly_twin,
                   raw_destroy, raw_poly_create, residual_polynomial)

RATIOS = [2, 30, 1000]
LMIN = Fraction(3, 8)  # dyadic, and so is every lmax = ratio * lmin: the float arguments are the exact ones
F64 = CODE[np.dtype(np.float64)]


# ---- the coefficients -----------------------------------------------------------------------------------------------------
def test_chebyshev_coefficients_against_exact_arithmetic(bsm):
    """float64 against Fractions for steps = 1 .. 16 and lmax / lmin in {2, 30, 1000}.  Observed: the largest relative
    deviation of any coefficient is 1.39e-15 (6.3 eps, at lmax / lmin = 1000, where 2 sigma - rho_k cancels); asserted: 4 x
    that."""
    worst = Fraction(0)
    for ratio in RATIOS:
        for steps in range(1, 17):
            a, b = bsm.chebyshev_coefficients(float(LMIN), float(LMIN * ratio), steps)
            ea, eb = chebyshev_exact(LMIN, LMIN * ratio, steps)
            assert a.shape == b.shape == (steps,) and a.dtype == b.dtype == np.float64 and a[0] == 0
            for k in range(steps):
                worst = max(worst, abs(Fraction(b[k]) - eb[k]) / eb[k], abs(Fraction(a[k]) - ea[k]) / ea[k] if k else 0)
    print(f"POLYSTAT chebyshev coefficients: largest relative deviation {float(worst):.3e}")
    assert worst <= 4 * 1.39e-15


@pytest.mark.parametrize("ratio", RATIOS)
def test_residual_polynomial_is_the_scaled_chebyshev_polynomial(ratio):
    """1 - lambda p(lambda) = T_s((theta - lambda) / delta) / T_s(sigma) on 200 points of [lmin, lmax], both sides in exact
    rational arithmetic: the recurrence itself, not its float evaluation"""
    lmin, lmax = LMIN, LMIN * ratio
    theta, delta = (lmax + lmin) / 2, (lmax - lmin) / 2
    for steps in (1, 2, 3, 5, 8, 16):
        a, b = chebyshev_exact(lmin, lmax, steps)
        ts = chebyshev_t(steps, theta / delta)
        for i in range(200):
            lam = lmin + (lmax - lmin) * Fraction(i, 199)
            assert residual_polynomial(a, b, lam) == chebyshev_t(steps, (theta - lam) / delta) / ts, (steps, i)


def test_chebyshev_coefficients_refusals(bsm):
    for args in [(0.0, 1.0, 2), (-1.0, 1.0, 2), (1.0, 1.0, 2), (2.0, 1.0, 2), (0.5, 1.0, 0), (0.5, float("inf"), 2), (float("nan"), 1.0, 2)]:
        with pytest.raises(ValueError, match="0 < lmin < lmax"):
            bsm.chebyshev_coefficients(*args)


# ---- the twin on a dense example ------------------------------------------------------------------------------------------------
def dense40():
    rng = np.random.default_rng(9100)
    n = 40
    T = uniform(rng, (n, n), np.float64)
    A = T.T @ T / n + np.eye(n)
    Dinv = np.diag(1 / np.diag(A)) + 0.01 * (lambda W: (W + W.T) / 2)(uniform(rng, (n, n), np.float64))
    return n, A, Dinv


def test_one_chebyshev_step_is_the_inner_preconditioner_over_theta(bsm):
    n, A, Dinv = dense40()
    a, b = bsm.chebyshev_coefficients(0.5, 2.5, 1)
    got = poly_twin(A, Dinv, a, b, np.eye(n), np.float64)
    # b_0 = 1 / theta is rounded once, the scaling of every entry once more
    assert np.max(np.abs(got - Dinv / 1.5)) <= 2 * np.finfo(np.float64).eps * np.max(np.abs(Dinv))
    assert np.array_equal(poly_twin(A, None, a, b, np.eye(n), np.float64), b[0] * np.eye(n))  # without D: I / theta


@pytest.mark.parametrize("steps", [1, 2, 3, 5])
def test_neumann_is_the_truncated_series(steps):
    """omega sum_{k < s} (I - omega D A)^k D.  Bound: s products with A and s with D, each a sum of n terms (n eps of the sum
    of the magnitudes), on vectors no larger than `scale` -- the size of D's columns times the growth of one step"""
    n, A, Dinv = dense40()
    omega = 0.8
    E = np.eye(n) - omega * Dinv @ A
    assert np.max(np.abs(np.linalg.eigvals(E))) < 1
    want = omega * sum(np.linalg.matrix_power(E, k) for k in range(steps)) @ Dinv
    got = poly_twin(A, Dinv, *neumann_coefficients(omega, steps), np.eye(n), np.float64)
    scale = np.max(np.abs(Dinv)) * (1 + omega * np.linalg.norm(np.abs(Dinv) @ np.abs(A), np.inf))
    err = np.max(np.abs(got - want))
    print(f"POLYSTAT neumann dense s={steps}: error {err:.3e}, bound {4 * steps * n * np.finfo(np.float64).eps * scale:.3e}")
    assert err <= 4 * steps * n * np.finfo(np.float64).eps * scale
    # and the dense form a solver's twin takes is the same map
    assert np.max(np.abs(dense_poly(A, Dinv, *neumann_coefficients(omega, steps)) - want)) <= 4 * steps * n * np.finfo(np.float64).eps * scale


def test_twin_takes_matrices_column_by_column_and_permuted_orders():
    n, A, Dinv = dense40()
    rng = np.random.default_rng(9101)
    R = np.asfortranarray(uniform(rng, (n, 3), np.float32))
    a, b = neumann_coefficients(0.8, 3)
    Y = poly_twin(A, Dinv, a, b, R, np.float32)
    assert Y.dtype == np.float32 and Y.shape == (n, 3)
    for c in range(3):
        assert np.array_equal(Y[:, c], poly_twin(A, Dinv, a, b, R[:, c], np.float32))
    Yp = poly_twin(A, Dinv, a, b, R, np.float32, order=rng.permutation(n))
    assert not np.array_equal(Y, Yp) and np.max(np.abs(Y - Yp)) <= 64 * np.finfo(np.float32).eps * np.max(np.abs(Y))


# ---- the twin and the CG twin together ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cg400():
    p, sets, D, B = cg_problem("vbcrs", np.float64)
    Minv = exact_minv(D, sets)
    ev = np.linalg.eigvals(Minv @ D).real
    return D, B, Minv, float(ev.min()), float(ev.max())


@pytest.mark.parametrize("steps, count", [(1, 20), (2, 10), (4, 6), (8, 3)])
def test_cg_counts_with_the_chebyshev_polynomial(bsm, cg400, steps, count):
    """CG on the suite's order-400 problem to rtol 1e-8 with M = p(A) over the exact block-Jacobi D and [0.95 lmin, 1.05 lmax]
    of D A: 20 iterations with D alone (steps = 1 is D / theta), 10, 6, 3 with 2, 4, 8 steps -- and the same under the 8
    permuted summation orders of _lockstep.spread's seeds, so that the GPU suite may ask +-1 of the device"""
    D, B, Minv, lmin, lmax = cg400
    assert abs(lmin - 0.364) < 5e-4 and abs(lmax - 1.624) < 5e-4
    P = dense_poly(D, Minv, *bsm.chebyshev_coefficients(0.95 * lmin, 1.05 * lmax, steps))
    for c in range(2):
        assert cg_twin(D, B[:, c], P, True, 1e-8, 0.0, 100, np.float64).iterations == count
        for seed in range(8):
            o = np.random.default_rng(seed).permutation(len(D))
            assert cg_twin(D, B[:, c], P, True, 1e-8, 0.0, 100, np.float64, order=o).iterations == count, (c, seed)
    if steps == 1:
        assert cg_twin(D, B[:, 0], Minv, True, 1e-8, 0.0, 100, np.float64).iterations == count


# ---- lanczos_bounds on numpy ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype, herm", [(np.float64, False), (np.float32, False), (np.complex128, True)], ids=["float64", "float32", "complex128-herm"])
def test_lanczos_bounds_core_on_numpy(bsm, dtype, herm):
    """the extreme Ritz values of D A lie inside its spectrum (1e-10 relative for rounding), and after 20 steps the widened
    interval [0.95 lo, 1.05 hi] contains it"""
    from bsm_amd.solvers import _lanczos_ritz
    p, sets, D, B = cg_problem("vbcrs", dtype, herm)
    Minv = exact_minv(D, sets)
    ev = np.linalg.eigvals(Minv.astype(np.complex128) @ D.astype(np.complex128)).real
    lmin, lmax = float(ev.min()), float(ev.max())
    v0 = np.random.default_rng(0).uniform(-1, 1, len(D)).astype(dtype)
    for steps in (3, 20):
        lo, hi = _lanczos_ritz(lambda v: (D @ v).astype(dtype), lambda v: (Minv @ v).astype(dtype), v0, steps, np)
        print(f"POLYSTAT lanczos {np.dtype(dtype).name} steps={steps}: lo / lmin {lo / lmin:.4f}, hi / lmax {hi / lmax:.4f}")
        assert lmin * (1 - 1e-10) <= lo <= hi <= lmax * (1 + 1e-10)
    assert 0.95 * lo <= lmin and 1.05 * hi >= lmax and lo / lmin <= 1.007 and hi / lmax >= 0.998
    # without D: the spectrum of A itself
    ea = np.linalg.eigvalsh(D.astype(np.complex128))
    lo, hi = _lanczos_ritz(lambda v: (D @ v).astype(dtype), lambda v: v, v0, 20, np)
    assert ea[0] * (1 - 1e-10) <= lo <= hi <= ea[-1] * (1 + 1e-10)
    with pytest.raises(ValueError, match="positive"):
        _lanczos_ritz(lambda v: v, lambda v: v, np.zeros(4), 3, np)


# ---- refusals decided before any device call -----------------------------------------------------------------------------------
def test_create_refusals_without_a_device(bsm):
    from bsm_amd import _lib as L
    p, sets, D, B = cg_problem("vbcrs", np.float64)
    A = bsm.synthetic.build(p, device=NODEV)
    Dj = bsm.block_jacobi(A, sets)
    A32 = bsm.synthetic.build(cg_problem("vbcrs", np.float32)[0], device=NODEV)
    small = bsm.BlockSparseMatrix([np.eye(2)], [[1, 2]], [[1, 2]], (2, 2), device=NODEV)
    wide = bsm.BlockSparseMatrix([np.ones((2, 3))], [[1, 2]], [[1, 2, 3]], (2, 3), device=NODEV)
    one, nan, inf = [0.0, 0.5], [0.0, float("nan")], [float("inf"), 0.5]
    cases = [((None, 0, None, 0, F64, 1, one, one), ERR_INVALID, "null handle"),
             ((A, 3, None, 0, F64, 1, one, one), ERR_INVALID, "bad op"),
             ((A, 0, Dj, -1, F64, 1, one, one), ERR_INVALID, "bad op"),
             ((A, 0, None, 7, F64, 1, one, one), ERR_DEVICE, "no device image"),  # opD without D is not looked at
             ((A, 0, None, 0, 4, 1, one, one), ERR_INVALID, "vdtype"),
             ((A, 0, None, 0, F64, 1, [], []), ERR_INVALID, "steps outside"),
             ((A, 0, None, 0, F64, 1, [0.0] * (MAX_STEPS + 1), [1.0] * (MAX_STEPS + 1)), ERR_INVALID, "steps outside"),
             ((A, 0, None, 0, F64, 1, None, one), ERR_INVALID, "null coefficient"),
             ((A, 0, None, 0, F64, 1, one, None, 2), ERR_INVALID, "null coefficient"),
             ((A, 0, None, 0, F64, 1, one, nan), ERR_INVALID, "not finite"),
             ((A, 0, None, 0, F64, 1, nan, one), ERR_INVALID, "not finite"),
             ((A, 0, None, 0, F64, 1, one, inf), ERR_INVALID, "not finite"),
             ((A, 0, None, 0, F64, 1, inf, one), ERR_DEVICE, "no device image"),  # a[0] is ignored
             ((A, 0, None, 0, F64, 0, one, one), ERR_INVALID, "nrhs_max"),
             ((A, 0, None, 0, F64, 17, one, one), ERR_INVALID, "nrhs_max"),
             ((A, 0, None, 0, F64, 17, one, nan), ERR_INVALID, "not finite"),  # the coefficients come before nrhs_max
             ((A, 3, None, 0, 4, 0, [], []), ERR_INVALID, "bad op"),  # ... and the op before everything but A
             ((wide, 0, None, 0, F64, 1, one, one), ERR_INVALID, "not square"),
             ((A, 0, small, 0, F64, 1, one, one), ERR_INVALID, "another order"),
             ((A32, 0, None, 0, F64, 1, one, one), ERR_INVALID, "vector type"),
             ((A, 0, None, 0, CODE[np.dtype(np.float32)], 1, one, one), ERR_INVALID, "vector type"),
             ((A, 0, None, 0, F64, 16, one, one), ERR_DEVICE, "no device image"),
             ((A, 0, Dj, 0, CODE[np.dtype(np.complex128)], 16, one, one), ERR_DEVICE, "no device image")]  # a real pair under complex vectors
    for args, code, word in cases:
        rc, out = raw_poly_create(*args)
        assert rc == code and not out.value, (args[1:], rc, out.value, L.lib().bsm_last_error())
        assert word in L.lib().bsm_last_error().decode(), (word, L.lib().bsm_last_error())
    assert raw_poly_create(A, 0, None, 0, F64, 1, one, one, want_out=False)[0] == ERR_INVALID
    # bsm_poly_info is for composed handles
    steps, ws = C.c_int32(-1), C.c_int64(-1)
    assert L.lib().bsm_poly_info(A._h.ptr, C.byref(steps), None, None, C.byref(ws)) == ERR_INVALID
    assert "not a composed handle" in L.lib().bsm_last_error().decode()
    assert L.lib().bsm_poly_info(None, C.byref(steps), None, None, C.byref(ws)) == ERR_INVALID and steps.value == -1
    assert raw_destroy(None) == 0


def test_python_refusals_without_a_device(bsm):
    p, sets, D, B = cg_problem("vbcrs", np.float64)
    A = bsm.synthetic.build(p, device=NODEV)
    wide = bsm.BlockSparseMatrix([np.ones((2, 3))], [[1, 2]], [[1, 2, 3]], (2, 3), device=NODEV)
    with pytest.raises(RuntimeError, match="no device image"):
        bsm.neumann(A, 0.8, 3)
    with pytest.raises(RuntimeError, match="no device image"):
        bsm.chebyshev(A, 0.3, 1.7, 4, D=bsm.block_jacobi(A, sets))
    with pytest.raises(TypeError, match="A must be a block matrix"):
        bsm.polynomial(D, [0.0], [1.0])
    with pytest.raises(TypeError, match="D must be a block matrix"):
        bsm.polynomial(A, [0.0], [1.0], D=D)
    with pytest.raises(TypeError, match="not a supported vector type"):
        bsm.polynomial(A, [0.0], [1.0], dtype=np.int32)
    with pytest.raises(ValueError, match="same length"):
        bsm.polynomial(A, [0.0, 0.0], [1.0])
    with pytest.raises(ValueError, match="same length"):
        bsm.polynomial(A, [], [])
    with pytest.raises(ValueError, match="same length"):
        bsm.polynomial(A, np.zeros(MAX_STEPS + 1), np.ones(MAX_STEPS + 1))
    with pytest.raises(ValueError, match="finite"):
        bsm.polynomial(A, [0.0, 0.0], [1.0, float("nan")])
    with pytest.raises(ValueError, match="square"):
        bsm.polynomial(wide, [0.0], [1.0])
    with pytest.raises(ValueError, match="0 < lmin < lmax"):
        bsm.chebyshev(A, 2.0, 1.0, 3)
    with pytest.raises(ValueError, match="steps >= 1"):
        bsm.neumann(A, 0.8, 0)
    with pytest.raises(ValueError, match="finite omega"):
        bsm.neumann(A, float("nan"), 2)
    with pytest.raises(ValueError, match="device image"):
        bsm.lanczos_bounds(A)
    with pytest.raises(TypeError, match="must be a block matrix"):
        bsm.lanczos_bounds(D)
    # exported by the package by name; the star-import set stays as it was
    for name in ("PolynomialPreconditioner", "polynomial", "chebyshev", "neumann", "chebyshev_coefficients", "lanczos_bounds"):
        assert name not in bsm.solvers.__all__ and getattr(bsm, name) is getattr(bsm.solvers, name)
    assert issubclass(bsm.PolynomialPreconditioner, bsm.AbstractBlockMatrix)


def test_ctypes_prototypes(bsm):
    from bsm_amd import _lib as L
    lib = L.lib()
    dp, vp = C.POINTER(C.c_double), C.c_void_p
    assert lib.bsm_poly_create.argtypes == [vp, C.c_int, vp, C.c_int, C.c_int, C.c_int32, C.c_int32, dp, dp, C.POINTER(vp)]
    assert lib.bsm_poly_info.argtypes == [vp, C.POINTER(C.c_int32), dp, dp, C.POINTER(C.c_int64)]
    assert lib.bsm_poly_create.restype == lib.bsm_poly_info.restype == C.c_int
    assert L.BSM_POLY_MAX_STEPS == MAX_STEPS == 64 and {"bsm_poly_create", "bsm_poly_info"} <= set(L.EXPORTS)
