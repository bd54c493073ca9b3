"""CPU suite of the eigsh grid cases (no GPU): what test_gpu_eigsh_grid.py takes for granted.  The orders of
_eigsh.grid_sizes put 2 and 3 workgroups on a vector under the grid rule (_lockstep.krylov_grid, the mirror of krylov_grid in
csrc/bsm_krylov.h); the grid problems meet their premises; the numpy twin converges on every (type, n, case) the GPU module
runs, against the spectrum of the blocks as stored, with its cycle counts pinned -- the device's count is compared with them
(<= twin + 1), and a case that is there for its restarts must restart --; the twin of the single types at the loose tolerance
and the share of the last row range in its residuals; the twin on the shifted operator of the side-stream test; and the twin
at ncv == n on the order-12 operator."""
import numpy as np
import pytest

from _eigsh import (BATCH_CASES, DTYPES, GRID_CASES, HIGH, HIGH40, LOOSE_CASE, LOOSE_RTOL, LOOSE_TYPES, LOW, SPECTRA, all_grid_cases, check_pairs,
                    eig_rtol, eigsh_twin, grid_id, grid_problem, grid_sizes, grid_twin, tridiagonal_block, wanted_reference)
from _gpu import TOL
from _krylov import wide_of
from _lockstep import krylov_grid

name = lambda d: np.dtype(d).name  # noqa: E731

SIZES = {"complex128": (513, 1027), "float64": (1025, 2051), "complex64": (1025, 2051), "float32": (2049, 4099)}


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
def test_the_sizes_give_two_and_three_workgroups(dtype):
    es = np.dtype(dtype).itemsize
    n2, n3 = grid_sizes(dtype)
    assert (n2, n3) == SIZES[name(dtype)]
    assert krylov_grid(n2, es) == 2 and krylov_grid(n3, es) == 3
    assert krylov_grid(n2 - 1, es) == 1 and krylov_grid(n3 - 3, es) == 2  # one row range less without the rows added
    assert n3 % 2 == 1  # the workspace's leading dimension (whole 16-byte groups) differs from n wherever an element is under 16 bytes
    assert ((n3 * es + 15) // 16 * 16 // es != n3) == (es < 16)


def test_the_spectra_meet_their_premises():
    assert len(HIGH40) == 40 and HIGH40[0] == HIGH[0] == 3.0 and np.allclose(np.diff(HIGH40), 0.4)
    assert len(SPECTRA["high20"][0]) == 20 and len({base for _, base in SPECTRA.values()}) == 3
    # every case with more than 5 wanted pairs wants fewer than there are outliers above the bulk
    assert all(nev < len(SPECTRA[spec][0]) for nev, _, which, spec in BATCH_CASES if which == "LA")
    assert all(nev <= 5 for nev, _, _ in GRID_CASES)


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
def test_the_grid_problems_meet_their_premises(dtype):
    eps = float(np.finfo(dtype).eps)
    for n in grid_sizes(dtype):
        for spec in (("high", "high20", "high40") if n == grid_sizes(dtype)[0] else ("high",)):
            p, Dop, ref, v0 = grid_problem(dtype, n, spec)
            high = SPECTRA[spec][0]
            assert len(Dop) == n == len(ref) == len(v0) and Dop.dtype == np.dtype(dtype) == v0.dtype and p["size"] == (n, n)
            assert Dop.main.shape == (n // 8, 8, 8) and Dop.tail.shape == (n % 8, n % 8) and n % 8
            assert np.array_equal(Dop.main, Dop.main.conj().transpose(0, 2, 1)) and np.array_equal(Dop.tail, Dop.tail.conj().T)
            assert len(p["blocks"]) == n // 8 + 1 and all(np.array_equal(b, Dop.main[i]) for i, b in enumerate(p["blocks"][:-1]))
            assert np.array_equal(p["blocks"][-1], Dop.tail) and p["rowstart"][-1] == n // 8 * 8 + 1
            # the stored blocks have the designed spectrum to the precision of the type (blocks of order 8, ||A|| = high[-1])
            assert np.max(np.abs(ref[:5] - LOW)) <= 8 * eps * high[-1] and np.max(np.abs(ref[-len(high):] - high)) <= 8 * eps * high[-1]
            assert ref[5] >= 1 - 8 * eps * high[-1] and ref[-len(high) - 1] <= 2 + 8 * eps * high[-1]
            # products with a vector and with a matrix against the dense form, and the operator's shifted sibling
            D = Dop.dense()
            X = np.stack([v0, v0[::-1]], axis=1)
            assert np.allclose(Dop @ v0, D @ v0, rtol=0, atol=64 * eps) and np.allclose(Dop @ X, D @ X, rtol=0, atol=64 * eps)
            assert np.array_equal(Dop.shifted(2.5).dense(), (D + 2.5 * np.eye(n)).astype(dtype))
            if n <= 1027:
                # block by block is the spectrum of the whole
                assert np.max(np.abs(np.linalg.eigvalsh(D.astype(wide_of(dtype))) - ref)) <= n * np.finfo(np.float64).eps * high[-1]


# cycles of the twin at eig_rtol from the problem's v0, per case id (_eigsh.grid_id): what test_gpu_eigsh_grid.py compares the
# device's counts with (<= twin + 1)
TWIN_CYCLES = {
    "float32-n2049-5of12-LA-high": 4,
    "float32-n2049-5of12-BE-high": 3,
    "float32-n2049-3of8-LM-high": 6,
    "float32-n2049-1of3-SA-high": 26,
    "float32-n4099-5of12-LA-high": 4,
    "float32-n4099-5of12-BE-high": 3,
    "float32-n4099-3of8-LM-high": 7,
    "float32-n4099-1of3-SA-high": 29,
    "float32-n2049-17of24-LA-high20": 5,
    "float32-n2049-33of48-LA-high40": 3,
    "float32-n2049-33of40-LA-high40": 8,
    "float64-n1025-5of12-LA-high": 8,
    "float64-n1025-5of12-BE-high": 5,
    "float64-n1025-3of8-LM-high": 9,
    "float64-n1025-1of3-SA-high": 53,
    "float64-n2051-5of12-LA-high": 8,
    "float64-n2051-5of12-BE-high": 4,
    "float64-n2051-3of8-LM-high": 11,
    "float64-n2051-1of3-SA-high": 52,
    "float64-n1025-17of24-LA-high20": 8,
    "float64-n1025-33of48-LA-high40": 4,
    "float64-n1025-33of40-LA-high40": 11,
    "complex64-n1025-5of12-LA-high": 4,
    "complex64-n1025-5of12-BE-high": 3,
    "complex64-n1025-3of8-LM-high": 5,
    "complex64-n1025-1of3-SA-high": 24,
    "complex64-n2051-5of12-LA-high": 4,
    "complex64-n2051-5of12-BE-high": 3,
    "complex64-n2051-3of8-LM-high": 6,
    "complex64-n2051-1of3-SA-high": 27,
    "complex64-n1025-17of24-LA-high20": 5,
    "complex64-n1025-33of48-LA-high40": 3,
    "complex64-n1025-33of40-LA-high40": 7,
    "complex128-n513-5of12-LA-high": 8,
    "complex128-n513-5of12-BE-high": 4,
    "complex128-n513-3of8-LM-high": 11,
    "complex128-n513-1of3-SA-high": 56,
    "complex128-n1027-5of12-LA-high": 8,
    "complex128-n1027-5of12-BE-high": 5,
    "complex128-n1027-3of8-LM-high": 11,
    "complex128-n1027-1of3-SA-high": 51,
    "complex128-n513-17of24-LA-high20": 8,
    "complex128-n513-33of48-LA-high40": 3,
    "complex128-n513-33of40-LA-high40": 10,
    "float64-n2051-5of12-LM-high": 6,
}
# the cases that are there for their restarts (every case but the 33-of-48 one, which is there for its three residual batches)
RESTARTING = [c for c in all_grid_cases() if (c[2], c[3]) != (33, 48)]


@pytest.mark.parametrize("case", all_grid_cases(), ids=grid_id)
def test_twin_on_the_grid_problems(case):
    dtype, n, nev, ncv, which, spec = case
    eps = float(np.finfo(dtype).eps)
    _, Dop, ref, _ = grid_problem(dtype, n, spec)
    r = grid_twin(*case)
    assert r.status == 0 and r.nconv == nev and r.X.shape == (n, nev)
    tol = eig_rtol(dtype) * r.anorm
    assert np.all(r.estimate <= tol)
    assert r.anorm <= np.max(np.abs(ref)) * (1 + n * eps)
    gap = check_pairs(r.value, r.estimate, r.residual, r.anorm, ref, which, tol, dtype, f"twin {grid_id(case)}")
    print(f"EIGSTAT twin {grid_id(case)}: cycles {r.cycles} steps {r.steps} gap / (eps anorm) {gap:.2f} of {n + ncv + 2} orth / eps {r.orth / eps:.1f}")
    assert gap <= n + ncv + 2
    assert r.orth > 0  # (8 x this is the device's bound)
    assert r.cycles == TWIN_CYCLES[grid_id(case)], (grid_id(case), r.cycles)
    if case in RESTARTING:
        assert r.cycles >= 3, "this case is there for its restarts"


def test_every_case_has_its_pinned_count():
    assert sorted(TWIN_CYCLES) == sorted(grid_id(c) for c in all_grid_cases())
    # the figures of the design: (1, 3) restarts 20 .. 60 times, the many-pair cases a few times
    for c in all_grid_cases():
        lo, hi = {(1, 3): (20, 60), (33, 48): (2, 4)}.get((c[2], c[3]), (3, 14))
        assert lo <= TWIN_CYCLES[grid_id(c)] <= hi, grid_id(c)


LOOSE_CYCLES = {"float32-n2049": 3, "float32-n4099": 4, "complex64-n1025": 3, "complex64-n2051": 3}


@pytest.mark.parametrize("dtype", LOOSE_TYPES, ids=name)
def test_twin_at_the_loose_tolerance(dtype):
    """the premise of test_a_lost_share_shows_in_single_precision: at LOOSE_RTOL the twin converges, and the share of the LAST
    row range of resid_kernel (wg_range over the n * NC reals of a column) in some pair's residual is more than ten times the
    1e-5 anorm that the acceptance allows between the reported residual and the one recomputed from X"""
    nev, ncv, which = LOOSE_CASE
    wide = wide_of(dtype)
    nc = 2 if np.dtype(dtype).kind == "c" else 1
    for n, G in zip(grid_sizes(dtype), (2, 3)):
        _, Dop, ref, _ = grid_problem(dtype, n)
        r = grid_twin(dtype, n, nev, ncv, which, rtol=LOOSE_RTOL)
        assert r.status == 0 and r.cycles == LOOSE_CYCLES[f"{name(dtype)}-n{n}"] and r.orth > 0
        tol = LOOSE_RTOL * r.anorm
        assert np.all(r.estimate <= tol)
        assert check_pairs(r.value, r.estimate, r.residual, r.anorm, ref, which, tol, dtype, f"loose twin {name(dtype)} n {n}") <= n + ncv + 2
        X = r.X.astype(wide)
        R = Dop.astype(wide) @ X - X * r.value
        rows = -(-n * nc // G) * (G - 1) // nc  # what the first G - 1 workgroups cover
        lost = np.linalg.norm(R, axis=0) - np.linalg.norm(R[:rows], axis=0)
        print(f"EIGSTAT loose twin {name(dtype)} n {n}: residual / anorm {r.residual / r.anorm}, the last range's share / anorm {lost / r.anorm}")
        assert np.max(lost) >= 10 * TOL[np.dtype(dtype)] * r.anorm


def test_twin_on_the_shifted_operator():
    """what test_update_and_solve_on_a_side_stream accepts the second solve against: diag(blocks) + 2.5 I at complex128, G = 3"""
    dtype, n = np.complex128, grid_sizes(np.complex128)[1]
    _, Dop, ref, v0 = grid_problem(dtype, n)
    D2 = Dop.shifted(2.5)
    ref2 = D2.eigenvalues()
    assert np.max(np.abs(ref2 - ref - 2.5)) <= 8 * np.finfo(dtype).eps * 8.5
    r = eigsh_twin(D2, v0, 5, 12, "LA", eig_rtol(dtype))
    assert r.status == 0 and r.cycles == 8 and r.orth > 0
    tol = eig_rtol(dtype) * r.anorm
    assert check_pairs(r.value, r.estimate, r.residual, r.anorm, ref2, "LA", tol, dtype, "twin, shifted") <= n + 12 + 2


# ---- ncv == n: the largest subspace bsm_eigsh_create accepts on the order-12 operator ------------------------------------------
FULL_CASES = [(10, 12, "LA"), (10, 12, "BE"), (1, 12, "SA")]


@pytest.mark.parametrize("case", FULL_CASES, ids=lambda c: f"{c[0]}of{c[1]}-{c[2]}")
@pytest.mark.parametrize("dtype", DTYPES, ids=name)
def test_twin_with_a_basis_of_the_whole_space(dtype, case):
    """step n - 1 leaves a w that is rounding alone: its norm is beta_m, every estimate is rounding, one cycle converges"""
    nev, ncv, which = case
    eps = float(np.finfo(dtype).eps)
    _, D, _ = tridiagonal_block(dtype)
    v0 = np.random.default_rng(5).uniform(-1, 1, 12).astype(dtype)
    r = eigsh_twin(D, v0, nev, ncv, which, eig_rtol(dtype))
    assert r.status == 0 and r.cycles == 1 and r.steps == 12 and r.nconv == nev
    lam = wanted_reference(np.linalg.eigvalsh(D.astype(wide_of(dtype))), which, nev)
    err = np.abs(r.value - lam)
    print(f"EIGSTAT twin ncv == n {name(dtype)} {case}: max (|theta - lam| - residual) / (eps anorm) {np.max(err - r.residual) / (eps * r.anorm):.2f} of 12, "
          f"max estimate / (eps anorm) {np.max(r.estimate) / (eps * r.anorm):.2f}, orth / eps {r.orth / eps:.1f}")
    assert np.all(err <= r.residual + 12 * eps * r.anorm)
    assert np.all(r.estimate <= eig_rtol(dtype) * r.anorm)
