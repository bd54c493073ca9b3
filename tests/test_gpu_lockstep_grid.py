"""GPU suite of the (G, K) layout that bsm_cg_solve and bsm_bicgstab_solve share: several columns on several row ranges at
once.  Every launch of the two units is a grid of G = krylov_grid(n, es) workgroups by K columns, every reduction leaves
part[(c * G + wg) * NC + k], and every consumer adds a column's G partials itself (wave_total).  The other solver suites
run G > 1 only with one float64 column and check it by count and true residual, which a lost share survives
(test_lockstep_grid_cpu.py shows that); here both factors are above one, in every type, and the check is the ITERATE:

  a. the workspace size says that the code's G is the table's G (no case below falls back to G = 1 unnoticed);
  b. x and the history after 4 iterations against the twin, over the (type, n, K) table of _lockstep.py, to MARGIN = 4 times
     what the twin moves by itself under permuted summation orders (_lockstep.spread, measured per case from column 0;
     the iterate in eps max|x|, the history in eps ||b||);
  c. ||b|| to m eps, m the longest chain of roundings counted from the kernels (_lockstep.bnorm_roundings: 20 .. 31);
  d. the decisions -- columns finishing at different counts, a zero column, a NaN in the last workgroup's range, freezing;
  e. the paths only a preconditioner, an initial guess, COCG or a real operator under complex vectors select, at G = 2, 3.

Every solve runs in the guarded buffers of _lockstep.solve_in_guarded_buffers, on a solver created for 16 columns.  The
figures are printed in LOCKSTAT lines before they are asserted."""
import numpy as np
import pytest

from _cg import MAX_RHS, column_tol, is_complex
from _gpu import torch_cuda  # noqa: F401
from _krylov import exact_minv
from _lockstep import (COLUMNS, ITS, MARGIN, RANGE_BYTES, TABLE, block_solve, bnorm_roundings, deviation, grid_case, half_sets,
                       krylov_grid, path_rtol, reference, run_twin, solve_in_guarded_buffers, spread, staggered6, workspace_bytes)
from _jacobi import uniform

pytestmark = pytest.mark.gpu

_built, _refs, _spreads = {}, {}, {}


def name(dtype):
    return np.dtype(dtype).name


def operator(bsm, method, n, dtype):
    """the device operator of grid_case(method, n, dtype), built once"""
    key = (method, n, name(dtype))
    if key not in _built:
        _built[key] = bsm.synthetic.build(grid_case(method, n, dtype)[0])
    return _built[key]


def solver(bsm, method, A, M=None, dtype=None):
    if method == "bicgstab":
        return bsm.BiCgStab(A, M, nrhs=MAX_RHS, dtype=dtype)
    return bsm.Cg(A, M, nrhs=MAX_RHS, dtype=dtype, method=method)


def check_grid(info, method, n, dtype, has_m=False):
    """the solve ran on the G this file means: info.workspace_bytes is the carve of create for the mirror's G"""
    assert info.workspace_bytes == workspace_bytes(method, n, dtype, MAX_RHS, has_m), (
        "the workspace is not the one of G =", krylov_grid(n, np.dtype(dtype).itemsize), info.workspace_bytes)


def check_iterates(tag, method, info, xh, Dop, B, dtype, k, Minv=None, X0=None):
    """every column of a solve cut at ITS iterations with rtol = 0: status 1, count ITS, x and the history within MARGIN x
    spread of the reference's (_lockstep.reference); references and the spread (of column 0) are computed once per tag"""
    devs = []
    if tag not in _spreads:
        _spreads[tag] = spread(method, Dop, B[:, 0], ITS, dtype, Minv=Minv, x0=None if X0 is None else X0[:, 0])
    sx, sh = _spreads[tag]
    for c in range(k):
        if (tag, c) not in _refs:
            _refs[tag, c] = reference(method, Dop, B[:, c], ITS, dtype, Minv=Minv, x0=None if X0 is None else X0[:, c])
        ref = _refs[tag, c]
        assert ref.status == 1 and ref.iterations == ITS
        devs.append(deviation(xh[:, c], info.history[:, c], ref, ITS, dtype))
    dx, dh = max(d[0] for d in devs), max(d[1] for d in devs)
    print(f"LOCKSTAT {tag} K={k}: iterate {dx:.2f} eps max|x|, spread {sx:.2f}, bound {MARGIN * sx:.2f}; history {dh:.2e}, spread {sh:.2e}, "
          f"bound {MARGIN * sh:.2e}")
    assert info.column_status.tolist() == [1] * k and info.column_iterations.tolist() == [ITS] * k, (info.column_status, info.column_iterations)
    assert info.history.shape == (ITS, k)
    assert dx <= MARGIN * sx, (tag, [d[0] for d in devs], sx)
    assert dh <= MARGIN * sh, (tag, [d[1] for d in devs], sh)


def check_converged(tag, method, info, xh, Dop, B, dtype, k, rtol, Minv=None, X0=None):
    """every column of a solve to rtol: status 0, the twin's count +-1, true residual <= 2 tol in complex128"""
    Dw = Dop.astype(np.complex128)
    for c in range(k):
        if (tag, "full", c) not in _refs:
            _refs[tag, "full", c] = run_twin(method, Dop, B[:, c], dtype, rtol, 200, Minv=Minv, x0=None if X0 is None else X0[:, c])
        run = _refs[tag, "full", c]
        true = float(np.linalg.norm(B[:, c].astype(np.complex128) - Dw @ xh[:, c].astype(np.complex128)))
        tol = column_tol(B[:, c], rtol)
        print(f"LOCKSTAT {tag} to rtol, column {c}: {info.column_iterations[c]} iterations, twin {run.iterations}, true residual / tol {true / tol:.3f}")
        assert run.status == 0 and info.column_status[c] == 0, (tag, c, run.status, info.column_status[c])
        assert abs(int(info.column_iterations[c]) - run.iterations) <= 1, (tag, c, info.column_iterations[c], run.iterations)
        assert true <= 2 * tol, (tag, c, true, tol)


# ---- a. the test's G is the code's G; c. ||b|| ------------------------------------------------------------------------------
_starts = {}


def start_only(torch, bsm, method, dtype, n):
    """a solve of 3 columns with maxiter = 0 (the start and the first decision only) -> (info, B)"""
    key = (method, name(dtype), n)
    if key not in _starts:
        B = np.asfortranarray(grid_case(method, n, dtype)[2][:, :3])
        S = solver(bsm, method, operator(bsm, method, n, dtype))
        xh, info = solve_in_guarded_buffers(torch, bsm, S, B, MAX_RHS, rtol=0.0, maxiter=0)
        assert info.column_status.tolist() == [1] * 3 and info.iterations == 0 and np.all(xh == 0)
        _starts[key] = (info, B)
    return _starts[key]


START = [(m, dt, n, G) for m in ("cg", "bicgstab") for dt, n, G in TABLE]
START_IDS = [f"{m}-{name(dt)}-n{n}-G{G}" for m, dt, n, G in START]


@pytest.mark.parametrize("method, dtype, n, G", START, ids=START_IDS)
def test_the_workspace_is_the_one_of_the_tables_grid(torch_cuda, bsm, method, dtype, n, G):
    """bsm_cg_create / bsm_bicgstab_create carve kmax * G partials per reduction out of the one allocation, so its size
    tells G; with another grid rule in the library this fails instead of the tests below passing at G = 1"""
    info, _ = start_only(torch_cuda, bsm, method, dtype, n)
    assert krylov_grid(n, np.dtype(dtype).itemsize) == G
    assert info.workspace_bytes == workspace_bytes(method, n, dtype)
    assert all(info.workspace_bytes != workspace_bytes(method, n, dtype, G=g) for g in (1, G - 1, G + 1)), "the size does not tell G"


@pytest.mark.parametrize("method, dtype, n, G", START, ids=START_IDS)
def test_bnorm_to_the_roundings_of_its_sum(torch_cuda, bsm, method, dtype, n, G):
    """info.bnorm against numpy.linalg.norm in complex128 to m eps, m = bnorm_roundings(n, dtype): 20 for G <= 64 in double,
    24 in single, 25 / 31 at the capped grid.  The terms are >= 0, so the bound is rigorous -- and one lost share of G moves
    the norm by about 1 / (2 G) >= 2e-3, which the n eps of the other suites hides at G = 256 in single precision"""
    info, B = start_only(torch_cuda, bsm, method, dtype, n)
    m, eps = bnorm_roundings(n, dtype), np.finfo(dtype).eps
    errs = [abs(info.bnorm[c] - nb) / nb for c in range(3) for nb in [float(np.linalg.norm(B[:, c].astype(np.complex128)))]]
    print(f"LOCKSTAT bnorm {method} {name(dtype)} n={n} G={G}: off by {max(errs) / eps:.2f} eps, m = {m}")
    assert 20 <= m <= 40
    assert max(errs) <= m * eps, (errs, m)


# ---- b. iterate and history after 4 iterations ------------------------------------------------------------------------------
ITER = [(m, dt, n, G, k) for m in ("cg", "bicgstab") for dt, n, G in TABLE for k in COLUMNS]
ITER += [("cocg", dt, n, G, k) for dt, n, G in TABLE if is_complex(dt) and G >= 65 for k in COLUMNS]


@pytest.mark.parametrize("method, dtype, n, G, k", ITER, ids=[f"{m}-{name(dt)}-n{n}-G{G}-k{k}" for m, dt, n, G, k in ITER])
def test_iterate_and_history_after_four_iterations(torch_cuda, bsm, method, dtype, n, G, k):
    _, Dop, B16 = grid_case(method, n, dtype)
    B = np.asfortranarray(B16[:, :k])
    S = solver(bsm, method, operator(bsm, method, n, dtype))
    xh, info = solve_in_guarded_buffers(torch_cuda, bsm, S, B, MAX_RHS, rtol=0.0, maxiter=ITS)
    check_grid(info, method, n, dtype)
    check_iterates(f"{method} {name(dtype)} n={n} G={G}", method, info, xh, Dop, B, dtype, k)
    assert info.a_products == (2 * ITS if method == "bicgstab" else ITS) and info.m_products == 0


# ---- d. decisions with G > 1 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.complex128, np.float32], ids=["complex128", "float32"])
@pytest.mark.parametrize("method", ["cg", "bicgstab"])
def test_decisions_across_workgroups(torch_cuda, bsm, method, dtype):
    """G = 65, six columns: four scaled so that they finish at four different counts under one absolute tolerance, one zero,
    one with a NaN in the last row (the LAST workgroup's range).  All 65 workgroups of a column must take the same
    decision from the partials they add themselves: the statuses, the counts, the frozen histories, and the same bytes
    from a second solve cut at the largest count"""
    torch = torch_cuda
    n = 64 * (RANGE_BYTES // np.dtype(dtype).itemsize) + 1
    _, Dop, B16 = grid_case(method, n, dtype)
    tau, step = (1e-4, 10.0) if dtype == np.float32 else (1e-10, 1000.0)  # as test_staggered_columns
    Bs, atol = staggered6(B16, dtype, tau, step)
    runs = [run_twin(method, Dop, Bs[:, c], dtype, 0.0, 200, atol=atol) for c in range(6)]
    counts = [r.iterations for r in runs]
    assert [r.status for r in runs] == [0, 0, 0, 0, 0, 2] and len(set(counts[:4])) == 4 and counts[4:] == [0, 0], counts
    S = solver(bsm, method, operator(bsm, method, n, dtype))
    xh, info = solve_in_guarded_buffers(torch, bsm, S, Bs, MAX_RHS, rtol=0.0, atol=atol, maxiter=200)
    check_grid(info, method, n, dtype)
    print(f"LOCKSTAT decisions {method} {name(dtype)} n={n}: counts {info.column_iterations.tolist()}, twin {counts}, statuses "
          f"{info.column_status.tolist()}")
    assert info.column_status.tolist() == [0, 0, 0, 0, 0, 2] and info.status == 2 and info.columns_converged == 5
    assert info.column_iterations[4] == 0 and info.column_iterations[5] == 0 and info.bnorm[4] == 0 and not np.isfinite(info.bnorm[5])
    assert np.all(xh[:, 4:] == 0)
    Dw = Dop.astype(np.complex128)
    for c in range(4):
        kc = int(info.column_iterations[c])
        assert abs(kc - counts[c]) <= 1, (c, kc, counts[c])
        true = float(np.linalg.norm(Bs[:, c].astype(np.complex128) - Dw @ xh[:, c].astype(np.complex128)))
        assert true <= 2 * atol, (c, true, atol)
        assert np.all(info.history[kc - 1:, c] == info.history[kc - 1, c]), ("a finished column's history moves", c)
        assert info.history[kc - 1, c] <= atol and (kc < 2 or info.history[kc - 2, c] > atol)
    assert info.iterations == max(info.column_iterations) and info.history.shape == (info.iterations, 6)
    x2, i2 = solve_in_guarded_buffers(torch, bsm, S, Bs, MAX_RHS, rtol=0.0, atol=atol, maxiter=int(info.iterations))
    assert i2.column_status.tolist() == [0, 0, 0, 0, 0, 2] and i2.column_iterations.tolist() == info.column_iterations.tolist()
    assert x2.tobytes() == xh.tobytes(), "a frozen column moved under the iterations enqueued behind its last"
    assert i2.history.tobytes() == info.history.tobytes()


# ---- e. the paths a preconditioner, an initial guess, a method or a pairing select ----------------------------------------
def grid_n(dtype, G):
    r0 = RANGE_BYTES // np.dtype(dtype).itemsize
    return {2: r0 + 1, 3: 2 * r0 + 3}[G]


def both_checks(torch, bsm, tag, method, S, Dop, B, dtype, n, has_m=False, Minv=None, X0=None):
    """K = 3: the iterate check of (b), then once to path_rtol(dtype) against the twin's count"""
    xh, info = solve_in_guarded_buffers(torch, bsm, S, B, MAX_RHS, X0=X0, rtol=0.0, maxiter=ITS)
    check_grid(info, method, n, dtype, has_m)
    check_iterates(tag, method, info, xh, Dop, B, dtype, 3, Minv=Minv, X0=X0)
    rtol = path_rtol(dtype)
    xh, info = solve_in_guarded_buffers(torch, bsm, S, B, MAX_RHS, X0=X0, rtol=rtol, maxiter=200)
    check_converged(tag, method, info, xh, Dop, B, dtype, 3, rtol, Minv=Minv, X0=X0)
    return info


@pytest.mark.parametrize("G", [2, 3])
@pytest.mark.parametrize("method", ["cg", "cocg", "bicgstab"])
def test_preconditioned_paths(torch_cuda, bsm, method, G):
    """M = block_jacobi over the HALVES of the 8-blocks: not the inverse, so the solve takes 9 .. 43 iterations through the
    RR = false kernels and dot_kernel of bsm_cg.hip / the SHAT kernel of bsm_bicgstab.hip; the twin takes the exact block
    inverse (the device's differs from it in its last bits -- 4 x 4 blocks with condition numbers of a few units)"""
    dtype = np.complex128
    n = grid_n(dtype, G)
    _, Dop, B16 = grid_case(method, n, dtype)
    B, sets = np.asfortranarray(B16[:, :3]), half_sets(n)
    Minv = exact_minv(Dop.dense(), sets)
    A = operator(bsm, method, n, dtype)
    S = solver(bsm, method, A, bsm.block_jacobi(A, sets))
    info = both_checks(torch_cuda, bsm, f"{method} M {name(dtype)} n={n} G={G}", method, S, Dop, B, dtype, n, has_m=True, Minv=Minv)
    assert info.iterations > 4 and info.m_products > 0


@pytest.mark.parametrize("G", [2, 3])
@pytest.mark.parametrize("method", ["cg", "bicgstab"])
def test_initial_guess_paths(torch_cuda, bsm, method, G):
    """X0 = the solution plus 1e-2 noise, handed over in the guarded X buffer: copy_kernel<TO_WS> and the start with q = A x0"""
    dtype = np.complex128
    n = grid_n(dtype, G)
    _, Dop, B16 = grid_case(method, n, dtype)
    B = np.asfortranarray(B16[:, :3])
    sol = block_solve(Dop, B)
    X0 = np.asfortranarray((sol + 1e-2 * np.max(np.abs(sol)) * uniform(np.random.default_rng(8900 + n), sol.shape, dtype)).astype(dtype))
    S = solver(bsm, method, operator(bsm, method, n, dtype))
    info = both_checks(torch_cuda, bsm, f"{method} x0 {name(dtype)} n={n} G={G}", method, S, Dop, B, dtype, n, X0=X0)
    assert info.a_products == (2 if method == "bicgstab" else 1) * info.iterations + 1


@pytest.mark.parametrize("G", [2, 3])
@pytest.mark.parametrize("dtype", [np.complex64, np.complex128], ids=["complex64", "complex128"])
def test_cocg_paths(torch_cuda, bsm, dtype, G):
    """the unconjugated form on the complex symmetric problem: the imaginary share of every partial (NC = 2, sgn = -1)"""
    n = grid_n(dtype, G)
    _, Dop, B16 = grid_case("cocg", n, dtype)
    assert np.array_equal(Dop.main, Dop.main.transpose(0, 2, 1)) and not np.array_equal(Dop.main, Dop.main.conj().transpose(0, 2, 1))
    S = solver(bsm, "cocg", operator(bsm, "cocg", n, dtype))
    both_checks(torch_cuda, bsm, f"cocg {name(dtype)} n={n} G={G}", "cocg", S, Dop, np.asfortranarray(B16[:, :3]), dtype, n)


@pytest.mark.parametrize("G", [2, 3])
@pytest.mark.parametrize("method", ["cg", "bicgstab"])
def test_real_operator_under_complex_vectors(torch_cuda, bsm, method, G):
    """a float64 operator under dtype = complex128: the grid follows the VECTOR type (16-byte elements)"""
    n = grid_n(np.complex128, G)
    _, Dop, _ = grid_case(method, n, np.float64)
    B = np.asfortranarray(grid_case(method, n, np.complex128)[2][:, :3])
    S = solver(bsm, method, operator(bsm, method, n, np.float64), dtype=np.complex128)
    both_checks(torch_cuda, bsm, f"{method} real A {n} G={G}", method, S, Dop.astype(np.complex128), B, np.complex128, n)
