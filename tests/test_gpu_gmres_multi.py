"""GPU suite of bsm_gmres_multi_solve / GmresMulti: right-preconditioned restarted GMRES on several right-hand sides in
lockstep against the numpy twin of tests/_gmres_multi.py (the same method, none of the code):

  1. the 12 order-400 operators with block-Jacobi, five columns: statuses, true residuals, counts, the history rules, the
     product counts, and the same bytes from the same solve again;
  2. the (G, K) grid of _lockstep.py: iterate and history after GMRES(3) x 5 iterations (one restart) to MARGIN = 4 times
     what the twin moves by itself under 8 permuted summation orders, in guarded buffers; with M, an initial guess and a
     real operator under complex vectors at G = 2, 3;
  3. the decisions on the device: columns finishing at different counts in different cycles, a zero column, a NaN column;
  4. the one-wave kernels past 64 (one cycle of 70) and at restart 1;
  5. one pass over the matrix per product, and the cost of the look-ahead;
  6. the Python surface, and every refusal through the raw ctypes drivers.

The twin itself, the pinned counts and the sharpness of check 2 are in test_gmres_multi_cpu.py.  Figures are printed in
LOCKSTAT lines before they are asserted."""
import ctypes as C

import numpy as np
import pytest

from _bicgstab import bicgstab_problem
from _cg import MAX_RHS, cg_problem, column_tol
from _ctors import ctor_build
from _gmres_multi import (GRID_ITS, GRID_RESTART, MARGIN, check_columns, check_history, columns400, cycles_of, gmres_multi_twin,
                          grid_spread, products, raw_gm_create, raw_gm_destroy, raw_gm_solve, reference, slack_of, workspace_bytes)
from _gpu import TOL, dev_copy, torch_cuda  # noqa: F401
from _jacobi import CODE, DTYPES, KINDS, NOP, uniform
from _krylov import (ERR_DEVICE, ERR_INVALID, ERR_UNSUPPORTED, MAX_RESTART, exact_minv, expected_products, krylov_problem, rtol_of,
                     true_residual)
from _lockstep import (COLUMNS, RANGE_BYTES, TABLE, block_solve, deviation, grid_case, half_sets, krylov_grid, path_rtol,
                       solve_in_guarded_buffers, staggered6)
from _submat import Truth

pytestmark = pytest.mark.gpu
NB = 5
LOOKAHEAD = 1  # products of A (and of M) a solve that ends early pays beyond info.a_products (m_products): include/bsm_rocm.h

_built, _refs, _solvers = {}, {}, {}


def name(dtype):
    return np.dtype(dtype).name


def reproducible(*ops):
    """the products of these handles are bitwise reproducible: exclusive forward images (no atomics)"""
    return all(o.stats()["exclusive"] == 1 for o in ops)


# ---- 1. the order-400 operators with block-Jacobi ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=[name(d) for d in DTYPES])
def test_solves_with_block_jacobi(torch_cuda, bsm, kind, dtype):
    torch, restart = torch_cuda, 20
    p, sets, _ = krylov_problem(kind, dtype)
    D, rtol, B = Truth(p).D, rtol_of(dtype), columns400(kind, dtype)
    Minv = exact_minv(D, sets)
    A = bsm.synthetic.build(p)
    M = bsm.block_jacobi(A, sets)
    S = bsm.GmresMulti(A, M, nrhs=NB, restart=restart)
    Bd = dev_copy(torch, B)
    X, info = S.solve(Bd, rtol=rtol, maxiter=100)
    xh = X.cpu().numpy()
    assert info.status == 0 and info.converged and info.columns_converged == NB
    for c in range(NB):
        its, tol = int(info.column_iterations[c]), column_tol(B[:, c], rtol)
        twin = gmres_multi_twin(D, B[:, c], Minv, restart, rtol, 100, dtype)
        true = true_residual(D, xh[:, c], B[:, c])
        print(f"LOCKSTAT gmres {kind} {name(dtype)} column {c}: {its} iterations, twin {twin.iterations}, true residual / tol {true / tol:.3f}")
        assert info.column_status[c] == 0 and twin.status == 0
        assert true <= 2 * tol, (c, true, tol)
        assert its <= twin.iterations + slack_of(twin.iterations), (c, its, twin.iterations)
        check_history(info.history[:its, c], 0, info.residual[c], rtol * info.bnorm[c], restart, dtype)
        assert np.all(info.history[its:, c] == info.residual[c]), "a finished column's history moves"
    assert info.iterations == max(info.column_iterations) and info.history.shape == (info.iterations, NB)
    assert info.cycles == cycles_of(info.iterations, restart)
    assert (info.a_products, info.m_products) == products(info, restart, False, True)
    X2, info2 = S.solve(Bd, rtol=rtol, maxiter=100)
    assert info2.column_iterations.tolist() == info.column_iterations.tolist()
    if reproducible(A, M):
        assert X2.cpu().numpy().tobytes() == xh.tobytes() and info2.history.tobytes() == info.history.tobytes()
    else:
        assert np.max(np.abs(X2.cpu().numpy() - xh)) <= TOL[np.dtype(dtype)] * np.max(np.abs(xh))


# ---- 2. the (G, K) grid ---------------------------------------------------------------------------------------------------------
def operator(bsm, n, dtype):
    """the device operator of grid_case("bicgstab", n, dtype) -- nonsymmetric block diagonal --, built once"""
    key = (n, name(dtype))
    if key not in _built:
        _built[key] = bsm.synthetic.build(grid_case("bicgstab", n, dtype)[0])
    return _built[key]


def grid_solver(bsm, n, dtype):
    key = (n, name(dtype))
    if key not in _solvers:
        _solvers[key] = bsm.GmresMulti(operator(bsm, n, dtype), nrhs=MAX_RHS, restart=GRID_RESTART)
    return _solvers[key]


def check_iterates(tag, info, xh, Dop, B, dtype, k, n, has_m=False, Minv=None, X0=None):
    """every column of a GMRES(GRID_RESTART) solve cut at GRID_ITS iterations with rtol = 0: status 1, the count, x and the
    history within MARGIN x spread of the reference's; the workspace is the one of the mirror's G"""
    assert info.workspace_bytes == workspace_bytes(n, dtype, GRID_RESTART, MAX_RHS, has_m), (
        "the workspace is not the one of G =", krylov_grid(n, np.dtype(dtype).itemsize), info.workspace_bytes)
    sx, sh = grid_spread(tag, Dop, B, k, dtype, Minv=Minv, x0=X0)
    devs = []
    for c in range(k):
        if (tag, c) not in _refs:
            _refs[tag, c] = reference(Dop, B[:, c], GRID_ITS, dtype, Minv=Minv, x0=None if X0 is None else X0[:, c])
        ref = _refs[tag, c]
        assert ref.status == 1 and ref.iterations == GRID_ITS and ref.cycles == 2
        devs.append(deviation(xh[:, c], info.history[:, c], ref, GRID_ITS, dtype))
    dx, dh = max(d[0] for d in devs), max(d[1] for d in devs)
    print(f"LOCKSTAT gmres {tag} K={k}: iterate {dx:.2f} eps max|x|, spread {sx:.2f}, bound {MARGIN * sx:.2f}; history {dh:.2e}, "
          f"spread {sh:.2e}, bound {MARGIN * sh:.2e}")
    assert info.column_status.tolist() == [1] * k and info.column_iterations.tolist() == [GRID_ITS] * k
    assert info.history.shape == (GRID_ITS, k) and info.cycles == 2
    assert (info.a_products, info.m_products) == expected_products(GRID_ITS, 2, X0 is not None, has_m)
    assert dx <= MARGIN * sx, (tag, [d[0] for d in devs], sx)
    assert dh <= MARGIN * sh, (tag, [d[1] for d in devs], sh)


GRID = [(dt, n, G, k) for dt, n, G in TABLE for k in COLUMNS]


@pytest.mark.parametrize("dtype, n, G, k", GRID, ids=[f"{name(dt)}-n{n}-G{G}-k{k}" for dt, n, G, k in GRID])
def test_iterate_and_history_after_a_restart(torch_cuda, bsm, dtype, n, G, k):
    assert krylov_grid(n, np.dtype(dtype).itemsize) == G
    _, Dop, B16 = grid_case("bicgstab", n, dtype)
    B = np.asfortranarray(B16[:, :k])
    xh, info = solve_in_guarded_buffers(torch_cuda, bsm, grid_solver(bsm, n, dtype), B, MAX_RHS, rtol=0.0, maxiter=GRID_ITS)
    check_iterates(f"{name(dtype)} n={n} G={G}", info, xh, Dop, B, dtype, k, n)


def grid_n(dtype, G):
    r0 = RANGE_BYTES // np.dtype(dtype).itemsize
    return {2: r0 + 1, 3: 2 * r0 + 3}[G]


def check_converged(tag, bsm, torch, A, M, Dop, B, dtype, Minv=None, X0=None, vdtype=None):
    """K = 3 at restart 5 to path_rtol: status 0, the twin's count +-1 (pinned and stable under permuted sums in
    test_gmres_multi_cpu.py), true residual <= 2 tol in complex128"""
    rtol = path_rtol(dtype)
    S = bsm.GmresMulti(A, M, nrhs=MAX_RHS, restart=5, dtype=vdtype)
    xh, info = solve_in_guarded_buffers(torch, bsm, S, B, MAX_RHS, X0=X0, rtol=rtol, maxiter=200)
    Dw = Dop.astype(np.complex128)
    for c in range(3):
        run = gmres_multi_twin(Dop, B[:, c], Minv, 5, rtol, 200, dtype, x0=None if X0 is None else X0[:, c])
        true = float(np.linalg.norm(B[:, c].astype(np.complex128) - Dw @ xh[:, c].astype(np.complex128)))
        tol = column_tol(B[:, c], rtol)
        print(f"LOCKSTAT gmres {tag} to rtol, column {c}: {info.column_iterations[c]} iterations, twin {run.iterations}, true residual / tol "
              f"{true / tol:.3f}")
        assert run.status == 0 and info.column_status[c] == 0
        assert abs(int(info.column_iterations[c]) - run.iterations) <= 1, (tag, c, info.column_iterations[c], run.iterations)
        assert true <= 2 * tol, (tag, c, true, tol)
    assert (info.a_products, info.m_products) == products(info, 5, X0 is not None, M is not None)


@pytest.mark.parametrize("G", [2, 3])
def test_preconditioned_path(torch_cuda, bsm, G):
    """M = block_jacobi over the HALVES of the 8-blocks (not the inverse): the products through Z, Z = opM(M) U at the cycle's
    end; the twin takes the exact block inverse"""
    dtype = np.complex128
    n = grid_n(dtype, G)
    _, Dop, B16 = grid_case("bicgstab", n, dtype)
    B, sets = np.asfortranarray(B16[:, :3]), half_sets(n)
    Minv = exact_minv(Dop.dense(), sets)
    A = operator(bsm, n, dtype)
    M = bsm.block_jacobi(A, sets)
    S = bsm.GmresMulti(A, M, nrhs=MAX_RHS, restart=GRID_RESTART)
    xh, info = solve_in_guarded_buffers(torch_cuda, bsm, S, B, MAX_RHS, rtol=0.0, maxiter=GRID_ITS)
    tag = f"M {name(dtype)} n={n} G={G}"
    check_iterates(tag, info, xh, Dop, B, dtype, 3, n, has_m=True, Minv=Minv)
    check_converged(tag, bsm, torch_cuda, A, M, Dop, B, dtype, Minv=Minv)


@pytest.mark.parametrize("G", [2, 3])
def test_initial_guess_path(torch_cuda, bsm, G):
    """X0 = the solution plus 1e-2 noise, handed over in the guarded X buffer: the copy into the workspace and the first start
    with Q = op(A) X0"""
    dtype = np.complex128
    n = grid_n(dtype, G)
    _, Dop, B16 = grid_case("bicgstab", n, dtype)
    B = np.asfortranarray(B16[:, :3])
    sol = block_solve(Dop, B)
    X0 = np.asfortranarray((sol + 1e-2 * np.max(np.abs(sol)) * uniform(np.random.default_rng(8900 + n), sol.shape, dtype)).astype(dtype))
    xh, info = solve_in_guarded_buffers(torch_cuda, bsm, grid_solver(bsm, n, dtype), B, MAX_RHS, X0=X0, rtol=0.0, maxiter=GRID_ITS)
    tag = f"x0 {name(dtype)} n={n} G={G}"
    check_iterates(tag, info, xh, Dop, B, dtype, 3, n, X0=X0)
    check_converged(tag, bsm, torch_cuda, operator(bsm, n, dtype), None, Dop, B, dtype, X0=X0)


@pytest.mark.parametrize("G", [2, 3])
def test_real_operator_under_complex_vectors(torch_cuda, bsm, G):
    """a float64 operator under dtype = complex128 (bsm_mul_multi_cvec): the grid follows the VECTOR type"""
    n = grid_n(np.complex128, G)
    _, Dop, _ = grid_case("bicgstab", n, np.float64)
    B = np.asfortranarray(grid_case("bicgstab", n, np.complex128)[2][:, :3])
    A = operator(bsm, n, np.float64)
    S = bsm.GmresMulti(A, nrhs=MAX_RHS, restart=GRID_RESTART, dtype=np.complex128)
    xh, info = solve_in_guarded_buffers(torch_cuda, bsm, S, B, MAX_RHS, rtol=0.0, maxiter=GRID_ITS)
    Dc = Dop.astype(np.complex128)
    tag = f"real A n={n} G={G}"
    check_iterates(tag, info, xh, Dc, B, np.complex128, 3, n)
    check_converged(tag, bsm, torch_cuda, A, None, Dc, B, np.complex128, vdtype=np.complex128)


# ---- 3. the decisions ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.complex128, np.float32], ids=["complex128", "float32"])
def test_decisions_across_workgroups_and_cycles(torch_cuda, bsm, dtype):
    """G = 65, restart 5, six columns under one absolute tolerance: four finish at four different counts in four different
    cycles, one is zero, one has a NaN in the last row (the LAST workgroup's range).  Every workgroup of a column takes the
    same decision from the partials it adds itself, a column that has finished inside a cycle gets its update at that
    cycle's end and nothing after it: the twin's counts, the frozen histories, and the same bytes from a second solve cut
    at the largest count"""
    torch, restart = torch_cuda, 5
    n = 64 * (RANGE_BYTES // np.dtype(dtype).itemsize) + 1
    _, Dop, B16 = grid_case("bicgstab", n, dtype)
    tau, step = (1e-4, 10.0) if dtype == np.float32 else (1e-10, 1000.0)  # as test_gpu_lockstep_grid.py
    Bs, atol = staggered6(B16, dtype, tau, step)
    runs = [gmres_multi_twin(Dop, Bs[:, c], None, restart, 0.0, 300, dtype, atol=atol) for c in range(6)]
    counts = [r.iterations for r in runs]
    assert [r.status for r in runs] == [0, 0, 0, 0, 0, 2] and len(set(counts[:4])) == 4 and counts[4:] == [0, 0], counts
    S = bsm.GmresMulti(operator(bsm, n, dtype), nrhs=MAX_RHS, restart=restart)
    xh, info = solve_in_guarded_buffers(torch, bsm, S, Bs, MAX_RHS, rtol=0.0, atol=atol, maxiter=300)
    print(f"LOCKSTAT gmres decisions {name(dtype)} n={n}: counts {info.column_iterations.tolist()}, twin {counts}, statuses "
          f"{info.column_status.tolist()}")
    assert info.workspace_bytes == workspace_bytes(n, dtype, restart)
    assert info.column_status.tolist() == [0, 0, 0, 0, 0, 2] and info.status == 2 and info.columns_converged == 5
    assert info.column_iterations.tolist() == counts
    assert info.bnorm[4] == 0 and not np.isfinite(info.bnorm[5]) and np.all(xh[:, 4:] == 0)
    Dw = Dop.astype(np.complex128)
    for c in range(4):
        kc = counts[c]
        true = float(np.linalg.norm(Bs[:, c].astype(np.complex128) - Dw @ xh[:, c].astype(np.complex128)))
        assert true <= 2 * atol, (c, true, atol)
        check_history(info.history[:kc, c], 0, info.residual[c], atol, restart, dtype)
        assert np.all(info.history[kc - 1:, c] == info.history[kc - 1, c]), ("a finished column's history moves", c)
    assert info.iterations == max(counts) and info.history.shape == (info.iterations, 6)
    assert (info.a_products, info.m_products) == products(info, restart, False, False)
    x2, i2 = solve_in_guarded_buffers(torch, bsm, S, Bs, MAX_RHS, rtol=0.0, atol=atol, maxiter=int(info.iterations))
    assert i2.column_status.tolist() == [0, 0, 0, 0, 0, 2] and i2.column_iterations.tolist() == counts
    assert x2.tobytes() == xh.tobytes(), "a frozen column moved under what was enqueued behind its last iteration"
    assert i2.history.tobytes() == info.history.tobytes()


# ---- 4. the one-wave kernels past 64, and restart 1 ---------------------------------------------------------------------------
WAVE = [("vbcrs", np.float32), ("blocksparse", np.complex128)]


@pytest.mark.parametrize("kind, dtype", WAVE, ids=[f"{k}-{name(d)}" for k, d in WAVE])
def test_one_cycle_of_seventy(torch_cuda, bsm, kind, dtype):
    """restart 70 without M, where GMRES stagnates: gm_hess applies up to 69 stored rotations, gm_trsolve walks a 70 x 70
    triangle with its second lane-strided pass, gm_dot / gm_update run 18 batches of basis vectors"""
    torch = torch_cuda
    p, _, _ = krylov_problem(kind, dtype)
    D, B = Truth(p).D, np.asfortranarray(columns400(kind, dtype)[:, :3])
    A = bsm.synthetic.build(p)
    X, info = bsm.GmresMulti(A, nrhs=3, restart=70).solve(dev_copy(torch, B), rtol=0.0, maxiter=70)
    xh = X.cpu().numpy()
    assert info.iterations == 70 and info.cycles == 1 and info.column_status.tolist() == [1] * 3
    assert (info.a_products, info.m_products) == (70, 0)
    for c in range(3):
        check_history(info.history[:, c], 1, info.residual[c], 0.0, 70, dtype)
        ratio = info.residual[c] / true_residual(D, xh[:, c], B[:, c])
        print(f"LOCKSTAT gmres one cycle of 70 {kind} {name(dtype)} column {c}: estimate / true - 1 = {ratio - 1:.3e}, estimate / |b| = "
              f"{info.residual[c] / info.bnorm[c]:.4f}")
        assert abs(ratio - 1) <= 1e3 * np.finfo(dtype).eps


@pytest.mark.parametrize("kind, dtype", WAVE, ids=[f"{k}-{name(d)}" for k, d in WAVE])
def test_restart_one_with_block_jacobi(torch_cuda, bsm, kind, dtype):
    """GMRES(1): every iteration is a cycle -- a start, one rotation, a 1 x 1 back substitution, an update through M"""
    torch = torch_cuda
    p, sets, _ = krylov_problem(kind, dtype)
    D, rtol, B = Truth(p).D, rtol_of(dtype), np.asfortranarray(columns400(kind, dtype)[:, :3])
    Minv = exact_minv(D, sets)
    A = bsm.synthetic.build(p)
    M = bsm.block_jacobi(A, sets)
    Bd = dev_copy(torch, B)
    Y = torch.empty((3, NOP), dtype=Bd.dtype, device="cuda").t()
    before = A.value_passes()
    bsm.mul(Y, A, Bd)
    per = A.value_passes() - before  # passes of one 3-column product
    S = bsm.GmresMulti(A, M, nrhs=3, restart=1)
    before = A.value_passes()
    X, info = S.solve(Bd, rtol=rtol, maxiter=400)
    passes = A.value_passes() - before
    xh = X.cpu().numpy()
    for c in range(3):
        twin = gmres_multi_twin(D, B[:, c], Minv, 1, rtol, 400, dtype)
        its = int(info.column_iterations[c])
        print(f"LOCKSTAT gmres restart 1 {kind} {name(dtype)} column {c}: {its} iterations, twin {twin.iterations}")
        assert twin.status == 0 and info.column_status[c] == 0
        assert its <= twin.iterations + slack_of(twin.iterations)
        assert true_residual(D, xh[:, c], B[:, c]) <= 2 * column_tol(B[:, c], rtol)
    assert info.cycles == info.iterations
    assert (info.a_products, info.m_products) == products(info, 1, False, True)
    # the handle's own count of what was enqueued: the reported products, and at most the look-ahead beyond them
    print(f"LOCKSTAT gmres restart 1 {kind} {name(dtype)}: a_products {info.a_products}, {passes} passes over A at {per} per product")
    assert info.a_products * per <= passes <= (info.a_products + LOOKAHEAD) * per


# ---- 5. one pass over the matrix per product ------------------------------------------------------------------------------------
def test_one_pass_per_product_and_the_look_ahead(torch_cuda, bsm):
    torch, dtype, K = torch_cuda, np.float64, 8
    p, sets, D, B = cg_problem("vbcrs", dtype)
    B8 = np.asfortranarray(np.concatenate([B, uniform(np.random.default_rng(4100), (B.shape[0], K - B.shape[1]), dtype)], axis=1))
    A = bsm.synthetic.build(p)
    M = bsm.block_jacobi(A, sets)
    Bd = dev_copy(torch, B8)
    Y = torch.empty((K, B.shape[0]), dtype=Bd.dtype, device="cuda").t()
    before = A.value_passes()
    bsm.mul(Y, A, Bd)
    assert A.value_passes() == before + 1, "a plain 8-column product does not stream the matrix once"
    S = bsm.GmresMulti(A, M, nrhs=K, restart=4)
    before, mbefore = A.value_passes(), M.value_passes()
    X, first = S.solve(Bd, rtol=1e-10, maxiter=100)
    free, mfree = A.value_passes() - before, M.value_passes() - mbefore
    print(f"LOCKSTAT gmres passes: {first.iterations} iterations in {first.cycles} cycles, a_products {first.a_products}, passes over A "
          f"{free}; m_products {first.m_products}, passes over M {mfree}")
    assert first.status == 0 and first.cycles > 1
    assert first.a_products <= free <= first.a_products + LOOKAHEAD
    assert first.m_products <= mfree <= first.m_products + LOOKAHEAD
    before = A.value_passes()
    X, info = S.solve(Bd, rtol=1e-10, maxiter=int(first.iterations))
    assert info.status == 0 and info.iterations == first.iterations
    assert A.value_passes() - before == info.a_products == first.a_products


# ---- 6. the surface ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(torch_cuda, bsm):
    """the blocksparse float64 problem of order 400 with its handles and the twin's runs"""
    dtype = np.float64
    p, sets, b = krylov_problem("blocksparse", dtype)
    D, B = Truth(p).D, columns400("blocksparse", dtype)
    A = bsm.synthetic.build(p)
    M = bsm.block_jacobi(A, sets)
    Minv = exact_minv(D, sets)
    runs = [gmres_multi_twin(D, B[:, c], Minv, 20, 1e-10, 100, dtype) for c in range(NB)]
    return dict(p=p, sets=sets, b=b, D=D, B=B, A=A, M=M, Minv=Minv, runs=runs)


def test_vectors_numpy_operands_and_the_one_shot_forms(torch_cuda, bsm, small):
    torch, s = torch_cuda, small
    D, B, A, M, runs = s["D"], s["B"], s["A"], s["M"], s["runs"]
    S = bsm.GmresMulti(A, M, nrhs=NB, restart=20)
    # a vector in gives a vector out
    b1 = np.ascontiguousarray(B[:, 1])
    xv, iv = S.solve(torch.from_numpy(b1).cuda(), rtol=1e-10, maxiter=100)
    assert tuple(xv.shape) == (NOP,) and iv.column_status.tolist() == [0] and iv.history.shape == (iv.iterations, 1)
    assert true_residual(D, xv.cpu().numpy(), b1) <= 2 * column_tol(b1, 1e-10)
    # numpy operands are staged
    Xh = np.full(B.shape, np.nan, dtype=B.dtype, order="F")
    got, info = S.solve(B, X=Xh, rtol=1e-10, maxiter=100)
    assert got is Xh and isinstance(info, bsm.CgInfo)
    check_columns(info, runs, D, Xh, B, 1e-10, "numpy B")
    # X0: from the converged answer nothing is left to do (the true residual of the start meets the tolerance)
    X0 = np.asfortranarray(Xh.copy())
    X1, i1 = S.solve(B, X0=X0, rtol=1e-8, maxiter=100)
    assert i1.iterations == 0 and i1.column_status.tolist() == [0] * NB and (i1.a_products, i1.m_products) == (1, 0)
    assert np.array_equal(X1, X0) and i1.cycles == 0 and np.all(i1.residual <= 1e-8 * i1.bnorm)
    # gmres(A, B) with a matrix goes to GmresMulti, with a vector it is the single-column solver as before
    Xm, im = bsm.gmres(A, dev_copy(torch, B), M=M, restart=20, rtol=1e-10, maxiter=100)
    assert isinstance(im, bsm.CgInfo) and im.cycles == cycles_of(im.iterations, 20)
    check_columns(im, runs, D, Xm.cpu().numpy(), B, 1e-10, "gmres(A, B)")
    xs, isingle = bsm.gmres(A, torch.from_numpy(b1).cuda(), M=M, restart=20, rtol=1e-10, maxiter=100)
    assert isinstance(isingle, bsm.GmresInfo) and isingle.status == 0 and isingle.history.ndim == 1
    assert isingle.iterations == im.column_iterations[1]
    with pytest.raises(ValueError):
        S.solve(dev_copy(torch, B), X=np.zeros(B.shape, B.dtype, order="F"))  # B on the device, X on the host
    with pytest.raises(ValueError):
        bsm.GmresMulti(A, M, nrhs=2).solve(dev_copy(torch, B))  # more columns than the solver holds


@pytest.mark.parametrize("wrapper", ["transpose", "adjoint"])
def test_transposed_operators(torch_cuda, bsm, wrapper):
    torch, dtype = torch_cuda, np.complex128
    p, sets, _ = krylov_problem("blocksparse", dtype)
    D, B = Truth(p).D, columns400("blocksparse", dtype)
    Dt = D.T if wrapper == "transpose" else D.conj().T
    A = bsm.synthetic.build(p)
    M = bsm.block_jacobi(A, sets)
    wrap = getattr(bsm, wrapper)
    X, info = bsm.gmres(wrap(A), dev_copy(torch, B), M=wrap(M), restart=20, rtol=1e-10, maxiter=100)
    Minv = exact_minv(Dt, sets)
    runs = [gmres_multi_twin(Dt, B[:, c], Minv, 20, 1e-10, 100, dtype) for c in range(NB)]
    check_columns(info, runs, Dt, X.cpu().numpy(), B, 1e-10, wrapper)


def test_single_precision_storage_solves_in_double(torch_cuda, bsm):
    """a storage=float32 handle has double vectors: the solve runs in float64 on the operator as rounded to float32 (the
    problem of test_gpu_bicgstab.py's test of the same pairing: its blocks do not overlap, so rounding them rounds D)"""
    torch = torch_cuda
    p, sets, D, B = bicgstab_problem("vbcrs", np.float64)
    D32 = D.astype(np.float32).astype(np.float64)
    A = bsm.synthetic.build(p, storage=np.float32)
    M = bsm.block_jacobi(A, sets)
    X, info = bsm.GmresMulti(A, M, nrhs=NB, restart=20).solve(dev_copy(torch, B), rtol=1e-10, maxiter=100)
    Minv = exact_minv(D32, sets)
    runs = [gmres_multi_twin(D32, B[:, c], Minv, 20, 1e-10, 100, np.float64) for c in range(NB)]
    assert X.dtype == torch.float64
    check_columns(info, runs, D32, X.cpu().numpy(), B, 1e-10, "storage=float32")


def test_identity_blocks_take_one_iteration(torch_cuda, bsm):
    """A = I (blocks of order 8) and B of +-1 columns at n = 256: ||w|| after the orthogonalisation is 0 -- the lucky
    breakdown: 1 / ||w|| is replaced by 0, the estimate is 0 -- and X == B exactly"""
    torch, n = torch_cuda, 256
    starts = np.arange(n // 8, dtype=np.int64) * 8 + 1
    p = dict(kind="vbcrs", blocks=[np.asfortranarray(np.eye(8))] * (n // 8), rowstart=starts, colstart=starts.copy(), size=(n, n))
    A = bsm.synthetic.build(p)
    B = np.asfortranarray(np.where(np.random.default_rng(9200).random((n, 4)) < 0.5, -1.0, 1.0))
    X, info = bsm.GmresMulti(A, nrhs=4, restart=10).solve(dev_copy(torch, B), rtol=0.0, atol=0.0, maxiter=50)
    assert info.column_status.tolist() == [0] * 4 and info.column_iterations.tolist() == [1] * 4
    assert np.array_equal(X.cpu().numpy(), B) and np.all(info.history == 0) and np.all(np.isfinite(X.cpu().numpy()))


def test_refusals(torch_cuda, bsm, small):
    torch, dtype, s = torch_cuda, np.float64, small
    f64 = CODE[np.dtype(dtype)]
    A, M, B, p = s["A"], s["M"], s["B"], s["p"]
    for what, args in [("nrhs_max 0", (A, 0, M, 0, f64, 0, 20)), ("nrhs_max 17", (A, 0, M, 0, f64, MAX_RHS + 1, 20)),
                       ("restart 0", (A, 0, M, 0, f64, 4, 0)), ("restart 129", (A, 0, M, 0, f64, 4, MAX_RESTART + 1)),
                       ("bad opA", (A, 3, M, 0, f64, 4, 20)), ("bad opM", (A, 0, M, -1, f64, 4, 20)),
                       ("vdtype of a stored type", (A, 0, M, 0, 4, 4, 20)), ("vdtype out of range", (A, 0, M, 0, 99, 4, 20)),
                       ("float64 A under complex64 vectors", (A, 0, None, 0, CODE[np.dtype(np.complex64)], 4, 20)),
                       ("null A", (None, 0, None, 0, f64, 4, 20))]:
        assert raw_gm_create(*args)[0] == ERR_INVALID, what
    pc, _, _ = krylov_problem("vbcrs", np.complex128)
    Ac = bsm.synthetic.build(pc)
    assert raw_gm_create(Ac, 0, None, 0, f64, 4, 20)[0] == ERR_INVALID      # a complex handle under real vectors
    assert raw_gm_create(A, 0, Ac, 0, f64, 4, 20)[0] == ERR_INVALID       # a complex M under real vectors
    rect = bsm.BlockSparseMatrix([np.ones((3, 5))], [[1, 2, 3]], [[1, 2, 3, 4, 5]], (3, 5))
    assert raw_gm_create(rect, 0, None, 0, f64, 4, 20)[0] == ERR_INVALID     # op(A) is not square
    small_m = bsm.BlockSparseMatrix([np.eye(3)], [[1, 2, 3]], [[1, 2, 3]], (3, 3))
    assert raw_gm_create(A, 0, small_m, 0, f64, 4, 20)[0] == ERR_INVALID     # M of another order
    A2 = ctor_build(bsm, "blocksparse", p, devices=[0, 0])
    assert raw_gm_create(A2, 0, None, 0, f64, 4, 20)[0] == ERR_UNSUPPORTED
    assert raw_gm_create(A, 0, A2, 0, f64, 4, 20)[0] == ERR_UNSUPPORTED
    with pytest.raises(bsm._lib.BsmError, match="multi-device"):
        bsm.GmresMulti(A2)
    An = bsm.synthetic.build(p, device=-2)  # BSM_DEVICE_NONE: analysis only
    assert raw_gm_create(An, 0, None, 0, f64, 4, 20)[0] == ERR_DEVICE
    with pytest.raises(bsm._lib.BsmError, match="restart"):
        bsm.GmresMulti(A, restart=0)
    rc, ptr = raw_gm_create(A, 0, M, 0, f64, MAX_RHS, 20)
    assert rc == 0 and ptr.value
    try:
        Bd = dev_copy(torch, np.asfortranarray(np.concatenate([B] * 4, axis=1)))  # 20 columns
        Xs = torch.zeros((20, NOP), dtype=Bd.dtype, device="cuda")
        Xd = Xs.t()
        st = torch.cuda.current_stream().cuda_stream
        b, x, es = Bd.data_ptr(), Xd.data_ptr(), 8
        ok = raw_gm_solve(ptr, NB, b, NOP, x, NOP, rtol=1e-10, stream=st)
        assert ok[0] == 0 and ok[1].status == 0 and ok[1].workspace_bytes == workspace_bytes(NOP, dtype, 20, MAX_RHS, True)
        for what, args, kw in [("nrhs 0", (0, b, NOP, x, NOP), {}), ("nrhs 17", (17, b, NOP, x, NOP), {}),
                               ("ldx < n", (NB, b, NOP, x, NOP - 1), {}), ("ldb < n", (NB, b, NOP - 1, x, NOP), {}),
                               ("X is B", (NB, b, NOP, b, NOP), {}),
                               ("X overlaps the last column of B", (NB, b, NOP, b + (NB * NOP - 8) * es, NOP), {}),
                               ("null B", (NB, None, NOP, x, NOP), {}), ("null X", (NB, b, NOP, None, NOP), {}),
                               ("negative rtol", (NB, b, NOP, x, NOP), dict(rtol=-1.0)),
                               ("NaN rtol", (NB, b, NOP, x, NOP), dict(rtol=float("nan"))),
                               ("negative atol", (NB, b, NOP, x, NOP), dict(atol=-1e-3)),
                               ("NaN atol", (NB, b, NOP, x, NOP), dict(atol=float("nan"))),
                               ("negative maxiter", (NB, b, NOP, x, NOP), dict(maxiter=-1, capacity=0)),
                               ("bad memspace", (NB, b, NOP, x, NOP), dict(memspace=2)),
                               ("struct size", (NB, b, NOP, x, NOP), dict(struct_size=8))]:
            assert raw_gm_solve(ptr, *args, stream=st, **kw)[0] == ERR_INVALID, what
        # X just behind the columns of B that are read is no overlap
        assert raw_gm_solve(ptr, NB, b, NOP, b + NB * NOP * es, NOP, rtol=1e-10, stream=st)[0] == 0
        # BSM_OK for every column status: 1 (maxiter), 2 (a NaN in b); the rows of the history beyond the count stay
        rc1, info1, cols1, h1 = raw_gm_solve(ptr, NB, b, NOP, x, NOP, rtol=1e-10, maxiter=2, capacity=4, stream=st)
        assert rc1 == 0 and info1.status == 1 and [c.status for c in cols1] == [1] * NB and [c.iterations for c in cols1] == [2] * NB
        assert np.all(h1[:2] > 0) and np.all(h1[2:] == -1)
        Bn = Bd.clone()
        Bn[3, 1] = float("nan")
        rc2, info2, cols2, _ = raw_gm_solve(ptr, NB, Bn.data_ptr(), NOP, x, NOP, rtol=1e-10, stream=st)
        assert rc2 == 0 and info2.status == 2 and [c.status for c in cols2] == [0, 2, 0, 0, 0] and cols2[1].iterations == 0
        # a capturing stream: refused before anything is enqueued, the capture stays valid
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            Xs.zero_()
            rc = raw_gm_solve(ptr, NB, b, NOP, x, NOP, stream=torch.cuda.current_stream().cuda_stream)[0]
        assert rc == ERR_INVALID
        torch.cuda.synchronize()
        # and without columns / history
        from bsm_amd import _lib as L
        prm = L.BsmCgParams(C.sizeof(L.BsmCgParams), 0, 1e-10, 0.0, 100, 0)
        info = L.BsmCgInfo()
        assert L.lib().bsm_gmres_multi_solve(ptr, NB, b, NOP, x, NOP, C.byref(prm), C.byref(info), None, None, 1, st) == 0
        assert info.status == 0 and info.columns_converged == NB and info.iterations == ok[1].iterations
    finally:
        assert raw_gm_destroy(ptr) == 0
    assert raw_gm_destroy(None) == 0


def test_an_operator_of_order_zero(torch_cuda, bsm):
    """n == 0: status 0, no iteration, nothing touched (B and X may be null)"""
    E = bsm.BlockSparseMatrix([], [], [], (0, 0))
    rc, ptr = raw_gm_create(E, 0, None, 0, CODE[np.dtype(np.float64)], 3, 5)
    assert rc == 0
    try:
        rc, info, cols, hist = raw_gm_solve(ptr, 3, None, 1, None, 1, stream=torch_cuda.cuda.current_stream().cuda_stream)
        assert rc == 0 and (info.status, info.iterations, info.columns_converged) == (0, 0, 3)
        assert [c.status for c in cols] == [0, 0, 0] and np.all(hist == -1)
    finally:
        assert raw_gm_destroy(ptr) == 0
