"""GPU suite of bsm_minres_solve / Minres: symmetric-preconditioned MINRES on several right-hand sides in lockstep against
the numpy twin of tests/_minres.py (same recurrences, none of the code) on symmetric / Hermitian INDEFINITE operators --
counts and true residuals, the iterate after four iterations over the (G, K) grid of _lockstep.py to MARGIN times what the
twin moves under permuted sums, the decisions and the freezing of finished columns, one pass over the matrix per
iteration, breakdown, the layout edges, the operator / vector pairings and the refusals.  The twin itself is tested in
test_minres_cpu.py.  The figures are printed in MRSTAT lines before they are asserted."""
import ctypes as C

import numpy as np
import pytest

from _cg import ERR_DEVICE, ERR_INVALID, ERR_UNSUPPORTED, MAX_RHS, NB, NCG, column_tol, is_complex
from _ctors import ctor_build
from _gpu import dev_copy, torch_cuda  # noqa: F401
from _jacobi import CODE, uniform
from _krylov import exact_minv, rtol_of, true_residual
from _lockstep import (COLUMNS, ITS, MARGIN, RANGE_BYTES, TABLE, block_solve, deviation, half_sets, krylov_grid, path_rtol, reference_of,
                       solve_in_guarded_buffers, staggered6)
from _minres import (BROKEN_COUNTS, check_columns, check_products, indef_case, minres_problem, minres_twin, raw_minres_create,
                     raw_minres_destroy, raw_minres_solve)

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64, np.complex64, np.complex128]
CASES = [(k, dt) for k in ("vbcrs", "blocksparse", "symmetric") for dt in DTYPES if not (k == "symmetric" and is_complex(dt))]
CASE_IDS = [f"{k}-{np.dtype(dt).name}" for k, dt in CASES]

_twins, _built, _refs, _spreads = {}, {}, {}, {}


def name(dtype):
    return np.dtype(dtype).name


def twins(dtype):
    """(D, P, B, sets, Minv, [twin run per column]) of the order-400 problem: the dense operator does not depend on its
    cut, so the reference is computed once per type and shared"""
    key = name(dtype)
    if key not in _twins:
        _, _, sets, D, P, B = minres_problem("vbcrs", dtype)
        Minv = exact_minv(P, sets)
        _twins[key] = (D, P, B, sets, Minv, [minres_twin(D, B[:, c], Minv, rtol_of(dtype), 0.0, 200, dtype) for c in range(NB)])
    return _twins[key]


def build_400(bsm, kind, dtype, **kw):
    """-> (A, M): the indefinite operator and block_jacobi of its definite sibling"""
    p, pp, sets, _, _, _ = minres_problem(kind, dtype)
    return bsm.synthetic.build(p, **kw), bsm.block_jacobi(bsm.synthetic.build(pp, **kw), sets)


# ---- 1. against the twin, order 400 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, dtype", CASES, ids=CASE_IDS)
def test_against_the_twin(torch_cuda, bsm, kind, dtype):
    torch = torch_cuda
    D, _, B, _, _, runs = twins(dtype)
    rtol = rtol_of(dtype)
    A, M = build_400(bsm, kind, dtype)
    S = bsm.Minres(A, M, nrhs=NB)
    X, info = S.solve(dev_copy(torch, B), rtol=rtol, maxiter=200)
    check_columns(info, runs, D, X.cpu().numpy(), B, [column_tol(B[:, c], rtol) for c in range(NB)], f"{kind}-{name(dtype)}")
    check_products(info, True)
    assert info.history.shape == (info.iterations, NB)
    for c in range(NB):
        k = int(info.column_iterations[c])
        assert info.history[k - 1, c] == info.residual[c] <= rtol * info.bnorm[c] < info.history[k - 2, c]
        assert abs(info.bnorm[c] - np.linalg.norm(B[:, c].astype(np.complex128))) <= NCG * np.finfo(dtype).eps * info.bnorm[c]
    assert info.workspace != 0 and info.workspace_bytes >= 9 * NB * NCG * np.dtype(dtype).itemsize


# ---- 2. iterate and history after 4 iterations on the (G, K) grid ------------------------------------------------------------
def operators(bsm, n, dtype):
    """the device operator of indef_case(n, dtype) and its definite sibling, built once"""
    key = (n, name(dtype))
    if key not in _built:
        p, _, ps, _, _ = indef_case(n, dtype)
        _built[key] = (bsm.synthetic.build(p), bsm.synthetic.build(ps))
    return _built[key]


def twin_spread(Dop, b, dtype, Minv=None, x0=None, orders=8):
    """_lockstep.spread for minres_twin: the largest deviation() of the twin IN dtype under `orders` permuted summation
    orders from its unpermuted run -> (iterate: eps max|x|, history: eps ||b||)"""
    a = minres_twin(Dop, b, Minv, 0.0, 0.0, ITS, dtype, x0=x0)
    assert a.status == 1 and a.iterations == ITS
    sx = sh = 0.0
    for seed in range(orders):
        p = minres_twin(Dop, b, Minv, 0.0, 0.0, ITS, dtype, x0=x0, order=np.random.default_rng(seed).permutation(len(b)))
        dx, dh = deviation(p.x, p.history, a, ITS, dtype)
        sx, sh = max(sx, dx), max(sh, dh)
    return sx, sh


def check_iterates(tag, info, xh, Dop, B, dtype, k, Minv=None, X0=None):
    """every column of a solve cut at ITS iterations with rtol = 0: status 1, count ITS, x and the history within MARGIN x
    spread of the reference's (the twin on the operator and right-hand side as rounded to dtype, evaluated in
    reference_of(dtype)); references and the spread (of column 0) are computed once per tag"""
    if tag not in _spreads:
        _spreads[tag] = twin_spread(Dop, B[:, 0], dtype, Minv=Minv, x0=None if X0 is None else X0[:, 0])
    sx, sh = _spreads[tag]
    devs = []
    for c in range(k):
        if (tag, c) not in _refs:
            _refs[tag, c] = minres_twin(Dop, B[:, c], Minv, 0.0, 0.0, ITS, reference_of(dtype), x0=None if X0 is None else X0[:, c])
        ref = _refs[tag, c]
        assert ref.status == 1 and ref.iterations == ITS
        devs.append(deviation(xh[:, c], info.history[:, c], ref, ITS, dtype))
    dx, dh = max(d[0] for d in devs), max(d[1] for d in devs)
    print(f"MRSTAT {tag} K={k}: iterate {dx:.2f} eps max|x|, spread {sx:.2f}, used {dx / (MARGIN * sx):.2f} of the bound; history {dh:.2e} "
          f"eps ||b||, spread {sh:.2e}, used {dh / (MARGIN * sh):.2f}")
    assert info.column_status.tolist() == [1] * k and info.column_iterations.tolist() == [ITS] * k, (info.column_status, info.column_iterations)
    assert info.history.shape == (ITS, k)
    assert dx <= MARGIN * sx, (tag, [d[0] for d in devs], sx)
    assert dh <= MARGIN * sh, (tag, [d[1] for d in devs], sh)


GRID = [(dt, n, G) for dt, n, G in TABLE if G in ((2, 3, 65, 256) if np.finfo(dt).eps < 1e-10 else (2, 65, 256))]
ITER = [(dt, n, G, k) for dt, n, G in GRID for k in COLUMNS]


@pytest.mark.parametrize("dtype, n, G, k", ITER, ids=[f"{name(dt)}-n{n}-G{G}-k{k}" for dt, n, G, k in ITER])
def test_iterate_and_history_after_four_iterations(torch_cuda, bsm, dtype, n, G, k):
    assert krylov_grid(n, np.dtype(dtype).itemsize) == G
    _, Dop, _, _, B16 = indef_case(n, dtype)
    B = np.asfortranarray(B16[:, :k])
    S = bsm.Minres(operators(bsm, n, dtype)[0], nrhs=MAX_RHS)
    xh, info = solve_in_guarded_buffers(torch_cuda, bsm, S, B, MAX_RHS, rtol=0.0, maxiter=ITS)
    check_iterates(f"{name(dtype)} n={n} G={G}", info, xh, Dop, B, dtype, k)
    assert info.a_products == ITS and info.m_products == 0


PATHS = [(dt, n, G) for dt, n, G in GRID if G in (2, 3)]
PATH_IDS = [f"{name(dt)}-n{n}-G{G}" for dt, n, G in PATHS]


def both_checks(torch, bsm, tag, S, Dop, B, dtype, Minv=None, X0=None):
    """K = 3: the iterate check after ITS iterations, then (3.) once to path_rtol(dtype): the twin's count +-1 and the true
    residual <= 2 tol"""
    xh, info = solve_in_guarded_buffers(torch, bsm, S, B, MAX_RHS, X0=X0, rtol=0.0, maxiter=ITS)
    check_iterates(tag, info, xh, Dop, B, dtype, 3, Minv=Minv, X0=X0)
    rtol = path_rtol(dtype)
    xh, info = solve_in_guarded_buffers(torch, bsm, S, B, MAX_RHS, X0=X0, rtol=rtol, maxiter=200)
    runs = [minres_twin(Dop, B[:, c], Minv, rtol, 0.0, 200, dtype, x0=None if X0 is None else X0[:, c]) for c in range(3)]
    check_columns(info, runs, Dop.dense(), xh, B, [column_tol(B[:, c], rtol) for c in range(3)], tag + " to rtol")
    check_products(info, Minv is not None, X0 is not None)
    return info


@pytest.mark.parametrize("dtype, n, G", PATHS, ids=PATH_IDS)
def test_paths_without_a_preconditioner(torch_cuda, bsm, dtype, n, G):
    _, Dop, _, _, B16 = indef_case(n, dtype)
    S = bsm.Minres(operators(bsm, n, dtype)[0], nrhs=MAX_RHS)
    both_checks(torch_cuda, bsm, f"{name(dtype)} n={n} G={G}", S, Dop, np.asfortranarray(B16[:, :3]), dtype)


@pytest.mark.parametrize("dtype, n, G", PATHS, ids=PATH_IDS)
def test_paths_with_a_preconditioner(torch_cuda, bsm, dtype, n, G):
    """M = block_jacobi of the definite sibling over the HALVES of its 8-blocks: positive definite, not the inverse of
    anything here; the twin takes the exact block inverse"""
    _, Dop, _, Dsib, B16 = indef_case(n, dtype)
    sets = half_sets(n)
    A, P = operators(bsm, n, dtype)
    S = bsm.Minres(A, bsm.block_jacobi(P, sets), nrhs=MAX_RHS)
    info = both_checks(torch_cuda, bsm, f"M {name(dtype)} n={n} G={G}", S, Dop, np.asfortranarray(B16[:, :3]), dtype,
                       Minv=exact_minv(Dsib.dense(), sets))
    assert info.iterations > ITS


@pytest.mark.parametrize("dtype, n, G", PATHS, ids=PATH_IDS)
def test_paths_with_an_initial_guess(torch_cuda, bsm, dtype, n, G):
    """X0 = the solution plus 1e-2 noise, handed over in the guarded X buffer: the copy into the workspace and the start
    with q = A x0"""
    _, Dop, _, _, B16 = indef_case(n, dtype)
    B = np.asfortranarray(B16[:, :3])
    sol = block_solve(Dop, B)
    X0 = np.asfortranarray((sol + 1e-2 * np.max(np.abs(sol)) * uniform(np.random.default_rng(9200 + n), sol.shape, dtype)).astype(dtype))
    S = bsm.Minres(operators(bsm, n, dtype)[0], nrhs=MAX_RHS)
    both_checks(torch_cuda, bsm, f"x0 {name(dtype)} n={n} G={G}", S, Dop, B, dtype, X0=X0)


# ---- 4. decisions ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.complex128, np.float32], ids=["complex128", "float32"])
def test_decisions_across_workgroups(torch_cuda, bsm, dtype):
    """G = 65, six columns: four scaled so that they finish at four different counts under one absolute tolerance, one zero,
    one with a NaN in the last row (the LAST workgroup's range).  All 65 workgroups of a column must derive the same
    rotation and the same decision from the partials they add themselves: the statuses, the counts, the frozen histories,
    and the same bytes from a second solve cut at the largest count"""
    torch = torch_cuda
    n = 64 * (RANGE_BYTES // np.dtype(dtype).itemsize) + 1
    _, Dop, _, _, B16 = indef_case(n, dtype)
    tau, step = (1e-4, 10.0) if dtype == np.float32 else (1e-10, 1000.0)
    Bs, atol = staggered6(B16, dtype, tau, step)
    runs = [minres_twin(Dop, Bs[:, c], None, 0.0, atol, 200, dtype) for c in range(6)]
    counts = [r.iterations for r in runs]
    assert [r.status for r in runs] == [0, 0, 0, 0, 0, 2] and len(set(counts[:4])) == 4 and counts[4:] == [0, 0], counts
    A = operators(bsm, n, dtype)[0]
    b = torch.from_numpy(np.ascontiguousarray(Bs[:, 0])).cuda()
    y1, y2 = torch.empty_like(b), torch.empty_like(b)
    bsm.mul(y1, A, b)
    bsm.mul(y2, A, b)
    torch.cuda.synchronize()
    assert y1.cpu().numpy().tobytes() == y2.cpu().numpy().tobytes(), "the products of this handle are not reproducible"
    S = bsm.Minres(A, nrhs=MAX_RHS)
    xh, info = solve_in_guarded_buffers(torch, bsm, S, Bs, MAX_RHS, rtol=0.0, atol=atol, maxiter=200)
    print(f"MRSTAT decisions {name(dtype)} n={n}: counts {info.column_iterations.tolist()}, twin {counts}, statuses {info.column_status.tolist()}")
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


# ---- 5. one pass over A, and over M, per iteration ---------------------------------------------------------------------------
def test_one_pass_per_iteration(torch_cuda, bsm):
    torch, dtype, K = torch_cuda, np.float64, 8
    _, _, B, _, _, _ = twins(dtype)
    B8 = np.asfortranarray(np.concatenate([B, uniform(np.random.default_rng(4100), (NCG, K - NB), dtype)], axis=1))
    A, M = build_400(bsm, "vbcrs", dtype)
    Bd = dev_copy(torch, B8)
    Y = torch.empty((K, NCG), dtype=Bd.dtype, device="cuda").t()
    for H in (A, M):
        before = H.value_passes()
        bsm.mul(Y, H, Bd)
        assert H.value_passes() == before + 1, "a plain 8-column product does not stream the matrix once"
    S = bsm.Minres(A, M, nrhs=K)
    before = A.value_passes(), M.value_passes()
    X, first = S.solve(Bd, rtol=1e-10, maxiter=200)
    assert first.status == 0
    # the free-running solve had one more iteration enqueued when the last record arrived (the look-ahead): one more
    # product of A and of M on frozen columns, which the counts do not include
    assert A.value_passes() - before[0] == first.a_products + 1
    assert M.value_passes() - before[1] == first.m_products + 1
    before = A.value_passes(), M.value_passes()
    X, info = S.solve(Bd, rtol=1e-10, maxiter=int(first.iterations))
    assert info.status == 0 and info.iterations == first.iterations
    assert A.value_passes() - before[0] == info.a_products == info.iterations
    assert M.value_passes() - before[1] == info.m_products == info.iterations + 1
    check_products(info, True)


# ---- 6. breakdown ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=[name(d) for d in DTYPES])
def test_an_indefinite_preconditioner_gives_status_3(torch_cuda, bsm, dtype):
    """M = block_jacobi(D ITSELF, sets): <v, z> < 0 at the start or after the first Lanczos step, at the iteration
    test_minres_cpu.py pins for the twin; X holds no NaN"""
    torch = torch_cuda
    p, _, sets, D, _, B = minres_problem("blocksparse", dtype)
    A = bsm.synthetic.build(p)
    X, info = bsm.Minres(A, bsm.block_jacobi(A, sets), nrhs=NB).solve(dev_copy(torch, B), rtol=rtol_of(dtype), maxiter=200)
    xh = X.cpu().numpy()
    print(f"MRSTAT indefinite M {name(dtype)}: statuses {info.column_status.tolist()}, counts {info.column_iterations.tolist()}")
    assert info.column_status.tolist() == [3] * NB and info.status == 3 and info.columns_converged == 0
    assert info.column_iterations.tolist() == BROKEN_COUNTS[name(dtype)]
    assert np.all(np.isfinite(xh)) and np.all(np.isfinite(info.history)) and np.all(np.isfinite(info.residual))
    for c in range(NB):
        if info.column_iterations[c] == 0:
            assert np.all(xh[:, c] == 0)


@pytest.mark.parametrize("dtype", [np.float64, np.complex64], ids=["float64", "complex64"])
def test_breakdown_freezes_its_column_only(torch_cuda, bsm, dtype):
    """the singular [[0, 0], [0, 1]] with b = e1 (in its null space): delta = 0 and gamma_new = 0, so a1 = 0 -- status 3, no
    iteration, x = 0, no NaN -- while the column b = e2 of the same solve converges in one iteration.  And [[0, 1], [1, 0]]
    with b = e1, which breaks CG down, is solved in two"""
    torch = torch_cuda
    A = bsm.BlockSparseMatrix([np.asfortranarray(np.array([[0, 0], [0, 1]], dtype=dtype))], [[1, 2]], [[1, 2]], (2, 2))
    B = np.asfortranarray(np.array([[1, 0], [0, 1]], dtype=dtype))
    X, info = bsm.Minres(A, nrhs=2).solve(dev_copy(torch, B), rtol=1e-6, maxiter=10)
    xh = X.cpu().numpy()
    assert info.column_status.tolist() == [3, 0] and info.status == 3 and info.columns_converged == 1
    assert info.column_iterations.tolist() == [0, 1] and info.iterations == 1
    assert np.all(xh[:, 0] == 0) and xh[:, 1].tolist() == [0, 1] and info.residual[0] == 1 and info.residual[1] == 0
    assert np.all(np.isfinite(info.history)) and info.history[:, 0].tolist() == [1.0]
    swap = bsm.BlockSparseMatrix([np.asfortranarray(np.array([[0, 1], [1, 0]], dtype=dtype))], [[1, 2]], [[1, 2]], (2, 2))
    x, info = bsm.minres(swap, torch.from_numpy(np.array([1, 0], dtype=dtype)).cuda(), rtol=1e-6, maxiter=10)
    assert (info.status, info.iterations) == (0, 2) and x.cpu().numpy().tolist() == [0, 1] and info.history[:, 0].tolist() == [1.0, 0.0]


# ---- 7. layout edges ----------------------------------------------------------------------------------------------------------
EDGE = [(dt, n, k) for dt in DTYPES for n, k in ((1, 1), (3, 2))] + [(dt, n, 5) for dt, n, G in GRID if G == 2]


@pytest.mark.parametrize("dtype, n, k", EDGE, ids=[f"{name(d)}-n{n}-k{k}" for d, n, k in EDGE])
def test_layout_edges(torch_cuda, bsm, dtype, n, k):
    """B at ldb = n + 3, X one element past a 16-byte boundary, kmax = 16 > nrhs, inside NaN-filled buffers
    (solve_in_guarded_buffers asserts that nothing outside the n x nrhs window changes); every column against the twin"""
    _, Dop, _, _, B16 = indef_case(n, dtype)
    B = np.asfortranarray(B16[:, :k])
    rtol = path_rtol(dtype)
    runs = [minres_twin(Dop, B[:, c], None, rtol, 0.0, 200, dtype) for c in range(k)]
    S = bsm.Minres(operators(bsm, n, dtype)[0], nrhs=MAX_RHS)
    xh, info = solve_in_guarded_buffers(torch_cuda, bsm, S, B, MAX_RHS, rtol=rtol)
    check_columns(info, runs, Dop.dense(), xh, B, [column_tol(B[:, c], rtol) for c in range(k)], f"edges {name(dtype)} n={n}")
    check_products(info, False)


# ---- 8. pairings ----------------------------------------------------------------------------------------------------------------
def test_real_operators_with_complex_right_hand_sides(torch_cuda, bsm):
    torch = torch_cuda
    D, P, B, sets, _, _ = twins(np.float64)
    Bc = np.asfortranarray((B + 1j * uniform(np.random.default_rng(4200), B.shape, np.float64)).astype(np.complex128))
    A, M = build_400(bsm, "blocksparse", np.float64)
    S = bsm.Minres(A, M, nrhs=NB, dtype=np.complex128)
    X, info = S.solve(dev_copy(torch, Bc), rtol=1e-10, maxiter=200)
    assert X.dtype == torch.complex128
    Dc, Minv = D.astype(np.complex128), exact_minv(P, sets).astype(np.complex128)
    runs = [minres_twin(Dc, Bc[:, c], Minv, 1e-10, 0.0, 200, np.complex128) for c in range(NB)]
    check_columns(info, runs, Dc, X.cpu().numpy(), Bc, [column_tol(Bc[:, c], 1e-10) for c in range(NB)], "real A and M, complex B")
    check_products(info, True)
    with pytest.raises(TypeError):
        S.solve(dev_copy(torch, B))  # float64 columns into a complex128 solver


def test_single_precision_storage_under_double_vectors(torch_cuda, bsm):
    torch = torch_cuda
    D, P, B, sets, _, _ = twins(np.float64)
    D32, P32 = D.astype(np.float32).astype(np.float64), P.astype(np.float32).astype(np.float64)  # the operators ARE the rounded ones
    p, pp, _, _, _, _ = minres_problem("symmetric", np.float64)
    A = bsm.synthetic.build(p, storage=np.float32)
    M = bsm.block_jacobi(bsm.synthetic.build(pp, storage=np.float32), sets)
    X, info = bsm.Minres(A, M, nrhs=NB).solve(dev_copy(torch, B), rtol=1e-10, maxiter=200)
    assert X.dtype == torch.float64
    Minv = exact_minv(P32, sets)
    runs = [minres_twin(D32, B[:, c], Minv, 1e-10, 0.0, 200, np.float64) for c in range(NB)]
    check_columns(info, runs, D32, X.cpu().numpy(), B, [column_tol(B[:, c], 1e-10) for c in range(NB)], "float32 storage")


@pytest.mark.parametrize("wrapper", ["transpose", "adjoint"])
def test_wrappers_of_the_hermitian_problem(torch_cuda, bsm, wrapper):
    """adjoint(A) of the Hermitian A is A; transpose(A) is conj(A), Hermitian too, and its M is transpose(M): the solve of
    the wrapped operator against the twin on the wrapped dense operator"""
    torch, dtype = torch_cuda, np.complex128
    D, P, B, sets, _, _ = twins(dtype)
    A, M = build_400(bsm, "vbcrs", dtype)
    wrap = getattr(bsm, wrapper)
    Dw, Pw = (D.T, P.T) if wrapper == "transpose" else (D.conj().T, P.conj().T)
    X, info = bsm.minres(wrap(A), dev_copy(torch, B), M=wrap(M), rtol=1e-10, maxiter=200)
    Minv = exact_minv(np.ascontiguousarray(Pw), sets)
    runs = [minres_twin(np.ascontiguousarray(Dw), B[:, c], Minv, 1e-10, 0.0, 200, dtype) for c in range(NB)]
    check_columns(info, runs, Dw, X.cpu().numpy(), B, [column_tol(B[:, c], 1e-10) for c in range(NB)], wrapper)
    check_products(info, True)


# ---- 9. surface and refusals ------------------------------------------------------------------------------------------------------
def test_host_matrices_vectors_and_two_solves(torch_cuda, bsm):
    torch, dtype = torch_cuda, np.float64
    D, _, B, _, _, runs = twins(dtype)
    tols = [column_tol(B[:, c], 1e-10) for c in range(NB)]
    A, M = build_400(bsm, "vbcrs", dtype)
    S = bsm.Minres(A, M, nrhs=NB)
    Xh = np.full(B.shape, np.nan, dtype=dtype, order="F")
    got, info = S.solve(B, X=Xh, rtol=1e-10, maxiter=200)  # numpy: staged
    assert got is Xh
    check_columns(info, runs, D, Xh, B, tols, "numpy B")
    xv, iv = S.solve(np.ascontiguousarray(B[:, 1]), rtol=1e-10, maxiter=200)  # a host vector in, a vector out
    assert xv.shape == (NCG,) and iv.column_status.tolist() == [0] and true_residual(D, xv, B[:, 1]) <= 2 * tols[1]
    Bd = dev_copy(torch, B)
    X1, i1 = S.solve(Bd, rtol=1e-10, maxiter=200)
    X2, i2 = S.solve(Bd, rtol=1e-10, maxiter=200, history=False)  # a second solve on the same solver, without history
    assert X1.cpu().numpy().tobytes() == X2.cpu().numpy().tobytes() and i2.history.shape == (0, NB)
    assert i1.column_iterations.tolist() == i2.column_iterations.tolist() and np.array_equal(i1.residual, i2.residual)
    xd, idv = bsm.minres(A, Bd[:, 2].contiguous(), M=M, rtol=1e-10, maxiter=200)  # a device vector in, a vector out
    assert xd.shape == (NCG,) and idv.status == 0
    x0, i0 = bsm.minres(A, Bd[:, 0].contiguous(), maxiter=0)
    assert (i0.status, i0.iterations) == (1, 0) and torch.count_nonzero(x0).item() == 0 and len(i0.history) == 0
    with pytest.raises(ValueError):
        S.solve(Bd, X=np.zeros(B.shape, dtype, order="F"))  # B on the device, X on the host
    with pytest.raises(ValueError):
        bsm.Minres(A, M, nrhs=2).solve(Bd)  # more columns than the solver holds


def test_refusals(torch_cuda, bsm):
    torch, dtype = torch_cuda, np.float64
    f64 = CODE[np.dtype(dtype)]
    p, pp, sets, D, P, B = minres_problem("blocksparse", dtype)
    A, M = build_400(bsm, "blocksparse", dtype)
    assert raw_minres_create(None, 0, None, 0, f64, 4)[0] == ERR_INVALID  # null A
    from bsm_amd import _lib as L
    assert L.lib().bsm_minres_create(A._h.ptr, 0, None, 0, f64, 4, None) == ERR_INVALID  # null out
    assert L.lib().bsm_minres_destroy(None) == 0
    for opA, opM in ((3, 0), (-1, 0), (0, 3)):
        assert raw_minres_create(A, opA, M, opM, f64, 4)[0] == ERR_INVALID, (opA, opM)
    assert raw_minres_create(A, 0, None, 0, 7, 4)[0] == ERR_INVALID  # not a vector type
    for kmax in (0, MAX_RHS + 1):
        assert raw_minres_create(A, 0, None, 0, f64, kmax)[0] == ERR_INVALID
    tall = bsm.BlockSparseMatrix([np.asfortranarray(np.ones((3, 2)))], [[1, 2, 3]], [[1, 2]], (3, 2))
    assert raw_minres_create(tall, 0, None, 0, f64, 4)[0] == ERR_INVALID  # op(A) not square
    A2 = ctor_build(bsm, "blocksparse", p, devices=[0, 0])
    assert raw_minres_create(A2, 0, None, 0, f64, 4)[0] == ERR_UNSUPPORTED
    assert raw_minres_create(A, 0, A2, 0, f64, 4)[0] == ERR_UNSUPPORTED
    small = bsm.BlockSparseMatrix([np.eye(3)], [[1, 2, 3]], [[1, 2, 3]], (3, 3))
    assert raw_minres_create(A, 0, small, 0, f64, 4)[0] == ERR_INVALID  # the order of M
    Ac = bsm.synthetic.build(minres_problem("vbcrs", np.complex128)[0])
    assert raw_minres_create(Ac, 0, None, 0, f64, 4)[0] == ERR_INVALID  # a complex handle under real vectors
    assert raw_minres_create(A, 0, Ac, 0, f64, 4)[0] == ERR_INVALID
    assert raw_minres_create(A, 0, None, 0, CODE[np.dtype(np.complex64)], 4)[0] == ERR_INVALID  # a real handle of the other precision
    # a mixed pair: values stored in float32 under double vectors takes real vectors only, as A and as M
    c128 = CODE[np.dtype(np.complex128)]
    Am = bsm.synthetic.build(p, storage=np.float32)
    assert raw_minres_create(Am, 0, None, 0, c128, 4)[0] == ERR_INVALID
    assert raw_minres_create(A, 0, Am, 0, c128, 4)[0] == ERR_INVALID
    for args in ((Am, 0, None, 0, f64), (A, 0, Am, 0, f64), (A, 0, None, 0, c128)):  # ... and these pairs are taken
        rc, ptr = raw_minres_create(*args, 4)
        assert rc == 0 and raw_minres_destroy(ptr) == 0, args[1:]
    with pytest.raises(bsm._lib.BsmError, match="multi-device"):
        bsm.Minres(A2)
    An = bsm.synthetic.build(p, device=-2)  # BSM_DEVICE_NONE: analysis only
    assert raw_minres_create(An, 0, None, 0, f64, 4)[0] == ERR_DEVICE
    rc, ptr = raw_minres_create(A, 0, M, 0, f64, MAX_RHS)
    assert rc == 0 and ptr.value
    try:
        Bd = dev_copy(torch, np.asfortranarray(np.concatenate([B] * 4, axis=1)))  # 20 columns
        Xs = torch.zeros((20, NCG), dtype=Bd.dtype, device="cuda")
        Xd = Xs.t()
        st = torch.cuda.current_stream().cuda_stream
        b, x, es = Bd.data_ptr(), Xd.data_ptr(), 8
        ok = raw_minres_solve(ptr, NB, b, NCG, x, NCG, rtol=1e-10, maxiter=200, stream=st)
        assert ok[0] == 0 and ok[1].status == 0
        for what, args, kw in [("nrhs 0", (0, b, NCG, x, NCG), {}), ("nrhs 17", (17, b, NCG, x, NCG), {}),
                               ("ldx < n", (NB, b, NCG, x, NCG - 1), {}), ("ldb < n", (NB, b, NCG - 1, x, NCG), {}),
                               ("X is B", (NB, b, NCG, b, NCG), {}),
                               ("X overlaps the last column of B", (NB, b, NCG, b + (NB * NCG - 8) * es, NCG), {}),
                               ("null B", (NB, None, NCG, x, NCG), {}), ("null X", (NB, b, NCG, None, NCG), {}),
                               ("negative rtol", (NB, b, NCG, x, NCG), dict(rtol=-1.0)),
                               ("negative atol", (NB, b, NCG, x, NCG), dict(atol=-1e-3)),
                               ("NaN atol", (NB, b, NCG, x, NCG), dict(atol=float("nan"))),
                               ("negative maxiter", (NB, b, NCG, x, NCG), dict(maxiter=-1, capacity=0)),
                               ("bad memspace", (NB, b, NCG, x, NCG), dict(memspace=2)),
                               ("struct size", (NB, b, NCG, x, NCG), dict(struct_size=8))]:
            assert raw_minres_solve(ptr, *args, stream=st, **kw)[0] == ERR_INVALID, what
        assert raw_minres_solve(None, NB, b, NCG, x, NCG, stream=st)[0] == ERR_INVALID  # null S
        # X just behind the columns of B that are read is no overlap
        assert raw_minres_solve(ptr, NB, b, NCG, b + NB * NCG * es, NCG, rtol=1e-10, maxiter=200, stream=st)[0] == 0
        # without columns / history
        prm = L.BsmCgParams(C.sizeof(L.BsmCgParams), 0, 1e-10, 0.0, 200, 0)
        info = L.BsmCgInfo()
        assert L.lib().bsm_minres_solve(ptr, NB, b, NCG, x, NCG, C.byref(prm), C.byref(info), None, None, 1, st) == 0
        assert info.status == 0 and info.columns_converged == NB and info.iterations == ok[1].iterations
    finally:
        assert raw_minres_destroy(ptr) == 0
    # n == 0: status 0, nothing touched, B and X may be null
    A0 = bsm.BlockSparseMatrix([], [], [], (0, 0))
    rc, ptr = raw_minres_create(A0, 0, None, 0, f64, 2)
    assert rc == 0
    try:
        rc, info, cols, _ = raw_minres_solve(ptr, 2, None, 1, None, 1, stream=torch.cuda.current_stream().cuda_stream)
        assert rc == 0 and info.status == 0 and info.columns_converged == 2 and info.iterations == 0
    finally:
        assert raw_minres_destroy(ptr) == 0
