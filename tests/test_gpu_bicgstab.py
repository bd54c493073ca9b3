"""GPU suite of bsm_bicgstab_solve / BiCgStab: right-preconditioned BiCGSTAB on several right-hand sides in lockstep against
the numpy twin of tests/_bicgstab.py (same recurrences, none of the code) -- counts, true residuals, the operator's
direction, the freezing of finished columns, two passes over the matrix per iteration, the operator / vector pairings, the
layout edges of the kernels, the four statuses and the refusals.  The twin itself is tested in test_bicgstab_cpu.py."""
import numpy as np
import pytest

from _bicgstab import (BI_KINDS, EDGE, EDGE_IDS, ERR_INVALID, ERR_UNSUPPORTED, MAX_RHS, NB, NBI, SIGMA_ZERO, TS_ZERO, bicgstab_problem,
                       bicgstab_twin, breakdown_problem, check_columns, check_products, column_tol, edge_case, edge_problem, exact_minv,
                       is_complex, raw_bicgstab_create, raw_bicgstab_destroy, raw_bicgstab_solve, rtol_of, staggered, third_iterate_spread,
                       true_residual)
from _ctors import ctor_build
from _gpu import dev_copy, dev_mat, outside_bytes, torch_cuda, torch_dtype  # noqa: F401
from _jacobi import CODE, DTYPES, uniform
from _lockstep import solve_in_guarded_buffers

pytestmark = pytest.mark.gpu

CASES = [(k, dt) for k in BI_KINDS for dt in DTYPES]
CASE_IDS = [f"{k}-{np.dtype(dt).name}" for k, dt in CASES]
STAGGERED = {"float32": [8, 7, 6, 4, 0], "float64": [17, 14, 9, 4, 0]}


@pytest.fixture(scope="module")
def twins():
    """dtype name -> (D, B, Minv, [twin run per column]): the dense operator does not depend on its cut, so the reference
    is computed once per type and shared"""
    out = {}

    def get(dtype):
        key = np.dtype(dtype).name
        if key not in out:
            _, sets, D, B = bicgstab_problem("vbcrs", dtype)
            Minv = exact_minv(D, sets)
            out[key] = (D, B, Minv, [bicgstab_twin(D, B[:, c], Minv, rtol_of(dtype), 0.0, 100, dtype) for c in range(NB)])
        return out[key]
    return get


# ---- 1. against the twin -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, dtype", CASES, ids=CASE_IDS)
def test_against_the_twin(torch_cuda, bsm, twins, kind, dtype):
    torch = torch_cuda
    p, sets, D, B = bicgstab_problem(kind, dtype)
    _, _, _, runs = twins(dtype)
    rtol = rtol_of(dtype)
    A = bsm.synthetic.build(p)
    M = bsm.block_jacobi(A, sets)
    S = bsm.BiCgStab(A, M, nrhs=NB)
    X, info = S.solve(dev_copy(torch, B), rtol=rtol, maxiter=100)
    check_columns(info, runs, D, X.cpu().numpy(), B, [column_tol(B[:, c], rtol) for c in range(NB)], CASE_IDS[CASES.index((kind, dtype))])
    check_products(info, True)
    assert info.history.shape == (info.iterations, NB)
    for c in range(NB):
        k = int(info.column_iterations[c])
        assert info.history[k - 1, c] == info.residual[c] <= rtol * info.bnorm[c] and np.all(info.history[:k - 1, c] > rtol * info.bnorm[c])
        assert abs(info.bnorm[c] - np.linalg.norm(B[:, c].astype(np.complex128))) <= NBI * np.finfo(dtype).eps * info.bnorm[c]
    assert info.workspace != 0 and info.workspace_bytes >= 7 * NB * NBI * np.dtype(dtype).itemsize


# ---- 2. the operator's direction -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.complex64], ids=["float64", "complex64"])
def test_transpose_of_a_nonsymmetric_operator(torch_cuda, bsm, dtype):
    """bicgstab(transpose(A), B) solves D^T X = B: the twin runs on D.T, and the true residual against D.T would be of the
    order of ||b|| had the product gone the other way"""
    torch = torch_cuda
    p, sets, D, B = bicgstab_problem("blocksparse", dtype)
    rtol = rtol_of(dtype)
    Dt = np.ascontiguousarray(D.T)
    Minv = exact_minv(Dt, sets)
    runs = [bicgstab_twin(Dt, B[:, c], Minv, rtol, 0.0, 100, dtype) for c in range(NB)]
    A = bsm.transpose(bsm.synthetic.build(p))
    M = bsm.block_jacobi(A, sets)
    X, info = bsm.bicgstab(A, dev_copy(torch, B), M=M, rtol=rtol, maxiter=100)
    xh = X.cpu().numpy()
    tols = [column_tol(B[:, c], rtol) for c in range(NB)]
    check_columns(info, runs, Dt, xh, B, tols, f"transpose {np.dtype(dtype).name}")
    check_products(info, True)
    assert all(true_residual(D, xh[:, c], B[:, c]) > 100 * tols[c] for c in range(NB)), "D and D^T are not told apart by this problem"


# ---- 3. staggered columns --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", BI_KINDS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_staggered_columns(torch_cuda, bsm, kind, dtype):
    torch = torch_cuda
    p, sets, D, B = bicgstab_problem(kind, dtype)
    Bs, atol = staggered(B, dtype)
    Minv = exact_minv(D, sets)
    runs = [bicgstab_twin(D, Bs[:, c], Minv, 0.0, atol, 100, dtype) for c in range(NB)]
    assert [r.iterations for r in runs] == STAGGERED[np.dtype(dtype).name]
    A = bsm.synthetic.build(p)
    M = bsm.block_jacobi(A, sets)
    X, info = bsm.BiCgStab(A, M, nrhs=NB).solve(dev_copy(torch, Bs), rtol=0.0, atol=atol, maxiter=100)
    xh = X.cpu().numpy()
    check_columns(info, runs, D, xh, Bs, [atol] * NB, f"staggered {kind} {np.dtype(dtype).name}")
    assert info.column_iterations[4] == 0 and np.all(xh[:, 4] == 0) and info.bnorm[4] == 0
    assert info.iterations == max(info.column_iterations) and info.history.shape == (info.iterations, NB)
    for c in range(4):
        k = int(info.column_iterations[c])
        assert np.all(info.history[k - 1:, c] == info.history[k - 1, c]), ("a finished column's history moves", c)
        assert info.history[k - 1, c] <= atol and (k < 2 or info.history[k - 2, c] > atol)
    check_products(info, True)


# ---- 4. freezing holds -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_freezing_holds(torch_cuda, bsm, dtype):
    """what the host enqueues beyond a column's last iteration changes nothing: on the staggered columns a solve cut by
    maxiter after the first columns converged leaves them the bytes of the free-running solve, whose later iterations ran
    their products over them; and two free-running solves on one solver give the same bytes everywhere"""
    torch = torch_cuda
    p, sets, D, B = bicgstab_problem("vbcrs", dtype)
    Bs, atol = staggered(B, dtype)
    A = bsm.synthetic.build(p)
    M = bsm.block_jacobi(A, sets)
    Bd = dev_copy(torch, Bs)
    Y1, Y2 = (torch.empty((NB, NBI), dtype=Bd.dtype, device="cuda").t() for _ in range(2))
    for H in (A, M):
        bsm.mul(Y1, H, Bd)
        bsm.mul(Y2, H, Bd)
        torch.cuda.synchronize()
        assert Y1.cpu().numpy().tobytes() == Y2.cpu().numpy().tobytes(), "the products of this handle are not reproducible"
    S = bsm.BiCgStab(A, M, nrhs=NB)
    x1, i1 = S.solve(Bd, rtol=0.0, atol=atol, maxiter=400)
    assert i1.status == 0 and 1 <= i1.iterations < 100
    cut = int(i1.column_iterations[2])  # columns 2, 3, 4 have converged by then; 0 and 1 have not
    assert i1.column_iterations[3] < cut < i1.column_iterations[1]
    x2, i2 = S.solve(Bd, rtol=0.0, atol=atol, maxiter=cut)
    assert i2.column_status.tolist() == [1, 1, 0, 0, 0] and i2.iterations == cut
    assert i2.column_iterations.tolist()[2:] == i1.column_iterations.tolist()[2:]
    h1, h2 = x1.cpu().numpy(), x2.cpu().numpy()
    assert h1[:, 2:].tobytes() == h2[:, 2:].tobytes(), "a frozen column moved"
    assert np.array_equal(i1.history[:cut], i2.history)
    x3, i3 = S.solve(Bd, rtol=0.0, atol=atol, maxiter=400)
    assert h1.tobytes() == x3.cpu().numpy().tobytes() and np.array_equal(i1.history, i3.history)


# ---- 5. two passes over the matrix per iteration ---------------------------------------------------------------------------
def test_two_passes_per_iteration(torch_cuda, bsm):
    torch, dtype, K = torch_cuda, np.float64, 8
    p, sets, D, B = bicgstab_problem("vbcrs", dtype)
    B8 = np.asfortranarray(np.concatenate([B, uniform(np.random.default_rng(6100), (NBI, K - NB), dtype)], axis=1))
    A = bsm.synthetic.build(p, storage=np.float32)  # value_passes counts the sweeps over a mixed-storage image
    M = bsm.block_jacobi(A, sets)
    Bd = dev_copy(torch, B8)
    Y = torch.empty((K, NBI), dtype=Bd.dtype, device="cuda").t()
    before = A.value_passes()
    bsm.mul(Y, A, Bd)
    assert A.value_passes() == before + 1, "a plain 8-column product does not stream the matrix once"
    S = bsm.BiCgStab(A, M, nrhs=K)
    before = A.value_passes()
    X, first = S.solve(Bd, rtol=1e-10, maxiter=100)
    assert first.status == 0
    # the free-running solve had one more iteration enqueued when the last record arrived (the look-ahead): at most two
    # more products on frozen columns, which a_products does not count
    assert 0 <= A.value_passes() - before - first.a_products <= 2
    before = A.value_passes()
    X, info = S.solve(Bd, rtol=1e-10, maxiter=int(first.iterations))
    assert info.status == 0 and info.iterations == first.iterations
    assert A.value_passes() - before == info.a_products == 2 * info.iterations
    check_products(info, True)


# ---- 6. pairings -----------------------------------------------------------------------------------------------------------
def test_real_operators_with_complex_right_hand_sides(torch_cuda, bsm):
    torch = torch_cuda
    p, sets, D, B = bicgstab_problem("blocksparse", np.float64)
    Bc = np.asfortranarray((B + 1j * uniform(np.random.default_rng(6200), B.shape, np.float64)).astype(np.complex128))
    A = bsm.synthetic.build(p)
    M = bsm.block_jacobi(A, sets)
    S = bsm.BiCgStab(A, M, nrhs=NB, dtype=np.complex128)
    X, info = S.solve(dev_copy(torch, Bc), rtol=1e-10, maxiter=100)
    assert X.dtype == torch.complex128
    Dc, Minv = D.astype(np.complex128), exact_minv(D, sets).astype(np.complex128)
    runs = [bicgstab_twin(Dc, Bc[:, c], Minv, 1e-10, 0.0, 100, np.complex128) for c in range(NB)]
    check_columns(info, runs, Dc, X.cpu().numpy(), Bc, [column_tol(Bc[:, c], 1e-10) for c in range(NB)], "real A and M, complex B")
    check_products(info, True)
    with pytest.raises(TypeError):
        S.solve(dev_copy(torch, B))  # float64 columns into a complex128 solver


def test_single_precision_storage_under_double_vectors(torch_cuda, bsm):
    torch = torch_cuda
    p, sets, D, B = bicgstab_problem("vbcrs", np.float64)
    D32 = D.astype(np.float32).astype(np.float64)  # the operator IS the rounded one
    A = bsm.synthetic.build(p, storage=np.float32)
    M = bsm.block_jacobi(A, sets)
    X, info = bsm.BiCgStab(A, M, nrhs=NB).solve(dev_copy(torch, B), rtol=1e-10, maxiter=100)
    assert X.dtype == torch.float64
    Minv = exact_minv(D32, sets)
    runs = [bicgstab_twin(D32, B[:, c], Minv, 1e-10, 0.0, 100, np.float64) for c in range(NB)]
    check_columns(info, runs, D32, X.cpu().numpy(), B, [column_tol(B[:, c], 1e-10) for c in range(NB)], "float32 storage")


# ---- 7. solve variants -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=[np.dtype(d).name for d in DTYPES])
def test_initial_guess_close_to_the_solution(torch_cuda, bsm, dtype):
    torch = torch_cuda
    p, sets, D, B = bicgstab_problem("blocksparse", dtype)
    rtol = rtol_of(dtype)
    wide = np.complex128 if is_complex(dtype) else np.float64
    sol = np.linalg.solve(D.astype(wide), B.astype(wide))
    noise = uniform(np.random.default_rng(6300), B.shape, dtype)
    X0 = np.asfortranarray((sol + 1e-2 * np.max(np.abs(sol)) * noise).astype(dtype))
    Minv = exact_minv(D, sets)
    runs = [bicgstab_twin(D, B[:, c], Minv, rtol, 0.0, 100, dtype, x0=X0[:, c]) for c in range(NB)]
    A = bsm.synthetic.build(p)
    M = bsm.block_jacobi(A, sets)
    S = bsm.BiCgStab(A, M, nrhs=NB)
    X, info = S.solve(dev_copy(torch, B), X0=dev_copy(torch, X0), rtol=rtol, maxiter=100)
    check_columns(info, runs, D, X.cpu().numpy(), B, [column_tol(B[:, c], rtol) for c in range(NB)], f"x0 {np.dtype(dtype).name}")
    check_products(info, True, use_x0=True)


def test_host_matrices_and_a_side_stream(torch_cuda, bsm, twins):
    torch, dtype = torch_cuda, np.float64
    p, sets, D, B = bicgstab_problem("vbcrs", dtype)
    _, _, _, runs = twins(dtype)
    tols = [column_tol(B[:, c], 1e-10) for c in range(NB)]
    A = bsm.synthetic.build(p)
    M = bsm.block_jacobi(A, sets)
    S = bsm.BiCgStab(A, M, nrhs=NB)
    Xh = np.full(B.shape, np.nan, dtype=dtype, order="F")
    got, info = S.solve(B, X=Xh, rtol=1e-10, maxiter=100)  # numpy: staged
    assert got is Xh
    check_columns(info, runs, D, Xh, B, tols, "numpy B")
    xv, iv = S.solve(np.ascontiguousarray(B[:, 1]), rtol=1e-10, maxiter=100)  # a host vector in, a vector out
    assert xv.shape == (NBI,) and iv.column_status.tolist() == [0] and true_residual(D, xv, B[:, 1]) <= 2 * tols[1]
    Bd = dev_copy(torch, B)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    Xs, info = S.solve(Bd, rtol=1e-10, maxiter=100, stream=side)
    check_columns(info, runs, D, Xs.cpu().numpy(), B, tols, "side stream")
    with pytest.raises(ValueError):
        S.solve(Bd, X=np.zeros(B.shape, dtype, order="F"))  # B on the device, X on the host
    with pytest.raises(ValueError):
        bsm.BiCgStab(A, M, nrhs=2).solve(Bd)  # more columns than the solver holds


# ---- 8. layout edges of the kernels ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype, n, k", EDGE, ids=EDGE_IDS)
def test_layout_edges(torch_cuda, bsm, dtype, n, k):
    """small nonsymmetric block-diagonal operators (blocks T + 8 I of order <= 8), no preconditioner, every column against
    the twin; the solver holds 16 columns whatever k is (nrhs < nrhs_max)"""
    torch = torch_cuda
    p, Dop, B16, runs16 = edge_case(n, dtype)
    B, runs = np.asfortranarray(B16[:, :k]), runs16[:k]
    rtol = rtol_of(dtype)
    A = bsm.synthetic.build(p)
    S = bsm.BiCgStab(A, nrhs=MAX_RHS)
    xh, info = solve_in_guarded_buffers(torch, bsm, S, B, MAX_RHS)
    Dw = Dop.astype(np.complex128)
    for c, run in enumerate(runs):
        assert run.status == 0 and info.column_status[c] == 0, (c, info.column_status[c])
        assert abs(int(info.column_iterations[c]) - run.iterations) <= 1, (c, info.column_iterations[c], run.iterations)
        true = float(np.linalg.norm(B[:, c].astype(np.complex128) - Dw @ xh[:, c].astype(np.complex128)))
        assert true <= 2 * column_tol(B[:, c], rtol), (c, true)
    check_products(info, False)


def test_a_workgroup_walks_several_tiles(torch_cuda, bsm):
    """n = 600 000 float64: 300 000 sixteen-byte groups on the 256 workgroups the grid is capped at, 1172 each -- three tiles
    of 512 in bicg_start, bicg_half, bicg_update and bicg_dir, two of 1024 in bicg_dot"""
    torch, dtype, n = torch_cuda, np.float64, 600000
    p, Dop, rng = edge_problem(n, dtype)
    b = uniform(rng, (n,), dtype)
    run = bicgstab_twin(Dop, b, None, 1e-10, 0.0, 200, dtype)
    A = bsm.synthetic.build(p)
    x, info = bsm.bicgstab(A, torch.from_numpy(b).cuda(), rtol=1e-10, maxiter=200)
    assert run.status == 0 and info.column_status[0] == 0 and abs(int(info.iterations) - run.iterations) <= 1
    assert float(np.linalg.norm(b - Dop @ x.cpu().numpy())) <= 2 * column_tol(b, 1e-10)


# ---- 9. statuses -------------------------------------------------------------------------------------------------------------
def test_maxiter_gives_status_1_and_the_twins_iterate(torch_cuda, bsm):
    """float64, the layout-edge operator at n = 256, column 0, no preconditioner, three iterations: x is the twin's third
    iterate to 4 times what the twin moves by itself under eight permuted summation orders (measured here, not fixed in
    advance: 1.69 eps max|x| when this was written, so a bound of 6.8 eps) -- the device's tree sums and multi-column
    product are further permutations, not another method"""
    torch, dtype = torch_cuda, np.float64
    p, Dop, B16, _ = edge_case(256, dtype)
    b = np.ascontiguousarray(B16[:, 0])
    run, spread = third_iterate_spread()
    A = bsm.synthetic.build(p)
    x, info = bsm.bicgstab(A, torch.from_numpy(b).cuda(), rtol=0.0, maxiter=3)
    assert run.status == 1 and info.status == 1 and not info.converged and info.column_status.tolist() == [1]
    assert info.iterations == 3 and info.column_iterations.tolist() == [3] and info.history.shape == (3, 1)
    assert info.columns_converged == 0 and (info.a_products, info.m_products) == (6, 0)
    dev = np.max(np.abs(x.cpu().numpy() - run.iterates[2])) / (np.finfo(dtype).eps * np.max(np.abs(run.iterates[2])))
    print(f"BICGSTAT third iterate against the twin's: {dev:.2f} eps max|x|; the twin under permuted sums: {spread:.2f}; bound {4 * spread:.2f}")
    assert dev <= 4 * spread
    assert np.allclose(info.history[:, 0], run.history, rtol=1e-10)
    x0, i0 = bsm.bicgstab(A, torch.from_numpy(b).cuda(), maxiter=0)
    assert (i0.status, i0.iterations) == (1, 0) and torch.count_nonzero(x0).item() == 0 and len(i0.history) == 0


@pytest.mark.parametrize("dtype", [np.float64, np.complex64], ids=["float64", "complex64"])
def test_breakdown_freezes_its_column_only(torch_cuda, bsm, dtype):
    """exact 2 x 2 blocks with b = e1.  [[0, 1], [1, 0]]: sigma = 0 at the top of iteration 1 -- status 3, no iteration,
    x = 0.  [[1, 1], [-1, 0]]: ts = 0 after the half step -- status 3, one iteration, x = e1, residual 1.  No NaN; the
    other column of the same solve, on the other blocks of the operator, converges as the twin's does"""
    torch = torch_cuda
    for block, its, x00 in ((SIGMA_ZERO, 0, 0.0), (TS_ZERO, 1, 1.0)):
        p, D, B = breakdown_problem(block, dtype)
        good = bicgstab_twin(D, B[:, 1], None, 1e-6, 0.0, 50, dtype)
        A = bsm.synthetic.build(p)
        X, info = bsm.BiCgStab(A, nrhs=2).solve(dev_copy(torch, B), rtol=1e-6, maxiter=50)
        xh = X.cpu().numpy()
        assert info.column_status.tolist() == [3, 0] and info.status == 3 and info.columns_converged == 1, block
        assert int(info.column_iterations[0]) == its and abs(int(info.column_iterations[1]) - good.iterations) <= 1
        assert xh[0, 0] == x00 and np.all(xh[1:, 0] == 0) and info.residual[0] == 1
        assert true_residual(D, xh[:, 1], B[:, 1]) <= 2 * column_tol(B[:, 1], 1e-6)
        assert np.all(np.isfinite(info.history)) and np.all(info.history[:, 0] == 1.0)


def test_nan_in_one_column_gives_status_2_for_it_only(torch_cuda, bsm, twins):
    torch, dtype = torch_cuda, np.float32
    p, sets, D, B = bicgstab_problem("blocksparse", dtype)
    _, _, _, runs = twins(dtype)
    Bn = B.copy(order="F")
    Bn[17, 2] = np.nan
    A = bsm.synthetic.build(p)
    M = bsm.block_jacobi(A, sets)
    S = bsm.BiCgStab(A, M, nrhs=NB)
    X, info = S.solve(dev_copy(torch, Bn), rtol=rtol_of(dtype), maxiter=100)
    xh = X.cpu().numpy()
    assert info.column_status.tolist() == [0, 0, 2, 0, 0] and info.status == 2 and info.columns_converged == 4
    assert info.column_iterations[2] == 0 and not np.isfinite(info.bnorm[2]) and np.all(xh[:, 2] == 0)
    for c in (0, 1, 3, 4):
        assert abs(int(info.column_iterations[c]) - runs[c].iterations) <= 1
        assert true_residual(D, xh[:, c], B[:, c]) <= 2 * column_tol(B[:, c], rtol_of(dtype))
    # and the solver is usable afterwards
    X, info = S.solve(dev_copy(torch, B), rtol=rtol_of(dtype), maxiter=100)
    assert info.column_status.tolist() == [0] * NB


# ---- 10. refusals, through raw ctypes -----------------------------------------------------------------------------------------
def test_refusals(torch_cuda, bsm):
    torch, dtype = torch_cuda, np.float64
    f64 = CODE[np.dtype(dtype)]
    p, sets, D, B = bicgstab_problem("blocksparse", dtype)
    A = bsm.synthetic.build(p)
    M = bsm.block_jacobi(A, sets)
    A2 = ctor_build(bsm, "blocksparse", p, devices=[0, 0])
    assert raw_bicgstab_create(A2, 0, None, 0, f64, 4)[0] == ERR_UNSUPPORTED
    assert raw_bicgstab_create(A, 0, A2, 0, f64, 4)[0] == ERR_UNSUPPORTED
    small = bsm.BlockSparseMatrix([np.eye(3)], [[1, 2, 3]], [[1, 2, 3]], (3, 3))
    assert raw_bicgstab_create(A, 0, small, 0, f64, 4)[0] == ERR_INVALID
    pc, _, _, _ = bicgstab_problem("vbcrs", np.complex128)
    Ac = bsm.synthetic.build(pc)
    assert raw_bicgstab_create(Ac, 0, None, 0, f64, 4)[0] == ERR_INVALID
    assert raw_bicgstab_create(A, 0, Ac, 0, f64, 4)[0] == ERR_INVALID
    with pytest.raises(bsm._lib.BsmError, match="multi-device"):
        bsm.BiCgStab(A2)
    rc, ptr = raw_bicgstab_create(A, 0, M, 0, f64, MAX_RHS)
    assert rc == 0 and ptr.value
    try:
        Bd = dev_copy(torch, np.asfortranarray(np.concatenate([B] * 4, axis=1)))  # 20 columns
        Xs = torch.zeros((20, NBI), dtype=Bd.dtype, device="cuda")
        Xd = Xs.t()
        st = torch.cuda.current_stream().cuda_stream
        b, x, es = Bd.data_ptr(), Xd.data_ptr(), 8
        ok = raw_bicgstab_solve(ptr, NB, b, NBI, x, NBI, rtol=1e-10, stream=st)
        assert ok[0] == 0 and ok[1].status == 0
        for what, args, kw in [("nrhs 0", (0, b, NBI, x, NBI), {}), ("nrhs 17", (17, b, NBI, x, NBI), {}),
                               ("ldx < n", (NB, b, NBI, x, NBI - 1), {}), ("ldb < n", (NB, b, NBI - 1, x, NBI), {}),
                               ("X is B", (NB, b, NBI, b, NBI), {}),
                               ("X overlaps the last column of B", (NB, b, NBI, b + (NB * NBI - 8) * es, NBI), {}),
                               ("null B", (NB, None, NBI, x, NBI), {}), ("null X", (NB, b, NBI, None, NBI), {}),
                               ("negative rtol", (NB, b, NBI, x, NBI), dict(rtol=-1.0)),
                               ("negative atol", (NB, b, NBI, x, NBI), dict(atol=-1e-3)),
                               ("NaN atol", (NB, b, NBI, x, NBI), dict(atol=float("nan"))),
                               ("negative maxiter", (NB, b, NBI, x, NBI), dict(maxiter=-1, capacity=0)),
                               ("bad memspace", (NB, b, NBI, x, NBI), dict(memspace=2)),
                               ("struct size", (NB, b, NBI, x, NBI), dict(struct_size=8))]:
            assert raw_bicgstab_solve(ptr, *args, stream=st, **kw)[0] == ERR_INVALID, what
        # X just behind the columns of B that are read is no overlap
        assert raw_bicgstab_solve(ptr, NB, b, NBI, b + NB * NBI * es, NBI, rtol=1e-10, stream=st)[0] == 0
        # BSM_OK for every column status: 1 (maxiter), 2 (a NaN in b); 3 at the end of this test
        rc1, info1, cols1, _ = raw_bicgstab_solve(ptr, NB, b, NBI, x, NBI, rtol=1e-10, maxiter=2, stream=st)
        assert rc1 == 0 and info1.status == 1 and [c.status for c in cols1] == [1] * NB
        Bn = Bd.clone()
        Bn[3, 1] = float("nan")
        rc2, info2, cols2, _ = raw_bicgstab_solve(ptr, NB, Bn.data_ptr(), NBI, x, NBI, rtol=1e-10, stream=st)
        assert rc2 == 0 and info2.status == 2 and [c.status for c in cols2] == [0, 2, 0, 0, 0]
        # a capturing stream: refused before anything is enqueued, the capture stays valid
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            Xs.zero_()
            rc = raw_bicgstab_solve(ptr, NB, b, NBI, x, NBI, stream=torch.cuda.current_stream().cuda_stream)[0]
        assert rc == ERR_INVALID
        torch.cuda.synchronize()
        # and without columns / history
        from bsm_amd import _lib as L
        import ctypes as C
        prm = L.BsmCgParams(C.sizeof(L.BsmCgParams), 0, 1e-10, 0.0, 100, 0)
        info = L.BsmCgInfo()
        assert L.lib().bsm_bicgstab_solve(ptr, NB, b, NBI, x, NBI, C.byref(prm), C.byref(info), None, None, 1, st) == 0
        assert info.status == 0 and info.columns_converged == NB and info.iterations == ok[1].iterations
    finally:
        assert raw_bicgstab_destroy(ptr) == 0
    # status 3 through the raw driver
    pb, Db, Bb = breakdown_problem(SIGMA_ZERO, dtype)
    Ab = bsm.synthetic.build(pb)
    rc, ptr = raw_bicgstab_create(Ab, 0, None, 0, f64, 2)
    assert rc == 0
    try:
        nb = Bb.shape[0]
        Bbd, Xb = dev_copy(torch, Bb), torch.zeros((2, nb), dtype=torch.float64, device="cuda").t()
        rc3, info3, cols3, _ = raw_bicgstab_solve(ptr, 2, Bbd.data_ptr(), nb, Xb.data_ptr(), nb, rtol=1e-6, maxiter=50,
                                                  stream=torch.cuda.current_stream().cuda_stream)
        assert rc3 == 0 and info3.status == 3 and [c.status for c in cols3] == [3, 0]
    finally:
        assert raw_bicgstab_destroy(ptr) == 0
