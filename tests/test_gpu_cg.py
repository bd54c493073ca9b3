"""GPU suite of bsm_cg_solve / Cg: preconditioned CG and COCG on several right-hand sides in lockstep against the numpy
twin of tests/_cg.py (same recurrences, none of the code) -- counts, true residuals, the freezing of finished columns,
one pass over the matrix per iteration, the operator / vector pairings, the layout edges of the kernels, the four
statuses and the refusals.  The twin itself is tested in test_cg_cpu.py."""
import numpy as np
import pytest

from _cg import (CG, COCG, ERR_INVALID, ERR_UNSUPPORTED, MAX_RHS, NB, NCG, cg_problem, cg_twin, check_columns, check_products, column_tol,
                 exact_minv, is_complex, raw_cg_create, raw_cg_destroy, raw_cg_solve, rtol_of, spd_problem, true_residual)
from _ctors import ctor_build
from _gpu import dev_copy, dev_mat, outside_bytes, torch_cuda, torch_dtype  # noqa: F401
from _jacobi import CODE, DTYPES, KINDS, uniform
from _lockstep import solve_in_guarded_buffers

pytestmark = pytest.mark.gpu

VARIANTS = [(np.float32, False), (np.float64, False), (np.complex64, False), (np.complex128, False), (np.complex64, True),
            (np.complex128, True)]
CASES = [(k, dt, h) for k in KINDS for dt, h in VARIANTS if not (h and k == "symmetric")]
CASE_IDS = [f"{k}-{np.dtype(dt).name}{'-herm' if h else ''}" for k, dt, h in CASES]


def conj_of(dtype, herm):
    return herm or not is_complex(dtype)


def method_of(dtype, herm):
    return "cg" if conj_of(dtype, herm) else "cocg"


@pytest.fixture(scope="module")
def twins():
    """(dtype name, herm) -> (D, B, Minv, [twin run per column]): the dense operator does not depend on its cut, so the
    reference is computed once per variant and shared"""
    out = {}

    def get(dtype, herm):
        key = (np.dtype(dtype).name, herm)
        if key not in out:
            _, sets, D, B = cg_problem("vbcrs", dtype, herm)
            Minv = exact_minv(D, sets)
            runs = [cg_twin(D, B[:, c], Minv, conj_of(dtype, herm), rtol_of(dtype), 0.0, 100, dtype) for c in range(NB)]
            out[key] = (D, B, Minv, runs)
        return out[key]
    return get


# ---- 1. against the twin -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, dtype, herm", CASES, ids=CASE_IDS)
def test_against_the_twin(torch_cuda, bsm, twins, kind, dtype, herm):
    torch = torch_cuda
    p, sets, D, B = cg_problem(kind, dtype, herm)
    _, _, _, runs = twins(dtype, herm)
    rtol = rtol_of(dtype)
    A = bsm.synthetic.build(p)
    M = bsm.block_jacobi(A, sets)
    S = bsm.Cg(A, M, nrhs=NB, method=method_of(dtype, herm))
    X, info = S.solve(dev_copy(torch, B), rtol=rtol, maxiter=100)
    check_columns(info, runs, D, X.cpu().numpy(), B, [column_tol(B[:, c], rtol) for c in range(NB)], CASE_IDS[CASES.index((kind, dtype, herm))])
    check_products(info, True)
    assert info.history.shape == (info.iterations, NB)
    for c in range(NB):
        k = int(info.column_iterations[c])
        assert info.history[k - 1, c] == info.residual[c] <= rtol * info.bnorm[c] and np.all(info.history[:k - 1, c] > rtol * info.bnorm[c])
        assert abs(info.bnorm[c] - np.linalg.norm(B[:, c].astype(np.complex128))) <= NCG * np.finfo(dtype).eps * info.bnorm[c]
    assert info.workspace != 0 and info.workspace_bytes >= 5 * NB * NCG * np.dtype(dtype).itemsize


# ---- 2. staggered columns --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["vbcrs", "symmetric"])
@pytest.mark.parametrize("dtype, counts", [(np.float32, [11, 9, 7, 4, 0]), (np.float64, [24, 18, 11, 4, 0])], ids=["float32", "float64"])
def test_staggered_columns(torch_cuda, bsm, kind, dtype, counts):
    torch = torch_cuda
    p, sets, D, B = cg_problem(kind, dtype)
    tau, step = (1e-4, 10.0) if dtype == np.float32 else (1e-10, 1000.0)
    Bs = B.copy(order="F")
    for c in range(4):
        Bs[:, c] = (B[:, c] * dtype(step ** -c)).astype(dtype)
    Bs[:, 4] = 0
    atol = tau * float(np.linalg.norm(Bs[:, 0].astype(np.float64)))
    Minv = exact_minv(D, sets)
    runs = [cg_twin(D, Bs[:, c], Minv, True, 0.0, atol, 100, dtype) for c in range(NB)]
    assert [r.iterations for r in runs] == counts
    A = bsm.synthetic.build(p)
    M = bsm.block_jacobi(A, sets)
    X, info = bsm.Cg(A, M, nrhs=NB).solve(dev_copy(torch, Bs), rtol=0.0, atol=atol, maxiter=100)
    xh = X.cpu().numpy()
    check_columns(info, runs, D, xh, Bs, [atol] * NB, f"staggered {kind} {np.dtype(dtype).name}")
    assert info.column_iterations[4] == 0 and np.all(xh[:, 4] == 0) and info.bnorm[4] == 0
    assert info.iterations == max(info.column_iterations) and info.history.shape == (info.iterations, NB)
    for c in range(4):
        k = int(info.column_iterations[c])
        assert np.all(info.history[k - 1:, c] == info.history[k - 1, c]), ("a finished column's history moves", c)
        assert info.history[k - 1, c] <= atol and (k < 2 or info.history[k - 2, c] > atol)
    check_products(info, True)


# ---- 3. freezing holds -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_freezing_holds(torch_cuda, bsm, dtype):
    """what the host enqueues beyond a column's last iteration changes nothing: a solve that may run 400 iterations and one
    that is cut at the count give the same bytes, and so do two solves on one solver"""
    torch = torch_cuda
    p, sets, D, B = cg_problem("vbcrs", dtype)
    A = bsm.synthetic.build(p)
    M = bsm.block_jacobi(A, sets)
    b = torch.from_numpy(np.ascontiguousarray(B[:, 0])).cuda()
    y1, y2 = torch.empty_like(b), torch.empty_like(b)
    for H in (A, M):
        bsm.mul(y1, H, b)
        bsm.mul(y2, H, b)
        torch.cuda.synchronize()
        assert y1.cpu().numpy().tobytes() == y2.cpu().numpy().tobytes(), "the products of this handle are not reproducible"
    S = bsm.Cg(A, M)
    x1, i1 = S.solve(b, rtol=rtol_of(dtype), maxiter=400)
    assert i1.status == 0 and x1.shape == b.shape and 1 <= i1.iterations < 100
    x2, i2 = S.solve(b, rtol=rtol_of(dtype), maxiter=int(i1.iterations))
    assert i2.status == 0 and i2.iterations == i1.iterations
    x3, i3 = S.solve(b, rtol=rtol_of(dtype), maxiter=400)
    assert x1.cpu().numpy().tobytes() == x2.cpu().numpy().tobytes() == x3.cpu().numpy().tobytes()
    assert np.array_equal(i1.history, i2.history) and np.array_equal(i1.history, i3.history)


# ---- 4. one pass over the matrix per iteration ----------------------------------------------------------------------------
def test_one_pass_per_iteration(torch_cuda, bsm):
    torch, dtype, K = torch_cuda, np.float64, 8
    p, sets, D, B = cg_problem("vbcrs", dtype)
    B8 = np.asfortranarray(np.concatenate([B, uniform(np.random.default_rng(4100), (NCG, K - NB), dtype)], axis=1))
    A = bsm.synthetic.build(p)
    M = bsm.block_jacobi(A, sets)
    Bd = dev_copy(torch, B8)
    Y = torch.empty((K, NCG), dtype=Bd.dtype, device="cuda").t()
    before = A.value_passes()
    bsm.mul(Y, A, Bd)
    assert A.value_passes() == before + 1, "a plain 8-column product does not stream the matrix once"
    S = bsm.Cg(A, M, nrhs=K)
    before = A.value_passes()
    X, first = S.solve(Bd, rtol=1e-10, maxiter=100)
    assert first.status == 0
    # the free-running solve had one more iteration enqueued when the last record arrived (the look-ahead): one more
    # product on frozen columns, which a_products does not count
    assert A.value_passes() - before == first.a_products + 1
    before = A.value_passes()
    X, info = S.solve(Bd, rtol=1e-10, maxiter=int(first.iterations))
    assert info.status == 0 and info.iterations == first.iterations
    assert A.value_passes() - before == info.a_products == info.iterations
    check_products(info, True)


# ---- 5. pairings -----------------------------------------------------------------------------------------------------------
def test_real_operators_with_complex_right_hand_sides(torch_cuda, bsm):
    torch = torch_cuda
    p, sets, D, B = cg_problem("blocksparse", np.float64)
    Bc = np.asfortranarray((B + 1j * uniform(np.random.default_rng(4200), B.shape, np.float64)).astype(np.complex128))
    A = bsm.synthetic.build(p)
    M = bsm.block_jacobi(A, sets)
    S = bsm.Cg(A, M, nrhs=NB, dtype=np.complex128)
    X, info = S.solve(dev_copy(torch, Bc), rtol=1e-10, maxiter=100)
    assert X.dtype == torch.complex128
    Dc, Minv = D.astype(np.complex128), exact_minv(D, sets).astype(np.complex128)
    runs = [cg_twin(Dc, Bc[:, c], Minv, True, 1e-10, 0.0, 100, np.complex128) for c in range(NB)]
    check_columns(info, runs, Dc, X.cpu().numpy(), Bc, [column_tol(Bc[:, c], 1e-10) for c in range(NB)], "real A and M, complex B")
    check_products(info, True)
    with pytest.raises(TypeError):
        S.solve(dev_copy(torch, B))  # float64 columns into a complex128 solver


def test_single_precision_storage_under_double_vectors(torch_cuda, bsm):
    torch = torch_cuda
    p, sets, D, B = cg_problem("symmetric", np.float64)
    D32 = D.astype(np.float32).astype(np.float64)  # the operator IS the rounded one
    A = bsm.synthetic.build(p, storage=np.float32)
    M = bsm.block_jacobi(A, sets)
    X, info = bsm.Cg(A, M, nrhs=NB).solve(dev_copy(torch, B), rtol=1e-10, maxiter=100)
    assert X.dtype == torch.float64
    Minv = exact_minv(D32, sets)
    runs = [cg_twin(D32, B[:, c], Minv, True, 1e-10, 0.0, 100, np.float64) for c in range(NB)]
    check_columns(info, runs, D32, X.cpu().numpy(), B, [column_tol(B[:, c], 1e-10) for c in range(NB)], "float32 storage")


def test_transpose_of_the_symmetric_kind(torch_cuda, bsm, twins):
    torch, dtype = torch_cuda, np.complex128
    p, sets, D, B = cg_problem("symmetric", dtype)
    _, _, _, runs = twins(dtype, False)
    A = bsm.transpose(bsm.synthetic.build(p))
    M = bsm.block_jacobi(A, sets)
    X, info = bsm.cocg(A, dev_copy(torch, B), M=M, rtol=1e-10, maxiter=100)
    check_columns(info, runs, D.T, X.cpu().numpy(), B, [column_tol(B[:, c], 1e-10) for c in range(NB)], "transpose(symmetric)")
    check_products(info, True)


@pytest.mark.parametrize("dtype", DTYPES, ids=[np.dtype(d).name for d in DTYPES])
def test_initial_guess_close_to_the_solution(torch_cuda, bsm, dtype):
    torch = torch_cuda
    p, sets, D, B = cg_problem("blocksparse", dtype)
    rtol = rtol_of(dtype)
    wide = np.complex128 if is_complex(dtype) else np.float64
    sol = np.linalg.solve(D.astype(wide), B.astype(wide))
    noise = uniform(np.random.default_rng(4300), B.shape, dtype)
    X0 = np.asfortranarray((sol + 1e-2 * np.max(np.abs(sol)) * noise).astype(dtype))
    Minv = exact_minv(D, sets)
    runs = [cg_twin(D, B[:, c], Minv, not is_complex(dtype), rtol, 0.0, 100, dtype, x0=X0[:, c]) for c in range(NB)]
    A = bsm.synthetic.build(p)
    M = bsm.block_jacobi(A, sets)
    S = bsm.Cg(A, M, nrhs=NB, method=method_of(dtype, False))
    X, info = S.solve(dev_copy(torch, B), X0=dev_copy(torch, X0), rtol=rtol, maxiter=100)
    check_columns(info, runs, D, X.cpu().numpy(), B, [column_tol(B[:, c], rtol) for c in range(NB)], f"x0 {np.dtype(dtype).name}")
    check_products(info, True, use_x0=True)


def test_host_matrices_and_a_side_stream(torch_cuda, bsm, twins):
    torch, dtype = torch_cuda, np.float64
    p, sets, D, B = cg_problem("vbcrs", dtype)
    _, _, _, runs = twins(dtype, False)
    tols = [column_tol(B[:, c], 1e-10) for c in range(NB)]
    A = bsm.synthetic.build(p)
    M = bsm.block_jacobi(A, sets)
    S = bsm.Cg(A, M, nrhs=NB)
    Xh = np.full(B.shape, np.nan, dtype=dtype, order="F")
    got, info = S.solve(B, X=Xh, rtol=1e-10, maxiter=100)  # numpy: staged
    assert got is Xh
    check_columns(info, runs, D, Xh, B, tols, "numpy B")
    xv, iv = S.solve(np.ascontiguousarray(B[:, 1]), rtol=1e-10, maxiter=100)  # a host vector in, a vector out
    assert xv.shape == (NCG,) and iv.column_status.tolist() == [0] and true_residual(D, xv, B[:, 1]) <= 2 * tols[1]
    Bd = dev_copy(torch, B)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    Xs, info = S.solve(Bd, rtol=1e-10, maxiter=100, stream=side)
    check_columns(info, runs, D, Xs.cpu().numpy(), B, tols, "side stream")
    with pytest.raises(ValueError):
        S.solve(Bd, X=np.zeros(B.shape, dtype, order="F"))  # B on the device, X on the host
    with pytest.raises(ValueError):
        bsm.Cg(A, M, nrhs=2).solve(Bd)  # more columns than the solver holds


# ---- 6. layout edges of the kernels ----------------------------------------------------------------------------------------
EDGE_N = [1, 2, 63, 64, 65, 255, 256, 257, 1000]
EDGE_K = [1, 2, 3, 8, 16]
EDGE = [(np.float64, n, k) for n in EDGE_N for k in EDGE_K]
for _dt in (np.float32, np.complex64, np.complex128):  # both diagonals of the n x K table
    for _i, _n in enumerate(EDGE_N):
        _j = _i * len(EDGE_K) // len(EDGE_N)
        EDGE += sorted({(_dt, _n, EDGE_K[_j]), (_dt, _n, EDGE_K[len(EDGE_K) - 1 - _j])}, key=lambda t: t[2])


@pytest.mark.parametrize("dtype, n, k", EDGE, ids=[f"{np.dtype(d).name}-n{n}-k{k}" for d, n, k in EDGE])
def test_layout_edges(torch_cuda, bsm, dtype, n, k):
    """small SPD / HPD operators (diagonal blocks T^H T + I of order <= 8), no preconditioner, every column against the
    twin; the solver holds 16 columns whatever k is (nrhs < nrhs_max)"""
    torch = torch_cuda
    rng = np.random.default_rng(5000 + 17 * n + k)
    p, Dop = spd_problem(rng, n, dtype)
    B = np.asfortranarray(uniform(rng, (n, k), dtype))
    rtol = rtol_of(dtype)
    runs = [cg_twin(Dop, B[:, c], None, True, rtol, 0.0, 200, dtype) for c in range(k)]
    A = bsm.synthetic.build(p)
    S = bsm.Cg(A, nrhs=MAX_RHS)
    xh, info = solve_in_guarded_buffers(torch, bsm, S, B, MAX_RHS)
    Dw = Dop.astype(np.complex128)
    for c, run in enumerate(runs):
        assert run.status == 0 and info.column_status[c] == 0, (c, info.column_status[c])
        assert abs(int(info.column_iterations[c]) - run.iterations) <= 1, (c, info.column_iterations[c], run.iterations)
        true = float(np.linalg.norm(B[:, c].astype(np.complex128) - Dw @ xh[:, c].astype(np.complex128)))
        assert true <= 2 * column_tol(B[:, c], rtol), (c, true)
    check_products(info, False)


def test_a_workgroup_walks_several_tiles(torch_cuda, bsm):
    """n = 300 000 float64: 150 000 sixteen-byte groups on the 256 workgroups the grid is capped at, 586 each, two tiles"""
    torch, dtype, n = torch_cuda, np.float64, 300000
    rng = np.random.default_rng(5100)
    p, Dop = spd_problem(rng, n, dtype)
    b = uniform(rng, (n,), dtype)
    run = cg_twin(Dop, b, None, True, 1e-10, 0.0, 200, dtype)
    A = bsm.synthetic.build(p)
    x, info = bsm.cg(A, torch.from_numpy(b).cuda(), rtol=1e-10, maxiter=200)
    assert run.status == 0 and info.column_status[0] == 0 and abs(int(info.iterations) - run.iterations) <= 1
    assert float(np.linalg.norm(b - Dop @ x.cpu().numpy())) <= 2 * column_tol(b, 1e-10)


# ---- 7. statuses -------------------------------------------------------------------------------------------------------------
def test_maxiter_gives_status_1_and_the_twins_iterate(torch_cuda, bsm):
    """float64, column 0, no preconditioner, three iterations: x is the twin's third iterate to 8 eps max|x| -- the bound
    test_cg_cpu.py shows to cover another summation order of every product and form"""
    torch, dtype = torch_cuda, np.float64
    p, _, D, B = cg_problem("vbcrs", dtype)
    run = cg_twin(D, B[:, 0], None, True, 1e-10, 0.0, 3, dtype)
    A = bsm.synthetic.build(p)
    x, info = bsm.cg(A, torch.from_numpy(np.ascontiguousarray(B[:, 0])).cuda(), rtol=1e-10, maxiter=3)
    assert run.status == 1 and info.status == 1 and not info.converged and info.column_status.tolist() == [1]
    assert info.iterations == 3 and info.column_iterations.tolist() == [3] and info.history.shape == (3, 1)
    assert info.columns_converged == 0 and (info.a_products, info.m_products) == (3, 0)
    dev = np.max(np.abs(x.cpu().numpy() - run.iterates[2])) / (np.finfo(dtype).eps * np.max(np.abs(run.iterates[2])))
    print(f"CGSTAT third iterate against the twin's: {dev:.2f} eps max|x|")
    assert dev <= 8
    assert np.allclose(info.history[:, 0], run.history, rtol=1e-10)
    x0, i0 = bsm.cg(A, torch.from_numpy(np.ascontiguousarray(B[:, 0])).cuda(), maxiter=0)
    assert (i0.status, i0.iterations) == (1, 0) and torch.count_nonzero(x0).item() == 0 and len(i0.history) == 0


@pytest.mark.parametrize("dtype", [np.float64, np.complex64], ids=["float64", "complex64"])
def test_breakdown_freezes_its_column_only(torch_cuda, bsm, dtype):
    """[[0, 1], [1, 0]] with b = e1: <p, A p> = 0 in iteration 1 -- status 3, no iteration, x = 0, no NaN -- while the
    column b = (1, 1) of the same solve converges in one iteration (A b = b)"""
    torch = torch_cuda
    A = bsm.BlockSparseMatrix([np.asfortranarray(np.array([[0, 1], [1, 0]], dtype=dtype))], [[1, 2]], [[1, 2]], (2, 2))
    B = np.asfortranarray(np.array([[1, 1], [0, 1]], dtype=dtype))
    for method in ("cg", "cocg"):
        X, info = bsm.Cg(A, nrhs=2, method=method).solve(dev_copy(torch, B), rtol=1e-6, maxiter=10)
        xh = X.cpu().numpy()
        assert info.column_status.tolist() == [3, 0] and info.status == 3 and info.columns_converged == 1
        assert info.column_iterations.tolist() == [0, 1] and info.iterations == 1
        assert np.all(xh[:, 0] == 0) and np.all(xh[:, 1] == 1) and info.residual[0] == 1 and info.residual[1] == 0
        assert np.all(np.isfinite(info.history)) and info.history[:, 0].tolist() == [1.0]


def test_nan_in_one_column_gives_status_2_for_it_only(torch_cuda, bsm, twins):
    torch, dtype = torch_cuda, np.float32
    p, sets, D, B = cg_problem("blocksparse", dtype)
    _, _, _, runs = twins(dtype, False)
    Bn = B.copy(order="F")
    Bn[17, 2] = np.nan
    A = bsm.synthetic.build(p)
    M = bsm.block_jacobi(A, sets)
    S = bsm.Cg(A, M, nrhs=NB)
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


# ---- 8. refusals, through raw ctypes ------------------------------------------------------------------------------------------
def test_refusals(torch_cuda, bsm):
    torch, dtype = torch_cuda, np.float64
    f64 = CODE[np.dtype(dtype)]
    p, sets, D, B = cg_problem("blocksparse", dtype)
    A = bsm.synthetic.build(p)
    M = bsm.block_jacobi(A, sets)
    A2 = ctor_build(bsm, "blocksparse", p, devices=[0, 0])
    assert raw_cg_create(A2, 0, None, 0, f64, 4)[0] == ERR_UNSUPPORTED
    assert raw_cg_create(A, 0, A2, 0, f64, 4)[0] == ERR_UNSUPPORTED
    small = bsm.BlockSparseMatrix([np.eye(3)], [[1, 2, 3]], [[1, 2, 3]], (3, 3))
    assert raw_cg_create(A, 0, small, 0, f64, 4)[0] == ERR_INVALID
    pc, _, _, _ = cg_problem("vbcrs", np.complex128)
    Ac = bsm.synthetic.build(pc)
    assert raw_cg_create(Ac, 0, None, 0, f64, 4)[0] == ERR_INVALID
    assert raw_cg_create(A, 0, Ac, 0, f64, 4)[0] == ERR_INVALID
    with pytest.raises(bsm._lib.BsmError, match="multi-device"):
        bsm.Cg(A2)
    rc, ptr = raw_cg_create(A, 0, M, 0, f64, MAX_RHS)
    assert rc == 0 and ptr.value
    try:
        Bd = dev_copy(torch, np.asfortranarray(np.concatenate([B] * 4, axis=1)))  # 20 columns
        Xs = torch.zeros((20, NCG), dtype=Bd.dtype, device="cuda")
        Xd = Xs.t()
        st = torch.cuda.current_stream().cuda_stream
        b, x, es = Bd.data_ptr(), Xd.data_ptr(), 8
        ok = raw_cg_solve(ptr, NB, b, NCG, x, NCG, rtol=1e-10, stream=st)
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
            assert raw_cg_solve(ptr, *args, stream=st, **kw)[0] == ERR_INVALID, what
        # X just behind the columns of B that are read is no overlap
        assert raw_cg_solve(ptr, NB, b, NCG, b + NB * NCG * es, NCG, rtol=1e-10, stream=st)[0] == 0
        # a capturing stream: refused before anything is enqueued, the capture stays valid
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            Xs.zero_()
            rc = raw_cg_solve(ptr, NB, b, NCG, x, NCG, stream=torch.cuda.current_stream().cuda_stream)[0]
        assert rc == ERR_INVALID
        torch.cuda.synchronize()
        # and without columns / history
        from bsm_amd import _lib as L
        import ctypes as C
        prm = L.BsmCgParams(C.sizeof(L.BsmCgParams), 0, 1e-10, 0.0, 100, 0)
        info = L.BsmCgInfo()
        assert L.lib().bsm_cg_solve(ptr, NB, b, NCG, x, NCG, C.byref(prm), C.byref(info), None, None, 1, st) == 0
        assert info.status == 0 and info.columns_converged == NB and info.iterations == ok[1].iterations
    finally:
        assert raw_cg_destroy(ptr) == 0
