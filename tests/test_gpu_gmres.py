"""GPU suite of bsm_gmres_solve / Gmres: right-preconditioned restarted GMRES on the 12 operators of tests/_krylov.py
against the numpy twin (same method, none of the code), the honest report of stagnation, the edge cases of the call, and
the operator / vector-type combinations a solver accepts.  The twin itself is tested in test_krylov_cpu.py."""
import numpy as np
import pytest

from _ctors import ctor_build
from _gpu import TOL, torch_cuda  # noqa: F401
from _jacobi import CODE, DTYPES, KINDS, NOP, dense_of, set_blocks
from _krylov import (ERR_INVALID, ERR_UNSUPPORTED, RESTART, Truth, check_against_twin, check_history, exact_minv, expected_products,
                     gmres_twin, krylov_problem, raw_gmres_create, raw_gmres_destroy, raw_gmres_solve, rtol_of, true_residual)

pytestmark = pytest.mark.gpu
IDS = [np.dtype(d).name for d in DTYPES]


def dev(torch, v):
    return torch.from_numpy(np.ascontiguousarray(v)).cuda()


def reproducible(*ops):
    """the products of these handles are bitwise reproducible: exclusive forward images (no atomics)"""
    return all(o.stats()["exclusive"] == 1 for o in ops)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_solves_with_block_jacobi(torch_cuda, bsm, kind, dtype):
    torch = torch_cuda
    p, sets, b = krylov_problem(kind, dtype)
    D, rtol = Truth(p).D, rtol_of(dtype)
    A = bsm.synthetic.build(p)
    M = bsm.block_jacobi(A, sets)
    S = bsm.Gmres(A, M, restart=RESTART)
    bd = dev(torch, b)
    x, info = S.solve(bd, rtol=rtol, maxiter=100)
    assert info.status == 0 and info.converged
    bnorm = float(np.linalg.norm(b.astype(np.complex128)))
    assert abs(info.bnorm - bnorm) <= NOP * np.finfo(dtype).eps * bnorm
    xh = x.cpu().numpy()
    true = true_residual(D, xh, b)
    print(f"KRYSTAT gmres {kind} {np.dtype(dtype).name}: true residual / (rtol |b|) = {true / (rtol * bnorm):.3f}")
    assert true <= 2 * rtol * bnorm
    check_history(info, rtol * info.bnorm, RESTART, dtype)
    twin = gmres_twin(D, b, exact_minv(D, sets), RESTART, rtol, 100, dtype)
    check_against_twin(info, twin, f"{kind} {np.dtype(dtype).name}")
    assert (info.a_products, info.m_products) == expected_products(info.iterations, info.cycles, False, True)
    # the same solve again
    x2, info2 = S.solve(bd, rtol=rtol, maxiter=100)
    assert info2.iterations == info.iterations and info2.cycles == info.cycles
    if reproducible(A, M):
        assert x2.cpu().numpy().tobytes() == xh.tobytes() and np.array_equal(info2.history, info.history)
    else:
        assert np.max(np.abs(x2.cpu().numpy() - xh)) <= TOL[np.dtype(dtype)] * np.max(np.abs(xh))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", [np.float32, np.complex128], ids=["float32", "complex128"])
def test_stagnation_is_reported_honestly(torch_cuda, bsm, kind, dtype):
    torch = torch_cuda
    p, _, b = krylov_problem(kind, dtype)
    D = Truth(p).D
    A = bsm.synthetic.build(p)
    x, info = bsm.gmres(A, dev(torch, b), restart=RESTART, rtol=rtol_of(dtype), maxiter=50)
    assert info.status == 1 and not info.converged and info.iterations == 50 and info.cycles == 3
    assert (info.a_products, info.m_products) == (52, 0)
    check_history(info, 0.0, RESTART, dtype)
    true = true_residual(D, x.cpu().numpy(), b)
    ratio = info.residual / true
    print(f"KRYSTAT stagnation {kind} {np.dtype(dtype).name}: estimate / true - 1 = {ratio - 1:.3e}, estimate / |b| = {info.residual / info.bnorm:.4f}")
    assert abs(ratio - 1) <= 1e3 * np.finfo(dtype).eps
    assert info.residual >= 0.9 * info.bnorm  # what the twin shows on these operators (test_krylov_cpu.py)


# ---- edge cases ------------------------------------------------------------------------------------------------------------
EDGE = [np.float64, np.complex64]
EDGE_IDS = ["float64", "complex64"]


@pytest.fixture(scope="module")
def edge(torch_cuda, bsm):
    """per type: the blocksparse problem, its handles, one Gmres(20) and its reference solve, made once"""
    out = {}
    for dtype in EDGE:
        p, sets, b = krylov_problem("blocksparse", dtype)
        A = bsm.synthetic.build(p)
        M = bsm.block_jacobi(A, sets)
        S = bsm.Gmres(A, M, restart=RESTART)
        x, info = S.solve(dev(torch_cuda, b), rtol=rtol_of(dtype), maxiter=100)
        out[np.dtype(dtype).name] = dict(p=p, sets=sets, b=b, D=Truth(p).D, A=A, M=M, S=S, x=x.cpu().numpy(), info=info,
                                         rtol=rtol_of(dtype), same=reproducible(A, M))
    return out


def same_solution(e, got, dtype):
    if e["same"]:
        assert got.tobytes() == e["x"].tobytes()
    else:
        assert np.max(np.abs(got - e["x"])) <= TOL[np.dtype(dtype)] * np.max(np.abs(e["x"]))


@pytest.mark.parametrize("dtype", EDGE, ids=EDGE_IDS)
def test_lucky_breakdown(torch_cuda, bsm, dtype):
    """A = I as identity blocks, b of +-1 entries with n = 256: ||b|| = 16, v_0 = b / 16, h = 1, w' = 0 and ||w'|| = 0 are
    all exact in binary floating point, so the breakdown is exact and x = 16 v_0 = b bit for bit"""
    torch = torch_cuda
    n, bs = 256, 32
    blocks = [np.asfortranarray(np.eye(bs, dtype=dtype)) for _ in range(n // bs)]
    idx = [np.arange(i * bs + 1, (i + 1) * bs + 1, dtype=np.int64) for i in range(n // bs)]
    A = bsm.BlockSparseMatrix(blocks, idx, idx, (n, n))
    b = np.where(np.random.default_rng(6000).uniform(-1, 1, n) < 0, -1, 1).astype(dtype)
    x, info = bsm.gmres(A, dev(torch, b), restart=5)
    xh = x.cpu().numpy()
    assert info.status == 0 and info.iterations == 1 and info.cycles == 1
    assert np.all(np.isfinite(xh.view(xh.real.dtype))) and np.all(xh == b) and info.residual == 0 and info.bnorm == 16


@pytest.mark.parametrize("dtype", EDGE, ids=EDGE_IDS)
def test_zero_right_hand_side_and_nan_in_x(torch_cuda, edge, dtype):
    torch, e = torch_cuda, edge[np.dtype(dtype).name]
    x = torch.full((NOP,), float("nan"), dtype=dev(torch, e["b"]).dtype, device="cuda")
    _, info = e["S"].solve(torch.zeros_like(x), x=x, rtol=e["rtol"])
    assert (info.status, info.iterations, info.cycles, info.a_products, info.m_products) == (0, 0, 0, 0, 0)
    assert torch.count_nonzero(x).item() == 0 and info.bnorm == 0 and len(info.history) == 0
    # use_x0 = 0: NaN in the incoming x does not survive, the solve is the reference solve
    x.fill_(float("nan"))
    _, info = e["S"].solve(dev(torch, e["b"]), x=x, rtol=e["rtol"], maxiter=100)
    assert info.status == 0 and info.iterations == e["info"].iterations
    same_solution(e, x.cpu().numpy(), dtype)


@pytest.mark.parametrize("dtype", EDGE, ids=EDGE_IDS)
def test_initial_guess(torch_cuda, edge, dtype):
    """x0 = the reference solution (true residual <= 2 rtol |b|, asserted above) under 10 rtol: 0 iterations, one product
    for the residual, x untouched; x0 = that solution under the same rtol from a perturbed start: converges, fewer iterations"""
    torch, e = torch_cuda, edge[np.dtype(dtype).name]
    bd = dev(torch, e["b"])
    x, info = e["S"].solve(bd, x0=dev(torch, e["x"]), rtol=10 * e["rtol"])
    assert (info.status, info.iterations, info.cycles, info.a_products, info.m_products) == (0, 0, 0, 1, 0)
    assert x.cpu().numpy().tobytes() == e["x"].tobytes()
    assert info.residual <= 10 * e["rtol"] * info.bnorm
    x0 = (e["x"] * dtype(1.001)).astype(dtype)
    x, info = e["S"].solve(bd, x0=x0, rtol=e["rtol"], maxiter=100)
    assert info.status == 0 and 1 <= info.iterations <= e["info"].iterations
    assert (info.a_products, info.m_products) == expected_products(info.iterations, info.cycles, True, True)
    assert true_residual(e["D"], x.cpu().numpy(), e["b"]) <= 2 * e["rtol"] * info.bnorm


@pytest.mark.parametrize("dtype", EDGE, ids=EDGE_IDS)
def test_nan_in_b_gives_status_2_and_returns(torch_cuda, edge, dtype):
    torch, e = torch_cuda, edge[np.dtype(dtype).name]
    b = e["b"].copy()
    b[17] = np.nan
    x, info = e["S"].solve(dev(torch, b), rtol=e["rtol"], maxiter=100)
    assert info.status == 2 and info.iterations == 0 and not np.isfinite(info.bnorm)
    # and the solver is usable afterwards
    x, info = e["S"].solve(dev(torch, e["b"]), rtol=e["rtol"], maxiter=100)
    assert info.status == 0
    same_solution(e, x.cpu().numpy(), dtype)


@pytest.mark.parametrize("dtype", EDGE, ids=EDGE_IDS)
def test_restart_values(torch_cuda, bsm, edge, dtype):
    """restart = 1 (every iteration is a cycle) and a restart larger than the iterations needed (one cycle), both against
    the twin with the same restart"""
    torch, e = torch_cuda, edge[np.dtype(dtype).name]
    Minv = exact_minv(e["D"], e["sets"])
    for restart in (1, 64):
        x, info = bsm.Gmres(e["A"], e["M"], restart=restart).solve(dev(torch, e["b"]), rtol=e["rtol"], maxiter=100)
        assert info.status == 0
        check_history(info, e["rtol"] * info.bnorm, restart, dtype)
        assert info.cycles == (info.iterations if restart == 1 else 1)
        assert (info.a_products, info.m_products) == expected_products(info.iterations, info.cycles, False, True)
        assert true_residual(e["D"], x.cpu().numpy(), e["b"]) <= 2 * e["rtol"] * info.bnorm
        check_against_twin(info, gmres_twin(e["D"], e["b"], Minv, restart, e["rtol"], 100, dtype), f"restart {restart} {np.dtype(dtype).name}")


@pytest.mark.parametrize("dtype", EDGE, ids=EDGE_IDS)
def test_atol_dominating(torch_cuda, edge, dtype):
    torch, e = torch_cuda, edge[np.dtype(dtype).name]
    atol = 1e-2 * float(np.linalg.norm(e["b"]))
    x, info = e["S"].solve(dev(torch, e["b"]), rtol=e["rtol"] * 1e-3, atol=atol, maxiter=100)
    assert info.status == 0 and 1 <= info.iterations < e["info"].iterations
    check_history(info, atol, RESTART, dtype)
    assert true_residual(e["D"], x.cpu().numpy(), e["b"]) <= 2 * atol
    twin = gmres_twin(e["D"], e["b"], exact_minv(e["D"], e["sets"]), RESTART, 0.0, 100, dtype, atol=atol)
    check_against_twin(info, twin, f"atol {np.dtype(dtype).name}")


@pytest.mark.parametrize("dtype", EDGE, ids=EDGE_IDS)
def test_maxiter_in_the_middle_of_a_cycle(torch_cuda, bsm, edge, dtype):
    """no preconditioner (stagnation), restart 20, maxiter 27: one full cycle and seven iterations of the second, whose
    update is applied -- the estimate is the true residual of the returned x"""
    torch, e = torch_cuda, edge[np.dtype(dtype).name]
    x, info = bsm.gmres(e["A"], dev(torch, e["b"]), restart=RESTART, rtol=e["rtol"], maxiter=27)
    assert (info.status, info.iterations, info.cycles, info.a_products, info.m_products) == (1, 27, 2, 28, 0)
    check_history(info, 0.0, RESTART, dtype)
    true = true_residual(e["D"], x.cpu().numpy(), e["b"])
    assert abs(info.residual / true - 1) <= 1e3 * np.finfo(dtype).eps
    x, info = bsm.gmres(e["A"], dev(torch, e["b"]), restart=RESTART, maxiter=0)
    assert (info.status, info.iterations, info.cycles) == (1, 0, 0) and torch.count_nonzero(x).item() == 0


@pytest.mark.parametrize("dtype", EDGE, ids=EDGE_IDS)
def test_history_capacity_and_raw_argument_checks(torch_cuda, edge, dtype):
    torch, e = torch_cuda, edge[np.dtype(dtype).name]
    ptr, its = e["S"]._ptr, e["info"].iterations
    bd = dev(torch, e["b"])
    xd = torch.empty_like(bd)
    st = torch.cuda.current_stream().cuda_stream
    assert its >= 3
    rc, info, hist = raw_gmres_solve(ptr, bd.data_ptr(), xd.data_ptr(), rtol=e["rtol"], capacity=its - 2, hist_len=its + 2, stream=st)
    assert rc == 0 and info.status == 0 and info.iterations == its
    assert np.array_equal(hist[:its - 2], e["info"].history[:its - 2]) if e["same"] else np.all(hist[:its - 2] > 0)
    assert np.all(hist[its - 2:] == -1), "history was written beyond history_capacity"
    same_solution(e, xd.cpu().numpy(), dtype)
    rc, info, _ = raw_gmres_solve(ptr, bd.data_ptr(), xd.data_ptr(), rtol=e["rtol"], capacity=0, stream=st)  # no history at all
    assert rc == 0 and info.iterations == its
    # refusals: x aliasing b (the same vector, and an overlap), null vectors, bad tolerances, memspace, struct size
    es = e["b"].itemsize
    for what, args, kw in [("x is b", (bd.data_ptr(), bd.data_ptr()), {}), ("x overlaps b", (bd.data_ptr(), bd.data_ptr() + 8 * es), {}),
                           ("null b", (None, xd.data_ptr()), {}), ("null x", (bd.data_ptr(), None), {}),
                           ("negative rtol", (bd.data_ptr(), xd.data_ptr()), dict(rtol=-1.0)),
                           ("NaN atol", (bd.data_ptr(), xd.data_ptr()), dict(atol=float("nan"))),
                           ("negative maxiter", (bd.data_ptr(), xd.data_ptr()), dict(maxiter=-1, capacity=0)),
                           ("negative capacity", (bd.data_ptr(), xd.data_ptr()), dict(capacity=-1)),
                           ("bad memspace", (bd.data_ptr(), xd.data_ptr()), dict(memspace=2)),
                           ("struct size", (bd.data_ptr(), xd.data_ptr()), dict(struct_size=8))]:
        assert raw_gmres_solve(ptr, *args, stream=st, **kw)[0] == ERR_INVALID, what
    assert raw_gmres_solve(None, bd.data_ptr(), xd.data_ptr())[0] == ERR_INVALID


@pytest.mark.parametrize("dtype", EDGE, ids=EDGE_IDS)
def test_host_vectors_and_a_side_stream(torch_cuda, edge, dtype):
    torch, e = torch_cuda, edge[np.dtype(dtype).name]
    x = np.full(NOP, np.nan, dtype)
    got, info = e["S"].solve(e["b"], x=x, rtol=e["rtol"], maxiter=100)
    assert got is x and info.status == 0 and info.iterations == e["info"].iterations
    same_solution(e, x, dtype)
    x1, info = e["S"].solve(e["b"], x0=e["x"], rtol=10 * e["rtol"])  # host vectors with an initial guess
    assert info.iterations == 0 and x1.tobytes() == e["x"].tobytes()
    bd = dev(torch, e["b"])
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    xs, info = e["S"].solve(bd, rtol=e["rtol"], maxiter=100, stream=side)
    assert info.status == 0 and info.iterations == e["info"].iterations
    same_solution(e, xs.cpu().numpy(), dtype)
    with pytest.raises(ValueError):
        e["S"].solve(bd, x=np.zeros(NOP, dtype))  # b on the device, x on the host
    with pytest.raises(ValueError):
        e["S"].solve(bd[:10])
    with pytest.raises(TypeError):
        e["S"].solve(torch.zeros(NOP, dtype=torch.complex128 if dtype == np.float64 else torch.float64, device="cuda"))


@pytest.mark.parametrize("use_x0", [False, True], ids=["from-zero", "x0"])
@pytest.mark.parametrize("dtype", EDGE, ids=EDGE_IDS)
def test_vectors_one_element_off_alignment(torch_cuda, edge, dtype, use_x0):
    """b and x as views that start ONE element into NaN-filled device buffers (no 16-byte alignment; torch allocations are
    aligned far beyond that) with 5 guard elements behind them: the solve is the aligned solve -- status, iterations, x --
    and not a byte of the guards changes.  b and x reach the workspace element by element (the start, the copy of x0) and
    x leaves it the same way (the copy-out)."""
    torch, e = torch_cuda, edge[np.dtype(dtype).name]
    bd = dev(torch, e["b"])
    assert bd.data_ptr() % 16 == 0
    x0 = dev(torch, (e["x"] * dtype(1.001)).astype(dtype)) if use_x0 else None
    if use_x0:
        xr, ref = e["S"].solve(bd, x0=x0, rtol=e["rtol"], maxiter=100)
        xr = xr.cpu().numpy()
    else:
        xr, ref = e["x"], e["info"]
    es = bd.element_size()
    bbuf = torch.full((NOP + 6,), float("nan"), dtype=bd.dtype, device="cuda")
    xbuf = torch.full((NOP + 6,), float("nan"), dtype=bd.dtype, device="cuda")
    bv, xv = bbuf[1:NOP + 1], xbuf[1:NOP + 1]
    assert bv.data_ptr() % 16 == es % 16 and xv.data_ptr() % 16 == es % 16
    bv.copy_(bd)
    before = [t.cpu().numpy().tobytes() for t in (bbuf[:1], bbuf[NOP + 1:], xbuf[:1], xbuf[NOP + 1:])]
    got, info = e["S"].solve(bv, x=xv, x0=x0, rtol=e["rtol"], maxiter=100)
    assert got is xv
    after = [t.cpu().numpy().tobytes() for t in (bbuf[:1], bbuf[NOP + 1:], xbuf[:1], xbuf[NOP + 1:])]
    assert after == before, "a guard element around b or x was written"
    assert len(before[1]) == 5 * es and bv.cpu().numpy().tobytes() == e["b"].tobytes()
    assert (info.status, info.iterations) == (ref.status, ref.iterations) and info.status == 0
    got = xv.cpu().numpy()
    if e["same"]:
        assert got.tobytes() == xr.tobytes()
    else:
        assert np.max(np.abs(got - xr)) <= TOL[np.dtype(dtype)] * np.max(np.abs(xr))


# ---- operator and vector-type combinations ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("op", ["T", "C"])
def test_transposed_and_adjoint_operators(torch_cuda, bsm, kind, op):
    torch, dtype = torch_cuda, np.complex128
    p, sets, b = krylov_problem(kind, dtype)
    wrap = bsm.transpose if op == "T" else bsm.adjoint
    Dop = Truth(p).D.T.copy() if op == "T" else Truth(p).D.conj().T.copy()
    A = bsm.synthetic.build(p)
    M = bsm.block_jacobi(wrap(A), sets)
    x, info = bsm.Gmres(wrap(A), M, restart=RESTART).solve(dev(torch, b), rtol=1e-10, maxiter=100)
    assert info.status == 0
    assert true_residual(Dop, x.cpu().numpy(), b) <= 2e-10 * info.bnorm
    check_history(info, 1e-10 * info.bnorm, RESTART, dtype)
    check_against_twin(info, gmres_twin(Dop, b, exact_minv(Dop, sets), RESTART, 1e-10, 100, dtype), f"op {op} {kind}")
    # the same system through the wrappers of M: inv(A[I, I])^T = inv(A^T[I, I])
    M2 = wrap(bsm.block_jacobi(A, sets))
    x2, info2 = bsm.Gmres(wrap(A), M2, restart=RESTART).solve(dev(torch, b), rtol=1e-10, maxiter=100)
    assert info2.status == 0 and abs(info2.iterations - info.iterations) <= 2
    assert true_residual(Dop, x2.cpu().numpy(), b) <= 2e-10 * info2.bnorm


@pytest.mark.parametrize("kind", KINDS)
def test_a_real_preconditioner_under_a_complex_operator(torch_cuda, bsm, kind):
    """M = the inverses of the REAL PARTS of the diagonal blocks, a float64 handle driven through bsm_mul_cvec: it must
    only converge; the twin with the same real M decides the count"""
    torch = torch_cuda
    p, sets, b = krylov_problem(kind, np.complex128)
    D = Truth(p).D
    blocks = [np.asfortranarray(np.linalg.inv(blk.real)) for blk in set_blocks(D, sets)]
    A = bsm.synthetic.build(p)
    M = bsm.BlockSparseMatrix(blocks, sets, sets, (NOP, NOP))
    assert M.dtype == np.float64
    x, info = bsm.Gmres(A, M, restart=RESTART).solve(dev(torch, b), rtol=1e-10, maxiter=200)
    assert info.status == 0 and info.m_products == info.iterations + info.cycles
    assert true_residual(D, x.cpu().numpy(), b) <= 2e-10 * info.bnorm
    twin = gmres_twin(D, b, dense_of(blocks, sets, NOP).astype(np.complex128), RESTART, 1e-10, 200, np.complex128)
    check_against_twin(info, twin, f"real M, complex A, {kind}")


@pytest.mark.parametrize("kind", KINDS)
def test_real_operators_with_a_complex_right_hand_side(torch_cuda, bsm, kind):
    torch = torch_cuda
    p, sets, b = krylov_problem(kind, np.float64)
    D = Truth(p).D
    bc = (b + 1j * np.random.default_rng(6100).uniform(-1, 1, NOP)).astype(np.complex128)
    A = bsm.synthetic.build(p)
    M = bsm.block_jacobi(A, sets)
    S = bsm.Gmres(A, M, restart=RESTART, dtype=np.complex128)
    x, info = S.solve(dev(torch, bc), rtol=1e-10, maxiter=100)
    assert info.status == 0 and x.dtype == torch.complex128
    assert true_residual(D, x.cpu().numpy(), bc) <= 2e-10 * info.bnorm
    twin = gmres_twin(D.astype(np.complex128), bc, exact_minv(D, sets).astype(np.complex128), RESTART, 1e-10, 100, np.complex128)
    check_against_twin(info, twin, f"real A and M, complex b, {kind}")
    x1, _ = bsm.gmres(A, dev(torch, bc), M=M, restart=RESTART, rtol=1e-10, maxiter=100)  # the one-shot form takes b's type
    assert x1.dtype == torch.complex128
    with pytest.raises(TypeError):
        S.solve(dev(torch, b))  # a float64 vector into a complex128 solver


@pytest.mark.parametrize("kind", KINDS)
def test_single_precision_storage_under_double_vectors(torch_cuda, bsm, kind):
    """storage=float32: the operator IS the rounded one; the solve reaches 1e-10 on it"""
    torch = torch_cuda
    p, sets, b = krylov_problem(kind, np.float64)
    D = Truth(p, storage=np.float32).D.astype(np.float64)
    A = bsm.synthetic.build(p, storage=np.float32)
    M = bsm.block_jacobi(A, sets)
    x, info = bsm.Gmres(A, M, restart=RESTART).solve(dev(torch, b), rtol=1e-10, maxiter=100)
    assert info.status == 0 and x.dtype == torch.float64
    assert true_residual(D, x.cpu().numpy(), b) <= 2e-10 * info.bnorm
    check_against_twin(info, gmres_twin(D, b, exact_minv(D, sets), RESTART, 1e-10, 100, np.float64), f"float32 storage {kind}")


def test_one_solver_three_right_hand_sides(torch_cuda, edge):
    torch, e = torch_cuda, edge["float64"]
    rng = np.random.default_rng(6200)
    seen = set()
    for _ in range(3):
        b = rng.uniform(-1, 1, NOP)
        x, info = e["S"].solve(dev(torch, b), rtol=1e-10, maxiter=100)
        assert info.status == 0 and true_residual(e["D"], x.cpu().numpy(), b) <= 2e-10 * info.bnorm
        seen.add((info.workspace, info.workspace_bytes))
    assert len(seen) == 1 and e["info"].workspace != 0
    assert (e["info"].workspace, e["info"].workspace_bytes) in seen
    # with M: the basis v_0 .. v_restart, w, x and z
    assert e["info"].workspace_bytes >= (RESTART + 4) * NOP * 8


def test_create_refusals_that_need_a_device(torch_cuda, bsm, edge):
    e = edge["float64"]
    A2 = ctor_build(bsm, "blocksparse", e["p"], devices=[0, 0])
    f64 = CODE[np.dtype(np.float64)]
    assert raw_gmres_create(A2, 0, None, 0, f64, RESTART)[0] == ERR_UNSUPPORTED
    assert raw_gmres_create(e["A"], 0, A2, 0, f64, RESTART)[0] == ERR_UNSUPPORTED
    rc, ptr = raw_gmres_create(e["A"], 0, e["M"], 0, f64, RESTART)
    assert rc == 0 and ptr.value
    assert raw_gmres_destroy(ptr) == 0
    with pytest.raises(bsm._lib.BsmError, match="multi-device"):
        bsm.Gmres(A2)
