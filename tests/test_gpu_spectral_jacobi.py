"""GPU suite of block_jacobi(kind="abs" | "pinv") on the device: submatrices, eigh_blocks, spectral_blocks and the constructor
from device tensors, as the preconditioner of Minres on the indefinite order-400 problem of tests/_minres.py -- where the
explicit block inverse of the operator itself breaks down at once -- against the numpy twin with numpy's abs inverse; the
inertia in M.eigenvalues; the pseudo-inverse of a rank-deficient block; refresh across update_blocks; Lobpcg."""
import numpy as np
import pytest

from _cg import NB, column_tol
from _eigh import DTYPES, abs_minv, check_spectral_jacobi, rank_deficient, real_of
from _gpu import dev_copy, torch_cuda  # noqa: F401
from _krylov import rtol_of
from _minres import check_columns, check_products, cut_operator, minres_problem, minres_twin
from _values import src_list

pytestmark = pytest.mark.gpu

CASES = [(k, dt) for k in ("vbcrs", "blocksparse", "symmetric") for dt in DTYPES if not (k == "symmetric" and np.dtype(dt).kind == "c")]
CASE_IDS = [f"{k}-{np.dtype(dt).name}" for k, dt in CASES]
_twins = {}


def name(dtype):
    return np.dtype(dtype).name


def twins(dtype, scale=1.0):
    """(D, B, sets, [twin run per column]) of the order-400 problem (times scale) with numpy's abs block inverse of D itself;
    computed once per type"""
    key = (name(dtype), scale)
    if key not in _twins:
        _, _, sets, D, _, B = minres_problem("vbcrs", dtype)
        D = (D * np.dtype(dtype).type(scale)).astype(dtype)
        Minv, _ = abs_minv(D, sets)
        _twins[key] = (D, B, sets, [minres_twin(D, B[:, c], Minv, rtol_of(dtype), 0.0, 200, dtype) for c in range(NB)])
    return _twins[key]


@pytest.mark.parametrize("kind, dtype", CASES, ids=CASE_IDS)
def test_minres_with_the_abs_preconditioner_of_the_operator_itself(torch_cuda, bsm, kind, dtype):
    torch = torch_cuda
    D, B, sets, runs = twins(dtype)
    rtol = rtol_of(dtype)
    A = bsm.synthetic.build(minres_problem(kind, dtype)[0])
    M = bsm.block_jacobi(A, sets, kind="abs")
    assert M.kind == "abs" and M.rcond == 0.0 and M.device == A.device and all(b.is_cuda for b in M.blocks)
    X, info = bsm.Minres(A, M, nrhs=NB).solve(dev_copy(torch, B), rtol=rtol, maxiter=200)
    check_columns(info, runs, D, X.cpu().numpy(), B, [column_tol(B[:, c], rtol) for c in range(NB)], f"abs {kind}-{name(dtype)}")
    check_products(info, True)
    # the inertia, set by set: D = W (S + s J) W with J = +1 / -1 alternating by set
    assert len(M.eigenvalues) == len(sets)
    for k, w in enumerate(M.eigenvalues):
        w = w.cpu().numpy()
        assert w.dtype == real_of(dtype) and len(w) == len(sets[k]) and np.all(np.diff(w) >= 0)
        assert np.all(w > 0) if k % 2 == 0 else np.all(w < 0), k
    check_spectral_jacobi(bsm, M, D, sets, "absinv", 0.0, f"device abs {kind}-{name(dtype)}")
    # kind="inverse" on the same operator still breaks down: status 3 on every column
    Xi, broken = bsm.Minres(A, bsm.block_jacobi(A, sets, kind="inverse"), nrhs=NB).solve(dev_copy(torch, B), rtol=rtol, maxiter=200)
    assert broken.column_status.tolist() == [3] * NB and broken.status == 3


@pytest.mark.parametrize("kind, dtype", [("blocksparse", np.float32), ("vbcrs", np.complex128), ("symmetric", np.float64)],
                         ids=["blocksparse-float32", "vbcrs-complex128", "symmetric-float64"])
def test_pinv_of_a_rank_deficient_block_on_the_device(torch_cuda, bsm, kind, dtype):
    p, sets, D, k = rank_deficient(kind, dtype)
    A = bsm.synthetic.build(p)
    M = bsm.block_jacobi(A, sets, kind="pinv")
    rcond = float(np.sqrt(np.finfo(real_of(dtype)).eps))
    assert M.kind == "pinv" and M.rcond == rcond and M.device == A.device
    check_spectral_jacobi(bsm, M, D, sets, "pinv", rcond, f"device pinv {kind}-{name(dtype)}")
    with pytest.raises(np.linalg.LinAlgError, match=rf"set {k + 1} "):
        bsm.block_jacobi(A, sets, kind="abs")


@pytest.mark.parametrize("dtype", [np.float64, np.complex64], ids=["float64", "complex64"])
def test_refresh_after_update_blocks_on_one_solver(torch_cuda, bsm, dtype):
    torch = torch_cuda
    kind, rtol = "blocksparse", rtol_of(dtype)
    D, B, sets, runs = twins(dtype)
    A = bsm.synthetic.build(cut_operator(kind, D, sets))  # (a cut of its own: minres_problem's arrays are shared and not written to)
    M = bsm.block_jacobi(A, sets, kind="abs")
    S = bsm.Minres(A, M, nrhs=NB)
    X, info = S.solve(dev_copy(torch, B), rtol=rtol, maxiter=200)
    check_columns(info, runs, D, X.cpu().numpy(), B, [column_tol(B[:, c], rtol) for c in range(NB)], f"before the update {name(dtype)}")
    D2, _, _, runs2 = twins(dtype, -0.5)
    bsm.update_blocks(A, src_list(cut_operator(kind, D2, sets)))
    kept = [b.data_ptr() for b in M.blocks]
    M.refresh()
    assert M.kind == "abs" and [b.data_ptr() for b in M.blocks] == kept
    assert all(np.all(w.cpu().numpy() < 0) if s % 2 == 0 else np.all(w.cpu().numpy() > 0) for s, w in enumerate(M.eigenvalues))
    X2, info2 = S.solve(dev_copy(torch, B), rtol=rtol, maxiter=200)
    check_columns(info2, runs2, D2, X2.cpu().numpy(), B, [column_tol(B[:, c], rtol) for c in range(NB)], f"after the update {name(dtype)}")
    check_products(info2, True)


def test_lobpcg_with_the_abs_preconditioner_of_a_definite_operator(torch_cuda, bsm):
    """there |A_ss|^-1 IS the inverse: the same pairs as with kind="inverse", both to the acceptance of _lobpcg.py"""
    from _lobpcg import CG_CASE, NEIG, accept, cg_dense, eig_rtol, start_block, twin_of
    dtype = np.float64
    which, nev, block = CG_CASE
    assert (which, nev) == ("SA", 3)
    twin = twin_of("cg", dtype, which, nev, block)
    p, sets, D, _ = cg_dense(dtype)
    A = bsm.synthetic.build(p)
    got = {}
    for kind in ("abs", "inverse"):
        M = bsm.block_jacobi(A, sets, kind=kind)
        w, X, info = bsm.Lobpcg(A, nev=3, block=block, M=M, which="SA").solve(dev_copy(torch_cuda, start_block(NEIG, block, dtype)),
                                                                             rtol=eig_rtol(dtype), maxiter=2 * twin.iterations)
        accept(torch_cuda, w, X, info, D, twin, nev, block, which, dtype, f"block-Jacobi kind={kind}", has_m=True)
        got[kind] = (w, np.sqrt(nev) * float(np.max(info.residual)) + NEIG * float(np.finfo(dtype).eps) * info.anorm)
    assert np.all(np.abs(got["abs"][0] - got["inverse"][0]) <= got["abs"][1] + got["inverse"][1])
    assert all(np.all(w.cpu().numpy() > 0) for w in bsm.block_jacobi(A, sets, kind="abs").eigenvalues)
