"""CPU suite of the Krylov layer: the numpy twin that the GPU suite measures bsm_gmres_solve against must itself solve the
test problems (so that no GPU test rests on an oracle that fails alone), the argument checks of bsm_gmres_create and
bsm_krylov_orth that need no device, and the host form of the solver's small dense step (Givens rotations + back
substitution, the test hook bsm_debug_krylov_lsq_host) against numpy.linalg.lstsq."""
import numpy as np
import pytest

from _jacobi import CODE, DTYPES, KINDS
from _krylov import (ERR_DEVICE, ERR_INVALID, MAX_RESTART, RESTART, Truth, exact_minv, gmres_twin, krylov_problem, lsq_hook, raw_gmres_create,
                     raw_gmres_destroy, raw_lsq, raw_orth, raw_orth_work, real_of, rtol_of, true_residual)

NODEV = -2  # BSM_DEVICE_NONE
IDS = [np.dtype(d).name for d in DTYPES]


@pytest.fixture(scope="module")
def twins():
    """(kind, dtype name) -> (D, b, preconditioned twin run, unpreconditioned twin run of 50 iterations), computed once"""
    out = {}
    for kind in KINDS:
        for dt in DTYPES:
            p, sets, b = krylov_problem(kind, dt)
            D = Truth(p).D
            out[kind, np.dtype(dt).name] = (D, b, gmres_twin(D, b, exact_minv(D, sets), RESTART, rtol_of(dt), 100, dt),
                                            gmres_twin(D, b, None, RESTART, 0.0, 50, dt))
    return out


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_twin_converges_with_the_exact_block_inverse(twins, kind, dtype):
    D, b, run, _ = twins[kind, np.dtype(dtype).name]
    rtol = rtol_of(dtype)
    assert run.status == 0 and 1 <= run.iterations <= 100
    assert run.history[-1] <= rtol * run.bnorm and np.all(run.history[:-1] > rtol * run.bnorm)
    true = true_residual(D, run.x, b)
    print(f"KRYSTAT twin {kind} {np.dtype(dtype).name}: {run.iterations} iterations, true residual / (rtol |b|) = {true / (rtol * run.bnorm):.3f}")
    assert true <= 2 * rtol * run.bnorm


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_twin_stagnates_without_a_preconditioner_and_says_so(twins, kind, dtype):
    D, b, _, run = twins[kind, np.dtype(dtype).name]
    assert run.status == 1 and run.iterations == 50 and run.cycles == 3
    assert run.residual >= 0.9 * run.bnorm
    true = true_residual(D, run.x, b)
    assert abs(run.residual - true) <= 10 * np.finfo(dtype).eps * true


# ---- what the C ABI answers without a device -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def handles(bsm):
    """analysis-only handles: a square float64 operator, its block-Jacobi preconditioner, an operator of another order, a
    non-square one, a complex one"""
    p, sets, _ = krylov_problem("blocksparse", np.float64)
    A = bsm.synthetic.build(p, device=NODEV)
    M = bsm.block_jacobi(A, sets)
    small = bsm.BlockSparseMatrix([np.eye(3)], [[1, 2, 3]], [[1, 2, 3]], (3, 3), device=NODEV)
    rect = bsm.BlockSparseMatrix([np.ones((2, 3))], [[1, 2]], [[1, 2, 3]], (4, 5), device=NODEV)
    pc, _, _ = krylov_problem("blocksparse", np.complex128)
    return A, M, small, rect, bsm.synthetic.build(pc, device=NODEV)


def test_create_refuses_analysis_only_handles(handles):
    A, M, *_ = handles
    for m in (None, M):
        rc, ptr = raw_gmres_create(A, 0, m, 0, CODE[np.dtype(np.float64)], RESTART)
        assert rc == ERR_DEVICE and not ptr.value


def test_python_wrapper_raises_through_the_error_path(bsm, handles):
    A, M, small, rect, _ = handles
    with pytest.raises(bsm._lib.BsmError, match="no device image"):
        bsm.Gmres(A, M, restart=RESTART)
    with pytest.raises(bsm._lib.BsmError, match="restart"):
        bsm.Gmres(A, restart=0)
    with pytest.raises(TypeError):
        bsm.Gmres(np.eye(3))
    with pytest.raises(TypeError):
        bsm.Gmres(A, dtype=np.int32)


def test_create_argument_checks(handles):
    A, M, small, rect, Ac = handles
    f64, c128, f32, c64 = (CODE[np.dtype(t)] for t in (np.float64, np.complex128, np.float32, np.complex64))
    bad = [
        ("restart 0", (A, 0, M, 0, f64, 0)),
        ("restart above the bound", (A, 0, M, 0, f64, MAX_RESTART + 1)),
        ("negative restart", (A, 0, None, 0, f64, -3)),
        ("non-square operator", (rect, 0, None, 0, f64, RESTART)),
        ("non-square operator, transposed", (rect, 1, None, 0, f64, RESTART)),
        ("M of another order", (A, 0, small, 0, f64, RESTART)),
        ("bad opA", (A, 3, None, 0, f64, RESTART)),
        ("bad opM", (A, 0, M, -1, f64, RESTART)),
        ("mixed storage code as vdtype", (A, 0, None, 0, 4, RESTART)),
        ("bad vdtype", (A, 0, None, 0, 9, RESTART)),
        ("a float64 operator under float32 vectors", (A, 0, None, 0, f32, RESTART)),
        ("a float64 operator under complex64 vectors", (A, 0, None, 0, c64, RESTART)),
        ("a complex operator under real vectors", (Ac, 0, None, 0, f64, RESTART)),
        ("a complex preconditioner under real vectors", (A, 0, Ac, 0, f64, RESTART)),
        ("null operator", (None, 0, None, 0, f64, RESTART)),
    ]
    for what, args in bad:
        rc, ptr = raw_gmres_create(*args)
        assert rc == ERR_INVALID and not ptr.value, what
    # what is acceptable up to the missing device answers BSM_ERR_DEVICE: the pairs a solver takes
    for what, args in [("real operator, complex vectors", (A, 0, M, 0, c128, RESTART)), ("adjoint", (A, 2, M, 2, f64, 1)),
                       ("the bound itself", (A, 0, None, 0, f64, MAX_RESTART))]:
        rc, ptr = raw_gmres_create(*args)
        assert rc == ERR_DEVICE and not ptr.value, what
    assert raw_gmres_destroy(None) == 0


def test_mixed_storage_handles_count_with_their_double_vectors(bsm):
    p, _, _ = krylov_problem("vbcrs", np.float64)
    A = bsm.synthetic.build(p, device=NODEV, storage=np.float32)
    assert raw_gmres_create(A, 0, None, 0, CODE[np.dtype(np.float64)], 5)[0] == ERR_DEVICE
    assert raw_gmres_create(A, 0, None, 0, CODE[np.dtype(np.float32)], 5)[0] == ERR_INVALID
    assert raw_gmres_create(A, 0, None, 0, CODE[np.dtype(np.complex128)], 5)[0] == ERR_INVALID  # bsm_mul_cvec refuses it too


def test_orth_argument_checks_come_before_any_launch():
    """every refusal of bsm_krylov_orth is answered on the host: fake, 16-byte aligned addresses are never dereferenced"""
    f64 = CODE[np.dtype(np.float64)]
    V, w, h, nrm, work = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000
    assert raw_orth_work(f64, 400, 20) > 0 and raw_orth_work(f64, 0, 0) > 0
    assert raw_orth_work(f64, 70001, MAX_RESTART) >= raw_orth_work(f64, 400, MAX_RESTART)
    for code in (4, 5, 7, -1):
        assert raw_orth(code, 10, 2, V, 10, w, h, nrm, work) == ERR_INVALID
        assert raw_orth_work(code, 10, 2) == ERR_INVALID
    assert raw_orth_work(f64, -1, 2) == ERR_INVALID and raw_orth_work(f64, 10, MAX_RESTART + 1) == ERR_INVALID
    bad = [(-1, 2, V, 10, w, h, nrm, work), (10, -1, V, 10, w, h, nrm, work), (10, MAX_RESTART + 1, V, 10, w, h, nrm, work),
           (10, 2, V, 9, w, h, nrm, work), (10, 2, None, 10, w, h, nrm, work), (10, 2, V, 10, None, h, nrm, work),
           (10, 2, V, 10, w, None, nrm, work), (10, 2, V, 10, w, h, None, work), (10, 2, V, 10, w, h, nrm, None),
           (10, 2, V, 10, w, h, nrm, work + 8)]
    for args in bad:
        assert raw_orth(f64, *args) == ERR_INVALID, args


# ---- the host form of hess / trsolve ------------------------------------------------------------------------------------------
def hessenberg(rng, k, dtype, zero_at=None):
    """(k + 1) x k upper Hessenberg: entries uniform in (-1, 1) / sqrt(k), the subdiagonal real and in (0.1, 1) -- the
    norms GMRES puts there -- plus 2 on the diagonal (conditioned like a preconditioned operator: a random triangle of
    unscaled entries has a condition number that grows exponentially with k); zero_at: that subdiagonal entry is 0"""
    H = np.triu(rng.uniform(-1, 1, (k + 1, k)) + (1j * rng.uniform(-1, 1, (k + 1, k)) if np.dtype(dtype).kind == "c" else 0), -1)
    H = (H / np.sqrt(k)).astype(dtype)
    H[np.arange(k), np.arange(k)] += 2
    H[np.arange(1, k + 1), np.arange(k)] = rng.uniform(0.1, 1, k)
    if zero_at is not None:
        H[zero_at + 1, zero_at] = 0
    return H


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("k", [1, 2, 20, MAX_RESTART])
def test_host_rotations_and_back_substitution_against_lstsq(k, dtype):
    """y and every prefix's residual norm against numpy.linalg.lstsq in float64 / complex128.  Bounds: Givens QR is
    backward stable, |dy| <= c k eps cond(H) |y| and |d res_j| <= c k eps |beta|; cond(H) <= 10 for these matrices over
    the sizes used (checked below), c = 8 covers the constants of the rotation and the complex arithmetic."""
    rng = np.random.default_rng(4000 + k)
    eps, wide = np.finfo(dtype).eps, np.complex128 if np.dtype(dtype).kind == "c" else np.float64
    for zero_at in (None, k // 2):
        H = hessenberg(rng, k, dtype, zero_at)
        beta = 1.75
        rc, y, res, R = raw_lsq(H, beta, ldh=k + 3)
        assert rc == 0 and np.all(np.isfinite(y)) and np.all(np.isfinite(res))
        Hw = H.astype(wide)
        cond = np.linalg.cond(Hw)
        assert cond <= 10
        e1 = np.zeros(k + 1, wide)
        e1[0] = beta
        want = np.linalg.lstsq(Hw, e1, rcond=None)[0]
        assert np.linalg.norm(y - want) <= 8 * k * eps * cond * np.linalg.norm(want), (k, zero_at)
        for j in range(k):
            yj = np.linalg.lstsq(Hw[:j + 2, :j + 1], e1[:j + 2], rcond=None)[0]
            rj = np.linalg.norm(e1[:j + 2] - Hw[:j + 2, :j + 1] @ yj)
            assert abs(res[j] - rj) <= 8 * k * eps * beta, (k, zero_at, j)
        if zero_at is not None:  # the lucky breakdown: the system is solved exactly at that column
            assert res[zero_at] <= 8 * k * eps * beta
        # R is upper triangular with the subdiagonal cleared, and |R| has H's column norms (rotations are unitary)
        assert np.all(np.tril(R, -1) == 0)
        assert np.allclose(np.linalg.norm(R.astype(wide), axis=0), np.linalg.norm(Hw, axis=0), rtol=8 * k * eps)


def test_host_form_all_zero_column_gives_no_nan():
    for dtype in DTYPES:
        H = np.zeros((3, 2), dtype)
        H[0, 1] = 1
        rc, y, res, _ = raw_lsq(H, 2.0)
        assert rc == 0 and np.all(np.isfinite(y)) and np.all(np.isfinite(res)) and res[0] == 2.0


def test_host_form_argument_checks():
    H = hessenberg(np.random.default_rng(1), 3, np.float64)
    assert raw_lsq(H, 1.0, ldh=3)[0] == ERR_INVALID
    y = np.zeros(4)
    for code, k in ((4, 3), (1, 0), (1, MAX_RESTART + 1)):
        assert lsq_hook()(code, k, H.ctypes.data, MAX_RESTART + 2, 1.0, y.ctypes.data, None) == ERR_INVALID
    assert raw_lsq(H, 1.0, res=False)[0] == 0
    assert real_of(np.complex64) == np.float32
