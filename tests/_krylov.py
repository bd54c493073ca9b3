"""What the Krylov suites (test_krylov_cpu.py, test_gpu_krylov_orth.py, test_gpu_gmres.py) share: the numpy twin of the
solver, the test problems, and raw ctypes drivers of bsm_krylov_orth, bsm_gmres_create / _solve and the test hook bsm_debug_krylov_lsq_host.  Test
code only.

The twin.  gmres_twin is right-preconditioned restarted GMRES with two classical Gram-Schmidt passes per iteration and a
least-squares solve (numpy.linalg.lstsq) on the Hessenberg matrix, every array and every product in `dtype`: the method
bsm_gmres_solve documents, with none of its code (no rotations, no back substitution).  Its estimate after iteration j is
the least-squares residual of the (j + 2) x (j + 1) Hessenberg system.

The problems.  The 12 operators of _jacobi.jacobi_problem (3 kinds x 4 types, order 400, seed 3000 + KINDS.index(kind)),
b uniform in (-1, 1) and real for the complex types too, drawn from the same generator after the problem.  Without a
preconditioner GMRES(20) stagnates on all of them (relative residual 0.97 .. 0.99 after 50 iterations); with the exact
block-Jacobi inverse it reaches rtol 1e-4 (single) / 1e-10 (double) in 3 .. 39 iterations."""
import ctypes as C

import numpy as np

from _jacobi import CODE, KINDS, NOP, dense_of, jacobi_problem, set_blocks
from _submat import Truth

RESTART = 20
MAX_RESTART = 128  # BSM_GMRES_MAX_RESTART
ERR_INVALID, ERR_UNSUPPORTED, ERR_DEVICE = -1, -2, -3


def rtol_of(dtype):
    return 1e-4 if np.finfo(dtype).eps > 1e-10 else 1e-10


def wide_of(dtype):
    return np.complex128 if np.dtype(dtype).kind == "c" else np.float64


def real_of(dtype):
    return np.zeros(1, dtype).real.dtype


def krylov_problem(kind, dtype):
    """-> (problem, sets, b): the operator, its index sets and the right-hand side"""
    rng = np.random.default_rng(3000 + KINDS.index(kind))
    p, sets = jacobi_problem(rng, kind, dtype)
    b = rng.uniform(-1, 1, NOP).astype(dtype)
    return p, sets, b


def exact_minv(D, sets, dtype=None):
    """the block-Jacobi inverse of the dense D over `sets`, inverted in float64 / complex128 and rounded to dtype"""
    dtype = D.dtype if dtype is None else dtype
    blocks = [np.linalg.inv(blk.astype(wide_of(D.dtype))).astype(dtype) for blk in set_blocks(D, sets)]
    return dense_of(blocks, sets, D.shape[0], dtype)


def true_residual(D, x, b):
    """|| b - D x ||_2 in complex128"""
    return float(np.linalg.norm(b.astype(np.complex128) - D.astype(np.complex128) @ np.asarray(x).astype(np.complex128)))


class TwinResult:
    def __init__(self, x, history, status, cycles, bnorm):
        self.x, self.history, self.status, self.cycles, self.bnorm = x, np.array(history, dtype=np.float64), status, cycles, bnorm
        self.iterations = len(history)
        self.residual = history[-1] if history else bnorm


def gmres_twin(D, b, Minv, restart, rtol, maxiter, dtype, atol=0.0, x0=None):
    """numpy twin of bsm_gmres_solve (module docstring) -> TwinResult.  Minv: dense preconditioner or None"""
    dtype = np.dtype(dtype)
    n = len(b)
    D = np.asarray(D).astype(dtype)
    Minv = None if Minv is None else np.asarray(Minv).astype(dtype)
    b = b.astype(dtype)
    x = np.zeros(n, dtype) if x0 is None else x0.astype(dtype)
    bnorm = float(np.linalg.norm(b))
    tol = max(rtol * bnorm, atol)
    hist, cycles, status = [], 0, 1
    first = True
    while True:
        r = b.copy() if (first and x0 is None) else (b - (D @ x).astype(dtype)).astype(dtype)
        first = False
        beta = np.linalg.norm(r).astype(real_of(dtype))
        if not np.isfinite(beta):
            status = 2
            break
        if beta <= tol:
            status = 0
            break
        if len(hist) >= maxiter:
            break
        cycles += 1
        m = int(min(restart, maxiter - len(hist)))
        V = np.zeros((n, m + 1), dtype)
        H = np.zeros((m + 1, m), dtype)
        V[:, 0] = r / beta
        k, done = 0, False
        y = np.zeros(0, dtype)
        for j in range(m):
            z = V[:, j] if Minv is None else (Minv @ V[:, j]).astype(dtype)
            w = (D @ z).astype(dtype)
            for _ in range(2):
                h = (V[:, :j + 1].conj().T @ w).astype(dtype)
                w = (w - V[:, :j + 1] @ h).astype(dtype)
                H[:j + 1, j] += h
            hn = np.linalg.norm(w).astype(real_of(dtype))
            H[j + 1, j] = hn
            V[:, j + 1] = w / hn if hn != 0 else 0
            e1 = np.zeros(j + 2, dtype)
            e1[0] = beta
            y = np.linalg.lstsq(H[:j + 2, :j + 1], e1, rcond=None)[0].astype(dtype)
            est = float(np.linalg.norm((e1 - H[:j + 2, :j + 1] @ y).astype(dtype)))
            hist.append(est)
            k = j + 1
            if not np.isfinite(est):
                status, done = 2, True
                break
            if est <= tol:
                status, done = 0, True
                break
        if status == 2:
            break
        u = (V[:, :k] @ y).astype(dtype)
        x = (x + (u if Minv is None else (Minv @ u).astype(dtype))).astype(dtype)
        if done:
            break
        if len(hist) >= maxiter:
            break
    return TwinResult(x, hist, status, cycles, bnorm)


def expected_products(iterations, cycles, use_x0, has_m):
    """(a_products, m_products) the documented method issues for a solve that ended inside (or at the end of) cycle
    `cycles` without a further residual product: one product per iteration, one residual product per cycle but the first
    of a solve from zero, one M product per cycle for x += M u"""
    a = iterations + cycles - (0 if use_x0 else 1) if cycles > 0 else (1 if use_x0 else 0)
    return a, (iterations + cycles) if has_m else 0


# ---- what the GPU suite accepts (test_gpu_gmres.py; the solver table of _lockstep.py) -------------------------------------
def check_history(info, tol, restart, dtype):
    """len(history) == iterations; a solve that converged on an ESTIMATE ends on an entry <= tol with every earlier one
    above it (one that converged on the true residual at a restart -- info.residual is then not the last entry -- has
    every entry above tol and that residual <= tol); inside each cycle the history does not rise.
    |g[j + 1]| = |s| |g[j]|.  Real types: s = +-hn / hypot(t, hn) and hypot(t, hn) >= hn, so |s| <= 1 in floating point
    too: no slack.  Complex types: s = (a / |a|) hn / r carries the rounded phase -- |a| and the final modulus are hypots
    (1 ulp = eps each), the divisions and the rounding of s eps / 2 each, the complex product conj(s) g sqrt(2) eps: under
    5 eps(T) relative in all; 8 eps(T) is allowed."""
    h = info.history
    assert len(h) == info.iterations
    if info.status == 0 and info.iterations:
        if info.residual == h[-1]:
            assert h[-1] <= tol and np.all(h[:-1] > tol)
        else:
            assert info.residual <= tol and np.all(h > tol)
    slack = 8 * float(np.finfo(dtype).eps) if np.dtype(dtype).kind == "c" else 0.0
    for c0 in range(0, len(h), restart):
        c = h[c0:c0 + restart]
        assert np.all(c[1:] <= c[:-1] * (1 + slack)), ("history rises inside a cycle", c0, float(np.max(c[1:] / c[:-1]) - 1))
    assert info.cycles == -(-info.iterations // restart)


def check_against_twin(info, twin, what):
    assert twin.status == 0, (what, "the twin did not converge")
    slack = max(2, twin.iterations // 10)
    print(f"KRYSTAT gmres {what}: {info.iterations} iterations, twin {twin.iterations}")
    assert info.iterations <= twin.iterations + slack, (what, info.iterations, twin.iterations)


# ---- raw ctypes drivers --------------------------------------------------------------------------------------------------
def raw_orth_work(code, n, k):
    from bsm_amd import _lib as L
    return L.lib().bsm_krylov_orth_work(code, n, k)


def raw_orth(code, n, k, V, ldv, w, hsum, nrm, work, stream=None):
    """bsm_krylov_orth as C sees it (device addresses or None) -> return code"""
    from bsm_amd import _lib as L
    return L.lib().bsm_krylov_orth(code, n, k, V, ldv, w, hsum, nrm, work, stream)


def lsq_hook():
    """the unexported test hook bsm_debug_krylov_lsq_host(dtype, k, H, ldh, beta, y, res) (csrc/bsm_krylov.cpp)"""
    from bsm_amd import _lib as L
    fn = L.lib().bsm_debug_krylov_lsq_host
    fn.argtypes = [C.c_int, C.c_int32, C.c_void_p, C.c_int64, C.c_double, C.c_void_p, C.POINTER(C.c_double)]
    fn.restype = C.c_int
    return fn


def raw_lsq(H, beta, ldh=None, res=True):
    """the host form of the solver's rotations and back substitution on a copy of the (k + 1) x k Hessenberg H ->
    (return code, y, res, R)"""
    k = H.shape[1]
    ldh = k + 1 if ldh is None else ldh
    buf = np.zeros((k, max(ldh, k + 1)), dtype=H.dtype)
    buf[:, :k + 1] = H.T
    y = np.zeros(k, dtype=H.dtype)
    r = np.zeros(k, dtype=np.float64)
    rc = lsq_hook()(CODE[np.dtype(H.dtype)], k, buf.ctypes.data, ldh, float(beta), y.ctypes.data,
                    r.ctypes.data_as(C.POINTER(C.c_double)) if res else None)
    return rc, y, r, buf[:, :k + 1].T.copy()


def raw_gmres_create(A, opA, M, opM, code, restart):
    """bsm_gmres_create as C sees it -> (return code, solver pointer); a created solver is destroyed by the caller"""
    from bsm_amd import _lib as L
    out = C.c_void_p()
    rc = L.lib().bsm_gmres_create(None if A is None else A._h.ptr, opA, None if M is None else M._h.ptr, opM, code, restart,
                                  C.byref(out))
    return rc, out


def raw_gmres_destroy(ptr):
    from bsm_amd import _lib as L
    return L.lib().bsm_gmres_destroy(ptr)


def raw_gmres_solve(ptr, b, x, rtol=1e-8, atol=0.0, maxiter=100, use_x0=0, capacity=None, hist_len=None, memspace=1, stream=None,
                    struct_size=None):
    """bsm_gmres_solve as C sees it (b, x: addresses) -> (return code, info, history buffer of hist_len doubles prefilled
    with -1; hist_len None: no history is passed)"""
    from bsm_amd import _lib as L
    cap = maxiter if capacity is None else capacity
    p = L.BsmGmresParams(C.sizeof(L.BsmGmresParams) if struct_size is None else struct_size, use_x0, rtol, atol, maxiter, cap)
    info = L.BsmGmresInfo()
    hist = None if hist_len is None else np.full(hist_len, -1.0)
    rc = L.lib().bsm_gmres_solve(ptr, b, x, C.byref(p), C.byref(info), None if hist is None else hist.ctypes.data_as(C.POINTER(C.c_double)),
                                 memspace, stream)
    return rc, info, hist
