"""What the suites of bsm_gmres_multi_solve / GmresMulti (test_gmres_multi_cpu.py, test_gpu_gmres_multi.py) share: the numpy
twin of one column of the lockstep solve, the spread of that twin under permuted summation orders, the Python mirror of the
workspace carve of bsm_gmres_multi_create, the history rules, and raw ctypes drivers.  Test code only.

The twin.  gmres_multi_twin is the method of _krylov.gmres_twin -- right-preconditioned restarted GMRES, two classical
Gram-Schmidt passes per iteration, a dense least-squares solve on the Hessenberg matrix (no rotations, no back substitution:
none of the library's code), every array and product in `dtype` -- with what the lockstep suites need on top: the operator as a
dense array or a _cg.BlockDiagonal, `order=` (a permutation the sums of every dot, norm and product run in), `keep=` (the
mutation of the tests of the tests: every dot sums its first `keep` terms only, as a kernel that loses the last workgroup's
share would) and the iterate after EVERY iteration (x of the cycle's start plus M V y of the least-squares solution so far:
what a solve cut at that count returns).  A column of a lockstep solve is, as a method, its stand-alone solve, so the twin
has one column.

The least-squares solve.  lsq="qr" (the default) is Householder QR (numpy.linalg.qr) and a triangular solve; lsq="lstsq" is
numpy.linalg.lstsq as in _krylov.gmres_twin, kept for the comparison with that twin.  The iterate checks need the former:
lstsq's SVD driver returned y 31 .. 163 eps off the 40-digit solution of a 4 x 3 Hessenberg system of condition number 4.9
(float64, n = 1025, column 0 of the grid problem, iteration 3; gelss does the same), the same error under every permuted
summation order, so that no spread shows it, while QR stays within 3.5 eps and the library's rotations within 0.9
(test_gmres_multi_cpu.py pins this).  The estimate is the residual norm of that solution in both forms.

Units are those of _lockstep.deviation: an iterate in eps max|x|, a history in eps ||b||."""
import ctypes as C

import numpy as np

from _cg import MAX_RHS, NB, BlockDiagonal, column_tol
from _jacobi import DTYPES, KINDS, NOP, uniform
from _krylov import MAX_RESTART, expected_products, real_of, true_residual
from _lockstep import MARGIN, deviation, krylov_grid, reference_of

GRID_RESTART = 3  # of the grid tests: maxiter = GRID_ITS takes one restart, with its op(A) X product and the second start
GRID_ITS = 5
ORDERS = 8        # permutations of a spread, as in _lockstep.spread
# sizeof(GmState) (csrc/bsm_gmres_multi.h): two slots of 16 doubles and 4 x 16 int32, tol, bnorm, and the CgRecord
STATE_BYTES = 2 * (16 * 8 + 4 * 16 * 4) + 16 * 8 + 16 * 8 + (2 * 16 * 8 + 2 * 16 * 4)


class GmTwin:
    def __init__(self, x, history, status, cycles, bnorm, iterates, residual):
        self.x, self.history, self.status, self.cycles, self.bnorm = x, np.array(history, dtype=np.float64), status, cycles, bnorm
        self.iterations = len(history)
        self.iterates = iterates  # x after every iteration
        self.residual = residual  # the last estimate, or the true residual norm of the start that ended the solve
        self.hessenberg = self.beta = None  # of the last cycle that ran: (k + 1) x k, and the norm it started from


def gmres_multi_twin(D, b, Minv, restart, rtol, maxiter, dtype, atol=0.0, x0=None, order=None, keep=None, lsq="qr"):
    """numpy twin of one column of bsm_gmres_multi_solve (module docstring) -> GmTwin.  D: dense array or BlockDiagonal;
    Minv: dense preconditioner or None; order / keep (not together) and lsq: module docstring"""
    dtype = np.dtype(dtype)
    real = real_of(dtype)
    D = D.astype(dtype) if isinstance(D, BlockDiagonal) else np.asarray(D).astype(dtype)
    Minv = None if Minv is None else np.asarray(Minv).astype(dtype)
    b = np.asarray(b).astype(dtype)
    n = len(b)
    perm = np.arange(n) if order is None else order
    assert order is None or keep is None

    def dots(V, w):  # V^H w, one fixed-order sum per basis vector
        terms = (np.conj(V) * w[:, None]).astype(dtype)
        return np.sum(terms[perm] if keep is None else terms[:keep], axis=0, dtype=dtype)

    def norm(v):
        return np.linalg.norm(v if order is None else v[perm]).astype(real)

    def times(H, v):
        if isinstance(H, BlockDiagonal):
            return H.times(v, order).astype(dtype)
        if order is None:
            return (H @ v).astype(dtype)
        return (np.ascontiguousarray(H[:, perm]) @ v[perm]).astype(dtype)

    def hat(v):
        return v if Minv is None else times(Minv, v)

    def least_squares(H, e):
        if lsq == "lstsq":
            return np.linalg.lstsq(H, e, rcond=None)[0].astype(dtype)
        Q, R = np.linalg.qr(H)
        d = np.abs(np.diag(R))
        if np.min(d) <= np.finfo(dtype).eps * np.max(d):  # (a lucky breakdown leaves a column of zeros: minimum norm)
            return np.linalg.lstsq(H, e, rcond=None)[0].astype(dtype)
        return np.linalg.solve(R, (Q.conj().T @ e).astype(dtype)).astype(dtype)

    with np.errstate(all="ignore"):
        x = np.zeros(n, dtype) if x0 is None else np.asarray(x0).astype(dtype)
        bnorm = float(norm(b))
        tol = max(rtol * bnorm, atol)
        hist, its, cycles, status = [], [], 0, 1
        residual = bnorm
        first = True
        while True:
            r = b.copy() if (first and x0 is None) else (b - times(D, x)).astype(dtype)
            first = False
            beta = norm(r)
            residual = float(beta)
            if not np.isfinite(beta):
                status = 2
                break
            if beta <= tol:
                status = 0
                break
            if len(hist) >= maxiter:
                break
            cycles += 1
            last_beta = beta
            m = int(min(restart, maxiter - len(hist)))
            V = np.zeros((n, m + 1), dtype)
            H = np.zeros((m + 1, m), dtype)
            V[:, 0] = r / beta
            k, done = 0, False
            u = np.zeros(n, dtype)
            for j in range(m):
                w = times(D, hat(V[:, j]))
                for _ in range(2):
                    h = dots(V[:, :j + 1], w)
                    w = (w - V[:, :j + 1] @ h).astype(dtype)
                    H[:j + 1, j] += h
                hn = norm(w)
                H[j + 1, j] = hn
                V[:, j + 1] = w / hn if hn != 0 else 0
                e1 = np.zeros(j + 2, dtype)
                e1[0] = beta
                if not np.all(np.isfinite(H[:j + 2, :j + 1])):
                    est = float("nan")
                else:
                    y = least_squares(H[:j + 2, :j + 1], e1)
                    est = float(np.linalg.norm((e1 - H[:j + 2, :j + 1] @ y).astype(dtype)))
                hist.append(est)
                residual = est
                k = j + 1
                if not np.isfinite(est):
                    status, done = 2, True
                    its.append(x.copy())
                    break
                u = (V[:, :k] @ y).astype(dtype)
                its.append((x + hat(u)).astype(dtype))
                if est <= tol:
                    status, done = 0, True
                    break
            if status == 2:
                break
            x = its[-1]
            if done or len(hist) >= maxiter:
                break
    out = GmTwin(x, hist, status, cycles, bnorm, its, residual)
    if cycles:
        out.hessenberg, out.beta = H[:k + 1, :k].copy(), float(last_beta)
    return out


def reference(Dop, b, its, dtype, restart=GRID_RESTART, Minv=None, x0=None):
    """the twin's run of `its` iterations (rtol = 0) on the operator and right-hand side AS ROUNDED to dtype, evaluated in
    _lockstep.reference_of(dtype)"""
    return gmres_multi_twin(Dop, b, Minv, restart, 0.0, its, reference_of(dtype), x0=x0)


def spread(Dop, b, its, dtype, restart=GRID_RESTART, orders=ORDERS, Minv=None, x0=None, lsq="qr"):
    """_lockstep.spread for this twin: the largest deviation() of its iterate number `its` and of its history from the
    unpermuted run IN dtype over `orders` permutations (seeds 0 ..) -> (iterate: eps max|x|, history: eps ||b||)"""
    a = gmres_multi_twin(Dop, b, Minv, restart, 0.0, its, dtype, x0=x0, lsq=lsq)
    assert a.status == 1 and a.iterations == its, (a.status, a.iterations)
    sx = sh = 0.0
    for seed in range(orders):
        o = np.random.default_rng(seed).permutation(len(b))
        p = gmres_multi_twin(Dop, b, Minv, restart, 0.0, its, dtype, x0=x0, order=o, lsq=lsq)
        dx, dh = deviation(p.x, p.history, a, its, dtype)
        sx, sh = max(sx, dx), max(sh, dh)
    return sx, sh


_spreads = {}


def grid_spread(tag, Dop, B, k, dtype, **kw):
    """the bound's spread of a grid case: the larger of the spreads of columns 0 and k - 1 of B, each measured once per
    (tag, column) -> (iterate, history)"""
    for c in {0, k - 1}:
        if (tag, c) not in _spreads:
            _spreads[tag, c] = spread(Dop, B[:, c], GRID_ITS, dtype, **{key: (v[:, c] if key == "x0" and v is not None else v)
                                                                      for key, v in kw.items()})
    return max(_spreads[tag, 0][0], _spreads[tag, k - 1][0]), max(_spreads[tag, 0][1], _spreads[tag, k - 1][1])


def workspace_bytes(n, dtype, restart, kmax=MAX_RHS, has_m=False, G=None):
    """info.workspace_bytes as bsm_gmres_multi_create carves it: V_0 .. V_restart as one piece, W, X (Z with M), each matrix
    ld x kmax (ld: n rounded up to whole 16-byte groups); per column the Hessenberg factor, cs, sn, g, y, hsum, 1 / ||w||, the
    partials of a pass (restart * G elements) and the G norm shares; the state; every piece rounded up to 64 bytes"""
    es, rs = np.dtype(dtype).itemsize, np.dtype(real_of(dtype)).itemsize
    G = krylov_grid(n, es) if G is None else G
    ld = (max(n, 1) * es + 15) // 16 * 16 // es
    vec, m, K = ld * es * kmax, restart, kmax
    pieces = [vec * (m + 1), vec, vec] + ([vec] if has_m else [])
    pieces += [K * m * (m + 1) * es, K * m * rs, K * m * es, K * (m + 1) * es, K * m * es, K * m * es, K * rs, K * m * G * es, K * G * rs]
    return sum((p + 63) // 64 * 64 for p in pieces + [STATE_BYTES])


def cycles_of(iterations, restart):
    return -(-int(iterations) // restart)


def check_history(h, status, residual, tol, restart, dtype):
    """the history rules of one column (those of test_gpu_gmres.py's check_history, restated for a column of estimates h that
    holds exactly the column's own iterations): a column that converged on an ESTIMATE ends on an entry <= tol with every
    earlier one above it; one that converged on the true residual at a restart has every entry above tol and that residual
    <= tol; inside each cycle the history does not rise -- |g[j + 1]| = |s| |g[j]| with |s| <= 1, exactly for the real types,
    to 8 eps for the complex ones (the rounded phase of s)"""
    h = np.asarray(h, dtype=np.float64)
    if status == 0 and len(h):
        if residual == h[-1]:
            assert h[-1] <= tol and np.all(h[:-1] > tol)
        else:
            assert residual <= tol and np.all(h > tol)
    slack = 8 * float(np.finfo(dtype).eps) if np.dtype(dtype).kind == "c" else 0.0
    for c0 in range(0, len(h), restart):
        c = h[c0:c0 + restart]
        assert np.all(c[1:] <= c[:-1] * (1 + slack)), ("history rises inside a cycle", c0, float(np.max(c[1:] / c[:-1]) - 1))


# ---- the order-400 columns and what the GPU suite accepts (test_gpu_gmres_multi.py; the solver table of _lockstep.py) ----
def columns400(kind, dtype):
    """five uniform right-hand sides of order 400 for krylov_problem(kind, dtype)"""
    rng = np.random.default_rng(9000 + 4 * KINDS.index(kind) + DTYPES.index(dtype))
    return np.asfortranarray(uniform(rng, (NOP, NB), dtype))


def products(info, restart, use_x0, has_m):
    """(a_products, m_products) by the documented formula (_krylov.expected_products on the largest count), plus the one
    true-residual product of a restart BEHIND the last iteration where a column was still running there and froze on that
    restart's true residual (its `residual` is then not its last estimate)"""
    its = int(info.iterations)
    a, m = expected_products(its, cycles_of(its, restart), use_x0, has_m)
    late = its > 0 and its % restart == 0 and any(
        info.column_status[c] == 0 and info.column_iterations[c] == its and info.residual[c] != info.history[its - 1, c]
        for c in range(len(info.column_status)))
    return a + (1 if late else 0), m


def slack_of(twin_iterations):
    """what test_gpu_gmres.py's check_against_twin allows above the twin's count"""
    return max(2, twin_iterations // 10)


def check_columns(info, runs, D, xh, B, rtol, what):
    for c, run in enumerate(runs):
        assert info.column_status[c] == 0 and run.status == 0, (what, c)
        assert int(info.column_iterations[c]) <= run.iterations + slack_of(run.iterations), (what, c)
        assert true_residual(D, xh[:, c], B[:, c]) <= 2 * column_tol(B[:, c], rtol), (what, c)


# ---- raw ctypes drivers --------------------------------------------------------------------------------------------------
def raw_gm_create(A, opA, M, opM, code, nrhs_max, restart):
    """bsm_gmres_multi_create as C sees it -> (return code, solver pointer); a created solver is destroyed by the caller"""
    from bsm_amd import _lib as L
    out = C.c_void_p()
    rc = L.lib().bsm_gmres_multi_create(None if A is None else A._h.ptr, opA, None if M is None else M._h.ptr, opM, code, nrhs_max,
                                        restart, C.byref(out))
    return rc, out


def raw_gm_destroy(ptr):
    from bsm_amd import _lib as L
    return L.lib().bsm_gmres_multi_destroy(ptr)


def raw_gm_solve(ptr, nrhs, B, ldb, X, ldx, rtol=1e-8, atol=0.0, maxiter=100, use_x0=0, capacity=None, memspace=1, stream=None,
                 struct_size=None, want_cols=True):
    """bsm_gmres_multi_solve as C sees it (B, X: addresses) -> (return code, info, columns, history of `capacity` rows
    prefilled with -1)"""
    from bsm_amd import _lib as L
    cap = maxiter if capacity is None else capacity
    p = L.BsmCgParams(C.sizeof(L.BsmCgParams) if struct_size is None else struct_size, use_x0, rtol, atol, maxiter, cap)
    info = L.BsmCgInfo()
    cols = (L.BsmCgColumn * max(nrhs, 1))() if want_cols else None
    hist = np.full((max(cap, 1), max(nrhs, 1)), -1.0)
    rc = L.lib().bsm_gmres_multi_solve(ptr, nrhs, B, ldb, X, ldx, C.byref(p), C.byref(info), cols,
                                       hist.ctypes.data_as(C.POINTER(C.c_double)), memspace, stream)
    return rc, info, cols, hist


__all__ = ["GRID_ITS", "GRID_RESTART", "MARGIN", "MAX_RESTART", "MAX_RHS", "ORDERS", "GmTwin", "check_columns", "check_history",
           "columns400", "cycles_of", "gmres_multi_twin", "grid_spread", "products", "raw_gm_create", "raw_gm_destroy", "raw_gm_solve",
           "reference", "slack_of", "spread", "workspace_bytes"]
