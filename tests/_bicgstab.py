"""What the BiCGSTAB suites (test_bicgstab_cpu.py, test_gpu_bicgstab.py) share: the numpy twin of bsm_bicgstab_solve, the
test problems and raw ctypes drivers of bsm_bicgstab_create / _solve / _destroy.  Test code only.

The twin.  bicgstab_twin is right-preconditioned BiCGSTAB as include/bsm_rocm.h states the recurrences, the inner product
always conjugated, every array, product and scalar rounded to `dtype`, with the four statuses of a column (0 converged --
after either half of an iteration, or at the start --, 1 maxiter, 2 a non-finite residual norm, 3 breakdown: rho == 0 or
sigma == 0 at the top of an iteration, or tt == 0, ts == 0 or omega = ts / tt == 0 after a half step that did not converge) and the fixed order
of the checks of the second half: non-finite sn, sn <= tol, then tt == 0 or ts == 0.  It shares no code with the library.

The problems.  The main one is _cg.cg_problem's recipe WITHOUT the symmetrisation: order 400, rng = default_rng(6000),
sets = _submat.cut(rng, 400), G uniform in (-1, 1) (both parts for complex types), D0 = G + s I with s = 24 (real) / 36
(complex), D = W D0 W with W diagonal, constant on each set, 2**k with k = rng.integers(-3, 4) per set; B (400 x 5)
uniform.  D is cut into a 4 x 4 grid of 100 x 100 blocks (vbcrs) or one block per pair of sets (blocksparse); there is no
symmetric kind: D is not symmetric.  M = block_jacobi(A, sets); the twin takes the exact block inverse.  The layout-edge
operators are block diagonal: blocks T + 8 I of order 8 and one of order n mod 8, T uniform."""
import ctypes as C

import numpy as np

from _cg import MAX_RHS, BlockDiagonal, column_tol, is_complex  # noqa: F401
from _jacobi import CODE, uniform  # noqa: F401
from _krylov import ERR_DEVICE, ERR_INVALID, ERR_UNSUPPORTED, exact_minv, real_of, rtol_of, true_residual  # noqa: F401
from _submat import cut

NBI = 400
NB = 5
BI_KINDS = ["vbcrs", "blocksparse"]


def bicgstab_problem(kind, dtype):
    """-> (problem, sets, D, B): the operator as a constructor dictionary, its index sets, its dense form and the
    right-hand sides"""
    rng = np.random.default_rng(6000)
    sets = cut(rng, NBI)
    G = uniform(rng, (NBI, NBI), dtype)
    D0 = G + dtype(36 if is_complex(dtype) else 24) * np.eye(NBI, dtype=dtype)
    w = np.ones(NBI)
    for s in sets:
        w[s - 1] = 2.0 ** int(rng.integers(-3, 4))
    D = (w[:, None] * D0 * w[None, :]).astype(dtype)
    B = np.asfortranarray(uniform(rng, (NBI, NB), dtype))
    if kind == "vbcrs":
        blocks, rs, cs = [], [], []
        for a in range(0, NBI, 100):
            for b in range(0, NBI, 100):
                blocks.append(np.asfortranarray(D[a:a + 100, b:b + 100]))
                rs.append(a + 1)
                cs.append(b + 1)
        p = dict(kind="vbcrs", blocks=blocks, rowstart=np.array(rs, np.int64), colstart=np.array(cs, np.int64), size=(NBI, NBI))
    else:
        assert kind == "blocksparse"
        blocks, ri, ci = [], [], []
        for a in sets:
            for b in sets:
                blocks.append(np.asfortranarray(D[np.ix_(a - 1, b - 1)]))
                ri.append(a)
                ci.append(b)
        p = dict(kind="blocksparse", blocks=blocks, rowindices=ri, colindices=ci, size=(NBI, NBI))
    return p, sets, D, B


def staggered(B, dtype):
    """the CG suite's scaling of the columns -> (Bs, atol): column c scaled by step**-c, the last one zero"""
    tau, step = (1e-4, 10.0) if dtype == np.float32 else (1e-10, 1000.0)
    Bs = B.copy(order="F")
    for c in range(4):
        Bs[:, c] = (B[:, c] * dtype(step ** -c)).astype(dtype)
    Bs[:, 4] = 0
    return Bs, tau * float(np.linalg.norm(Bs[:, 0].astype(np.float64)))


def edge_problem(n, dtype, bs=8):
    """-> (vbcrs problem, BlockDiagonal, rng): diagonal blocks T + 8 I of order bs (the last one n mod bs), T uniform, seed
    7000 + 17 n; the generator is handed back for the right-hand sides"""
    rng = np.random.default_rng(7000 + 17 * n)
    nb, t = n // bs, n % bs
    main = (uniform(rng, (nb, bs, bs), dtype) + dtype(8) * np.eye(bs, dtype=dtype)).astype(dtype)
    tail = (uniform(rng, (t, t), dtype) + dtype(8) * np.eye(t, dtype=dtype)).astype(dtype)
    blocks = [np.asfortranarray(main[b]) for b in range(nb)] + ([np.asfortranarray(tail)] if t else [])
    starts = np.arange(len(blocks), dtype=np.int64) * bs + 1
    return dict(kind="vbcrs", blocks=blocks, rowstart=starts, colstart=starts.copy(), size=(n, n)), BlockDiagonal(main, tail), rng


def breakdown_problem(block, dtype, nb=3):
    """-> (vbcrs problem, dense D, B): diag(block, T + 8 I x nb) with the exact 2 x 2 `block` first; column 0 of B is e1 (of
    that block), column 1 is uniform on the other blocks only and converges"""
    rng = np.random.default_rng(7900)
    good = (uniform(rng, (nb, 8, 8), dtype) + dtype(8) * np.eye(8, dtype=dtype)).astype(dtype)
    n = 2 + 8 * nb
    D = np.zeros((n, n), dtype)
    D[:2, :2] = np.array(block, dtype=dtype)
    blocks, starts = [np.asfortranarray(D[:2, :2])], [1]
    for b in range(nb):
        D[2 + 8 * b:10 + 8 * b, 2 + 8 * b:10 + 8 * b] = good[b]
        blocks.append(np.asfortranarray(good[b]))
        starts.append(3 + 8 * b)
    B = np.zeros((n, 2), dtype, order="F")
    B[0, 0] = 1
    B[2:, 1] = uniform(rng, (n - 2,), dtype)
    starts = np.array(starts, np.int64)
    return dict(kind="vbcrs", blocks=blocks, rowstart=starts, colstart=starts.copy(), size=(n, n)), D, B


SIGMA_ZERO = [[0, 1], [1, 0]]  # b = e1: v = A e1 = e2, sigma = <e1, e2> = 0 at the top of iteration 1
TS_ZERO = [[1, 1], [-1, 0]]    # b = e1: alpha = 1, s = e2, t = A e2 = e1, ts = <e1, e2> = 0 after the half step x = e1


class BicgTwin:
    def __init__(self, x, history, status, bnorm, iterates, rn0):
        self.x, self.history, self.status, self.bnorm = x, np.array(history, dtype=np.float64), status, bnorm
        self.iterations = len(history)
        self.iterates = iterates  # x after every iteration
        self.residual = history[-1] if history else rn0


def bicgstab_twin(D, b, Minv, rtol, atol, maxiter, dtype, x0=None, order=None, keep=None):
    """numpy twin of one column of bsm_bicgstab_solve (module docstring) -> BicgTwin.  D: dense array or BlockDiagonal;
    Minv: dense preconditioner or None; order: a permutation the sums of the forms, of the norms and of the products run
    in (None: as stored; a BlockDiagonal permutes inside its blocks); keep: a MUTATION for the tests of the tests -- every
    form sums its first `keep` terms only, as a kernel that loses the last workgroup's share would (None: all; not
    together with order)"""
    dtype = np.dtype(dtype)
    real = real_of(dtype)
    D = D.astype(dtype)
    Minv = None if Minv is None else np.asarray(Minv).astype(dtype)
    b = np.asarray(b).astype(dtype)
    n = len(b)
    perm = np.arange(n) if order is None else order

    assert order is None or keep is None

    def form(u, v):
        terms = (np.conj(u) * v).astype(dtype)
        return np.sum(terms[perm] if keep is None else terms[:keep], dtype=dtype)

    def norm(v):
        return float(np.linalg.norm(v if order is None else v[perm]).astype(real))

    def times(H, v):
        if isinstance(H, BlockDiagonal):
            return H.times(v, order).astype(dtype)
        if order is None:
            return (H @ v).astype(dtype)
        return (np.ascontiguousarray(H[:, perm]) @ v[perm]).astype(dtype)

    def hat(v):
        return v if Minv is None else times(Minv, v)

    with np.errstate(all="ignore"):
        x = np.zeros(n, dtype) if x0 is None else np.asarray(x0).astype(dtype)
        r = b.copy() if x0 is None else (b - times(D, x)).astype(dtype)
        bnorm = norm(b)
        tol = max(rtol * bnorm, atol)
        rn0 = norm(r)
        status = 2 if not np.isfinite(rn0) else (0 if rn0 <= tol else None)
        hist, its = [], []
        rhat = r.copy()
        rho = form(rhat, r)
        p = r.copy()
        while status is None:
            if len(hist) >= maxiter:
                status = 1
                break
            phat = hat(p)
            v = times(D, phat)
            sigma = form(rhat, v)
            if rho == 0 or sigma == 0:
                status = 3  # nothing written, the count stays
                break
            alpha = dtype.type(rho / sigma)
            x = (x + alpha * phat).astype(dtype)
            r = (r - alpha * v).astype(dtype)  # s
            sn = norm(r)
            shat = hat(r)
            t = times(D, shat)
            ts, tt = form(t, r), form(t, t)
            if not np.isfinite(sn):
                status = 2
            elif sn <= tol:
                status = 0
            elif tt == 0 or ts == 0 or dtype.type(ts / tt) == 0:  # (the last: the quotient underflowed)
                status = 3
            if status is not None:
                hist.append(sn)
                its.append(x.copy())
                break
            omega = dtype.type(ts / tt)
            x = (x + omega * shat).astype(dtype)
            r = (r - omega * t).astype(dtype)
            rn = norm(r)
            hist.append(rn)
            its.append(x.copy())
            status = 2 if not np.isfinite(rn) else (0 if rn <= tol else None)
            if status is None:
                rhon = form(rhat, r)
                beta = dtype.type(dtype.type(rhon / rho) * dtype.type(alpha / omega))
                p = (r + beta * (p - omega * v).astype(dtype)).astype(dtype)
                rho = rhon
    return BicgTwin(x, hist, status, bnorm, its, rn0)


# the n x K table of the layout-edge tests, as the CG suite cuts it: all K for float64, both diagonals for the other types
EDGE_N = [1, 2, 63, 64, 65, 255, 256, 257, 1000]
EDGE_K = [1, 2, 3, 8, 16]
EDGE = [(np.float64, n, k) for n in EDGE_N for k in EDGE_K]
for _dt in (np.float32, np.complex64, np.complex128):
    for _i, _n in enumerate(EDGE_N):
        _j = _i * len(EDGE_K) // len(EDGE_N)
        EDGE += sorted({(_dt, _n, EDGE_K[_j]), (_dt, _n, EDGE_K[len(EDGE_K) - 1 - _j])}, key=lambda t: t[2])
EDGE_IDS = [f"{np.dtype(d).name}-n{n}-k{k}" for d, n, k in EDGE]
_edge_cache = {}


def edge_case(n, dtype):
    """-> (problem, BlockDiagonal, B of MAX_RHS columns, [twin run per column] at rtol_of(dtype)), computed once per (n, dtype):
    a test with K right-hand sides takes the first K columns"""
    key = (n, np.dtype(dtype).name)
    if key not in _edge_cache:
        p, Dop, rng = edge_problem(n, dtype)
        B = np.asfortranarray(uniform(rng, (n, MAX_RHS), dtype))
        runs = [bicgstab_twin(Dop, B[:, c], None, rtol_of(dtype), 0.0, 200, dtype) for c in range(MAX_RHS)]
        _edge_cache[key] = (p, Dop, B, runs)
    return _edge_cache[key]


def third_iterate_spread(orders=8):
    """The case of the maxiter = 3 test (float64, the layout-edge operator at n = 256, column 0, no preconditioner) ->
    (the twin's run as stored, the largest deviation of its third iterate from itself under `orders` permuted summation
    orders of every form and product, in units of eps max|x|)"""
    _, Dop, B, _ = edge_case(256, np.float64)
    D = Dop.dense()
    a = bicgstab_twin(D, B[:, 0], None, 0.0, 0.0, 3, np.float64)
    worst = 0.0
    for seed in range(orders):
        o = np.random.default_rng(seed).permutation(len(D))
        b = bicgstab_twin(D, B[:, 0], None, 0.0, 0.0, 3, np.float64, order=o)
        worst = max(worst, float(np.max(np.abs(a.x - b.x)) / (np.finfo(np.float64).eps * np.max(np.abs(a.x)))))
    return a, worst


# ---- what the GPU suite accepts (test_gpu_bicgstab.py; the solver table of _lockstep.py) ------------------------------------
def check_columns(info, runs, D, x, B, tols, what):
    """every column: status 0, the twin's count (+-1: the multi-column product rounds differently from one column, the
    twin's count is stable under permuted sums -- test_bicgstab_cpu.py), true residual <= 2 tol evaluated in complex128"""
    x = np.asarray(x).reshape(len(D), -1)
    for c, run in enumerate(runs):
        true = true_residual(D, x[:, c], B[:, c])
        print(f"BICGSTAT {what} column {c}: {info.column_iterations[c]} iterations, twin {run.iterations}, true residual / tol "
              f"{true / tols[c] if tols[c] else 0:.3f}")
        assert run.status == 0, (what, c, "the twin did not converge")
        assert info.column_status[c] == 0, (what, c, info.column_status[c])
        assert abs(int(info.column_iterations[c]) - run.iterations) <= 1, (what, c, info.column_iterations[c], run.iterations)
        assert true <= 2 * tols[c], (what, c, true, tols[c])
    assert info.iterations == max(info.column_iterations) and info.status == 0 and info.columns_converged == len(runs)


def check_products(info, has_m, use_x0=False):
    """the documented counts: two A products per lockstep iteration (one more for the residual of an initial guess), two M
    products per iteration"""
    assert info.a_products == 2 * info.iterations + (1 if use_x0 else 0)
    assert info.m_products == (2 * info.iterations if has_m else 0)


# ---- raw ctypes drivers --------------------------------------------------------------------------------------------------
def raw_bicgstab_create(A, opA, M, opM, code, nrhs_max):
    """bsm_bicgstab_create as C sees it -> (return code, solver pointer); a created solver is destroyed by the caller"""
    from bsm_amd import _lib as L
    out = C.c_void_p()
    rc = L.lib().bsm_bicgstab_create(None if A is None else A._h.ptr, opA, None if M is None else M._h.ptr, opM, code, nrhs_max,
                                     C.byref(out))
    return rc, out


def raw_bicgstab_destroy(ptr):
    from bsm_amd import _lib as L
    return L.lib().bsm_bicgstab_destroy(ptr)


def raw_bicgstab_solve(ptr, nrhs, B, ldb, X, ldx, rtol=1e-8, atol=0.0, maxiter=100, use_x0=0, capacity=None, memspace=1, stream=None,
                       struct_size=None, want_cols=True):
    """bsm_bicgstab_solve as C sees it (B, X: addresses) -> (return code, info, columns, history of `capacity` rows
    prefilled with -1)"""
    from bsm_amd import _lib as L
    cap = maxiter if capacity is None else capacity
    p = L.BsmCgParams(C.sizeof(L.BsmCgParams) if struct_size is None else struct_size, use_x0, rtol, atol, maxiter, cap)
    info = L.BsmCgInfo()
    cols = (L.BsmCgColumn * max(nrhs, 1))() if want_cols else None
    hist = np.full((max(cap, 1), max(nrhs, 1)), -1.0)
    rc = L.lib().bsm_bicgstab_solve(ptr, nrhs, B, ldb, X, ldx, C.byref(p), C.byref(info), cols,
                                    hist.ctypes.data_as(C.POINTER(C.c_double)), memspace, stream)
    return rc, info, cols, hist
