"""What the CG suites (test_cg_cpu.py, test_gpu_cg.py) share: the numpy twin of bsm_cg_solve, the test problems and raw
ctypes drivers of bsm_cg_create / _solve / _destroy.  Test code only.

The twin.  cg_twin is preconditioned CG (conj=True: <u, v> = sum conj(u) v) / COCG (conj=False: sum u v) as
include/bsm_rocm.h states the recurrences, every array, product and scalar rounded to `dtype`, with the four statuses of a
column (0 converged, 1 maxiter, 2 a non-finite residual norm, 3 breakdown: <p, A p> == 0 or <r, z> == 0 on a column that
has not converged).  It shares no code with the library.

The problems.  Order 400, rng = default_rng(4000), sets = _submat.cut(rng, 400).  G uniform in (-1, 1) (both parts for
complex types), S = (G + G^T) / 2 (Hermitian variant: (G + G^H) / 2), D0 = S + s I with s = 24 (real) / 36 (complex),
D = W D0 W with W diagonal, constant on each set, 2**k with k = rng.integers(-3, 4) per set (exact in binary floating
point: D is symmetric to the bit); B (400 x 5) uniform.  D is cut into a 4 x 4 grid of 100 x 100 blocks (vbcrs), one block
per pair of sets (blocksparse), or D[I_s, I_s] as diagonals and D[I_a, I_b], a > b, as off-diagonals (symmetric: not for
the Hermitian variant, whose mirrored blocks would have to be conjugated).  M = block_jacobi(A, sets); the twin takes the
exact block inverse."""
import ctypes as C

import numpy as np

from _jacobi import CODE, KINDS, dense_of, set_blocks, uniform
from _krylov import ERR_DEVICE, ERR_INVALID, ERR_UNSUPPORTED, exact_minv, real_of, rtol_of, true_residual, wide_of  # noqa: F401
from _submat import cut

NCG = 400
NB = 5
MAX_RHS = 16  # BSM_CG_MAX_RHS
CG, COCG = 0, 1
METHOD = {True: "cg", False: "cocg"}


def is_complex(dtype):
    return np.dtype(dtype).kind == "c"


def cg_problem(kind, dtype, herm=False):
    """-> (problem, sets, D, B): the operator as a constructor dictionary, its index sets, its dense form and the
    right-hand sides.  herm: the Hermitian variant (complex types, vbcrs / blocksparse only)"""
    assert not (herm and kind == "symmetric")
    rng = np.random.default_rng(4000)
    sets = cut(rng, NCG)
    G = uniform(rng, (NCG, NCG), dtype)
    S = ((G + (G.conj().T if herm else G.T)) / 2).astype(dtype)
    D0 = S + dtype(36 if is_complex(dtype) else 24) * np.eye(NCG, dtype=dtype)
    w = np.ones(NCG)
    for s in sets:
        w[s - 1] = 2.0 ** int(rng.integers(-3, 4))
    D = (w[:, None] * D0 * w[None, :]).astype(dtype)
    B = np.asfortranarray(uniform(rng, (NCG, NB), dtype))
    if kind == "vbcrs":
        blocks, rs, cs = [], [], []
        for a in range(0, NCG, 100):
            for b in range(0, NCG, 100):
                blocks.append(np.asfortranarray(D[a:a + 100, b:b + 100]))
                rs.append(a + 1)
                cs.append(b + 1)
        p = dict(kind="vbcrs", blocks=blocks, rowstart=np.array(rs, np.int64), colstart=np.array(cs, np.int64), size=(NCG, NCG))
    elif kind == "blocksparse":
        blocks, ri, ci = [], [], []
        for a in sets:
            for b in sets:
                blocks.append(np.asfortranarray(D[np.ix_(a - 1, b - 1)]))
                ri.append(a)
                ci.append(b)
        p = dict(kind="blocksparse", blocks=blocks, rowindices=ri, colindices=ci, size=(NCG, NCG))
    else:
        offs, ri, ci = [], [], []
        for a in range(len(sets)):
            for b in range(a):
                offs.append(np.asfortranarray(D[np.ix_(sets[a] - 1, sets[b] - 1)]))
                ri.append(sets[a])
                ci.append(sets[b])
        p = dict(kind="symmetric", diagonals=set_blocks(D, sets), diagonalindices=list(sets), offdiagonals=offs, rowindices=ri,
                 colindices=ci, size=(NCG, NCG))
    return p, sets, D, B


class BlockDiagonal:
    """diag(blocks) as the twin's operator where a dense array would not fit: nb blocks of order bs and one of the rest"""

    def __init__(self, main, tail):
        self.main, self.tail = main, tail  # (nb, bs, bs), (t, t)

    def astype(self, dtype):
        return BlockDiagonal(self.main.astype(dtype), self.tail.astype(dtype))

    def __matmul__(self, v):
        return self.times(v)

    def times(self, v, order=None):
        """diag(blocks) v.  order: a permutation of the rows; the ranks of its first bs (tail: t) entries are the order the
        columns of every block are summed in (None: as stored)"""
        nb, bs, _ = self.main.shape
        t = self.tail.shape[0]
        out = np.empty_like(v)
        if order is None:
            out[:nb * bs] = np.einsum("bij,bj->bi", self.main, v[:nb * bs].reshape(nb, bs)).ravel()
            out[nb * bs:] = self.tail @ v[nb * bs:]
            return out
        q, qt = np.argsort(order[:bs]), np.argsort(order[:t])
        out[:nb * bs] = np.einsum("bij,bj->bi", np.ascontiguousarray(self.main[:, :, q]),
                                  np.ascontiguousarray(v[:nb * bs].reshape(nb, bs)[:, q])).ravel()
        out[nb * bs:] = np.ascontiguousarray(self.tail[:, qt]) @ v[nb * bs:][qt]
        return out

    def dense(self):
        nb, bs, _ = self.main.shape
        n = nb * bs + self.tail.shape[0]
        D = np.zeros((n, n), self.main.dtype)
        for b in range(nb):
            D[b * bs:(b + 1) * bs, b * bs:(b + 1) * bs] = self.main[b]
        D[nb * bs:, nb * bs:] = self.tail
        return D


def spd_problem(rng, n, dtype, bs=8):
    """-> (vbcrs problem, BlockDiagonal): diagonal blocks T^H T + I of order bs (the last one n mod bs), T uniform"""
    nb, t = n // bs, n % bs
    T = uniform(rng, (nb, bs, bs), dtype)
    main = (np.einsum("bki,bkj->bij", T.conj(), T) + np.eye(bs, dtype=dtype)).astype(dtype)
    Tt = uniform(rng, (t, t), dtype)
    tail = (Tt.conj().T @ Tt + np.eye(t, dtype=dtype)).astype(dtype)
    # (the products above round: symmetrise to the bit)
    main = ((main + main.conj().transpose(0, 2, 1)) / 2).astype(dtype)
    tail = ((tail + tail.conj().T) / 2).astype(dtype)
    blocks = [np.asfortranarray(main[b]) for b in range(nb)] + ([np.asfortranarray(tail)] if t else [])
    starts = np.arange(len(blocks), dtype=np.int64) * bs + 1
    return dict(kind="vbcrs", blocks=blocks, rowstart=starts, colstart=starts.copy(), size=(n, n)), BlockDiagonal(main, tail)


class CgTwin:
    def __init__(self, x, history, status, bnorm, iterates):
        self.x, self.history, self.status, self.bnorm = x, np.array(history, dtype=np.float64), status, bnorm
        self.iterations = len(history)
        self.iterates = iterates  # x after every iteration
        self.residual = history[-1] if history else None


def cg_twin(D, b, Minv, conj, rtol, atol, maxiter, dtype, x0=None, order=None, keep=None):
    """numpy twin of one column of bsm_cg_solve (module docstring) -> CgTwin.  D: dense array or BlockDiagonal; Minv:
    dense preconditioner or None; order: a permutation the sums of the forms, of the norms and of the products with D run
    in (None: as stored; a BlockDiagonal permutes inside its blocks); keep: a MUTATION for the tests of the tests -- the
    forms <p, q> and <r, z> sum their first `keep` terms only, as a kernel that loses the last workgroup's share would
    (None: all; not together with order)"""
    dtype = np.dtype(dtype)
    real = real_of(dtype)
    D = D.astype(dtype)
    Minv = None if Minv is None else np.asarray(Minv).astype(dtype)
    b = np.asarray(b).astype(dtype)
    n = len(b)
    perm = np.arange(n) if order is None else order

    assert order is None or keep is None

    def form(u, v):
        terms = ((np.conj(u) if conj else u) * v).astype(dtype)
        return np.sum(terms[perm] if keep is None else terms[:keep], dtype=dtype)

    def norm(v):
        return float(np.linalg.norm(v if order is None else v[perm]).astype(real))

    def times(v):
        if isinstance(D, BlockDiagonal):
            return D.times(v, order).astype(dtype)
        if order is None:
            return (D @ v).astype(dtype)
        return (np.ascontiguousarray(D[:, perm]) @ v[perm]).astype(dtype)

    def decide(rn, tol):
        return 2 if not np.isfinite(rn) else (0 if rn <= tol else None)

    with np.errstate(all="ignore"):
        x = np.zeros(n, dtype) if x0 is None else np.asarray(x0).astype(dtype)
        r = b.copy() if x0 is None else (b - times(x)).astype(dtype)
        bnorm = norm(b)
        tol = max(rtol * bnorm, atol)
        rn0 = norm(r)
        status = decide(rn0, tol)
        hist, its = [], []
        z = r if Minv is None else (Minv @ r).astype(dtype)
        p = z.copy()
        rz = form(r, z)
        while status is None:
            if len(hist) >= maxiter:
                status = 1
                break
            q = times(p)
            pq = form(p, q)
            if pq == 0 or rz == 0:
                status = 3
                break
            alpha = dtype.type(rz / pq)
            x = (x + alpha * p).astype(dtype)
            r = (r - alpha * q).astype(dtype)
            rn = norm(r)
            hist.append(rn)
            its.append(x.copy())
            status = decide(rn, tol)
            if status is None:
                z = r if Minv is None else (Minv @ r).astype(dtype)
                rzn = form(r, z)
                p = (z + dtype.type(rzn / rz) * p).astype(dtype)
                rz = rzn
    out = CgTwin(x, hist, status, bnorm, its)
    if not hist:
        out.residual = rn0
    return out


def column_tol(b, rtol, atol=0.0):
    return max(rtol * float(np.linalg.norm(np.asarray(b).astype(np.complex128))), atol)


# ---- what the GPU suite accepts (test_gpu_cg.py; the solver table of _lockstep.py) ------------------------------------------
def check_columns(info, runs, D, x, B, tols, what):
    """every column: status 0, the twin's count (+-1: the multi-column product rounds differently from one column, the
    twin's count is stable under permuted sums -- test_cg_cpu.py), true residual <= 2 tol evaluated in complex128"""
    x = np.asarray(x).reshape(len(D), -1)
    for c, run in enumerate(runs):
        true = true_residual(D, x[:, c], B[:, c])
        print(f"CGSTAT {what} column {c}: {info.column_iterations[c]} iterations, twin {run.iterations}, true residual / tol "
              f"{true / tols[c] if tols[c] else 0:.3f}")
        assert run.status == 0, (what, c, "the twin did not converge")
        assert info.column_status[c] == 0, (what, c, info.column_status[c])
        assert abs(int(info.column_iterations[c]) - run.iterations) <= 1, (what, c, info.column_iterations[c], run.iterations)
        assert true <= 2 * tols[c], (what, c, true, tols[c])
    assert info.iterations == max(info.column_iterations) and info.status == 0 and info.columns_converged == len(runs)


def check_products(info, has_m, use_x0=False):
    """the documented counts: one A product per lockstep iteration (one more for the residual of an initial guess), one
    M product per iteration and one for the first z"""
    assert info.a_products == info.iterations + (1 if use_x0 else 0)
    assert info.m_products == (info.iterations + 1 if has_m else 0)


# ---- raw ctypes drivers --------------------------------------------------------------------------------------------------
def raw_cg_create(A, opA, M, opM, code, nrhs_max, method=CG):
    """bsm_cg_create as C sees it -> (return code, solver pointer); a created solver is destroyed by the caller"""
    from bsm_amd import _lib as L
    out = C.c_void_p()
    rc = L.lib().bsm_cg_create(None if A is None else A._h.ptr, opA, None if M is None else M._h.ptr, opM, code, nrhs_max, method,
                               C.byref(out))
    return rc, out


def raw_cg_destroy(ptr):
    from bsm_amd import _lib as L
    return L.lib().bsm_cg_destroy(ptr)


def raw_cg_solve(ptr, nrhs, B, ldb, X, ldx, rtol=1e-8, atol=0.0, maxiter=100, use_x0=0, capacity=None, memspace=1, stream=None,
                 struct_size=None, want_cols=True):
    """bsm_cg_solve as C sees it (B, X: addresses) -> (return code, info, columns, history of `capacity` rows prefilled
    with -1)"""
    from bsm_amd import _lib as L
    cap = maxiter if capacity is None else capacity
    p = L.BsmCgParams(C.sizeof(L.BsmCgParams) if struct_size is None else struct_size, use_x0, rtol, atol, maxiter, cap)
    info = L.BsmCgInfo()
    cols = (L.BsmCgColumn * max(nrhs, 1))() if want_cols else None
    hist = np.full((max(cap, 1), max(nrhs, 1)), -1.0)
    rc = L.lib().bsm_cg_solve(ptr, nrhs, B, ldb, X, ldx, C.byref(p), C.byref(info), cols, hist.ctypes.data_as(C.POINTER(C.c_double)),
                              memspace, stream)
    return rc, info, cols, hist
