"""What the MINRES suites (test_minres_cpu.py, test_gpu_minres.py) share: the numpy twin of bsm_minres_solve, the indefinite
test problems and raw ctypes drivers of bsm_minres_create / _solve / _destroy.  Test code only.

The twin.  minres_twin is symmetric-preconditioned MINRES as include/bsm_rocm.h states the recurrences -- the forms are the
real parts of sum conj(u) v, every scalar is real, the decision is on the 2-norm of the CARRIED residual --, every array,
product and scalar rounded to `dtype` (scalars to its real type), with the four statuses of a column (0 converged, 1
maxiter, 2 a non-finite residual norm, 3 breakdown: <v, z> not positive at the start, <v_new, z_new> negative or not
finite, a1 not a positive finite number, gamma_new == 0 above the tolerance).  It shares no code with the library.

The problems.
  Order 400 (minres_problem): the ingredients of _cg.cg_problem drawn in its order from rng = default_rng(4000) -- sets =
  cut(rng, 400), G uniform, S = (G + G^T) / 2 (complex types: the Hermitian (G + G^H) / 2), W diagonal and constant on each
  set, B (400 x 5) uniform --, D = W (S + s J) W with J = +1 / -1 constant on each set, alternating by set number, s = 24
  (real) / 36 (complex): symmetric / Hermitian with 190 negative eigenvalues.  The definite sibling P = W (S + s I) W IS
  cg_problem's operator; M = block_jacobi(P, sets) is positive definite, the twin takes its exact block inverse.
  Grid (indef_problem): block diagonal, blocks +-(T^H T + shift I) of order 8 (the last one n mod 8), symmetrised to the
  bit, the sign alternating by block; with the definite sibling (all signs +) for the preconditioner over half_sets(n)."""
import ctypes as C

import numpy as np

from _cg import MAX_RHS, NB, NCG, BlockDiagonal, CgTwin, is_complex
from _jacobi import set_blocks, uniform
from _krylov import real_of, true_residual
from _submat import cut


# the twin's iterations on the five columns of the order-400 problems, M = the exact block inverse of the definite sibling
COUNTS = {"float32": [29] * 5, "float64": [63, 63, 63, 63, 65], "complex64": [28, 28, 28, 28, 27], "complex128": [60] * 5}
# with M = the block inverse of D ITSELF (indefinite): status 3 on every column, after this many iterations
BROKEN_COUNTS = {"float32": [0, 0, 0, 0, 1], "float64": [0, 0, 0, 0, 1], "complex64": [0, 1, 0, 0, 0], "complex128": [0, 1, 0, 0, 0]}


# ---- the twin ---------------------------------------------------------------------------------------------------------------
def minres_twin(D, b, Minv, rtol, atol, maxiter, dtype, x0=None, order=None, keep=None):
    """numpy twin of one column of bsm_minres_solve (module docstring) -> CgTwin.  D: dense array or BlockDiagonal; Minv:
    dense preconditioner or None; order: a permutation the sums of the forms, of the norms and of the products with D and
    with Minv run in (None: as stored; a BlockDiagonal permutes inside its blocks); keep: a MUTATION for the tests of the tests --
    the forms <z, q> and <v_new, z_new> sum their first `keep` terms only, as a kernel that loses the last workgroup's share would
    (None: all; not together with order)"""
    dtype = np.dtype(dtype)
    real = real_of(dtype)
    R = real.type
    D = D.astype(dtype)
    Minv = None if Minv is None else np.asarray(Minv).astype(dtype)
    b = np.asarray(b).astype(dtype)
    n = len(b)
    perm = np.arange(n) if order is None else order
    assert order is None or keep is None
    MinvP = None if Minv is None or order is None else np.ascontiguousarray(Minv[:, perm])

    def form(u, v):
        terms = (np.conj(u) * v).real.astype(real)
        return R(np.sum(terms[perm] if keep is None else terms[:keep], dtype=real))

    def norm(v):
        return float(np.linalg.norm(v if order is None else v[perm]).astype(real))

    def times(v):
        if isinstance(D, BlockDiagonal):
            return D.times(v, order).astype(dtype)
        if order is None:
            return (D @ v).astype(dtype)
        return (np.ascontiguousarray(D[:, perm]) @ v[perm]).astype(dtype)

    def prec(v):
        if Minv is None:
            return v
        return ((Minv @ v) if order is None else (MinvP @ v[perm])).astype(dtype)

    def decide(rn, tol):
        return 2 if not np.isfinite(rn) else (0 if rn <= tol else None)

    with np.errstate(all="ignore"):
        x = np.zeros(n, dtype) if x0 is None else np.asarray(x0).astype(dtype)
        r = b.copy() if x0 is None else (b - times(x)).astype(dtype)
        bnorm = norm(b)
        tol = max(rtol * bnorm, atol)
        rn0 = norm(r)
        status = decide(rn0, tol)
        hist, its, etas = [], [], []
        v, v_old, w, w_old = r.copy(), np.zeros(n, dtype), np.zeros(n, dtype), np.zeros(n, dtype)
        z = prec(v)
        vz = form(v, z)
        pd = bool(vz > 0 and np.isfinite(vz))
        if status is None and not pd:
            status = 3
        gamma = R(np.sqrt(vz)) if pd else R(0)
        gamma_old, eta, s, s_old, c, c_old = R(1), gamma, R(0), R(0), R(1), R(1)
        while status is None:
            if len(hist) >= maxiter:
                status = 1
                break
            q = times(z)
            zq = form(z, q)
            ig = R(R(1) / gamma)
            delta = R(zq / R(gamma * gamma))
            v_new = ((ig * q - R(delta * ig) * v) - R(gamma / gamma_old) * v_old).astype(dtype)
            z_new = prec(v_new)
            vz = form(v_new, z_new)
            if not (vz >= 0) or not np.isfinite(vz):
                status = 3
                break
            gn = R(np.sqrt(vz))
            a0 = R(R(c * delta) - R(R(c_old * s) * gamma))
            a1 = R(np.sqrt(R(R(a0 * a0) + R(gn * gn))))
            if not (a1 > 0) or not np.isfinite(a1):
                status = 3
                break
            a2 = R(R(s * delta) + R(R(c_old * c) * gamma))
            a3 = R(s_old * gamma)
            ia = R(R(1) / a1)
            cn, sn = R(a0 * ia), R(gn * ia)
            w_new = (((ig * z - a3 * w_old) - a2 * w) * ia).astype(dtype)
            x = (x + R(cn * eta) * w_new).astype(dtype)
            en = R(-sn * eta)
            cr = R(0) if gn == 0 else R(R(cn * en) / gn)
            r = (R(sn * sn) * r + cr * v_new).astype(dtype)
            rn = norm(r)
            hist.append(rn)
            its.append(x.copy())
            etas.append(abs(float(en)))
            status = decide(rn, tol)
            if status is None and gn == 0:
                status = 3
            v_old, v, z, w_old, w = v, v_new, z_new, w, w_new
            gamma_old, gamma, eta, c_old, c, s_old, s = gamma, gn, en, c, cn, s, sn
    out = CgTwin(x, hist, status, bnorm, its)
    out.etas = np.array(etas)  # |eta| after every iteration: with M the residual in the M-norm, sqrt<r, M r>
    if not hist:
        out.residual = rn0
    return out


# ---- the problems -----------------------------------------------------------------------------------------------------------
def cut_operator(kind, D, sets):
    """the dense D of order NCG as a constructor dictionary of `kind`: a 4 x 4 grid of 100 x 100 blocks (vbcrs), one block
    per pair of sets (blocksparse), or diagonals D[I_s, I_s] and off-diagonals D[I_a, I_b], a > b (symmetric: real D only)"""
    if kind == "vbcrs":
        blocks, rs, cs = [], [], []
        for a in range(0, NCG, 100):
            for b in range(0, NCG, 100):
                blocks.append(np.asfortranarray(D[a:a + 100, b:b + 100]))
                rs.append(a + 1)
                cs.append(b + 1)
        return dict(kind="vbcrs", blocks=blocks, rowstart=np.array(rs, np.int64), colstart=np.array(cs, np.int64), size=(NCG, NCG))
    if kind == "blocksparse":
        blocks, ri, ci = [], [], []
        for a in sets:
            for b in sets:
                blocks.append(np.asfortranarray(D[np.ix_(a - 1, b - 1)]))
                ri.append(a)
                ci.append(b)
        return dict(kind="blocksparse", blocks=blocks, rowindices=ri, colindices=ci, size=(NCG, NCG))
    assert kind == "symmetric" and not is_complex(D.dtype)
    offs, ri, ci = [], [], []
    for a in range(len(sets)):
        for b in range(a):
            offs.append(np.asfortranarray(D[np.ix_(sets[a] - 1, sets[b] - 1)]))
            ri.append(sets[a])
            ci.append(sets[b])
    return dict(kind="symmetric", diagonals=set_blocks(D, sets), diagonalindices=list(sets), offdiagonals=offs, rowindices=ri,
                colindices=ci, size=(NCG, NCG))


_problems = {}


def minres_problem(kind, dtype):
    """-> (problem of D, problem of the definite sibling P, sets, D, P, B) (module docstring); computed once per (kind,
    dtype) and not to be written to"""
    key = (kind, np.dtype(dtype).name)
    if key in _problems:
        return _problems[key]
    herm = is_complex(dtype)
    rng = np.random.default_rng(4000)
    sets = cut(rng, NCG)
    G = uniform(rng, (NCG, NCG), dtype)
    S = ((G + (G.conj().T if herm else G.T)) / 2).astype(dtype)
    shift = dtype(36 if herm else 24)
    w, J = np.ones(NCG), np.ones(NCG)
    for k, s in enumerate(sets):
        w[s - 1] = 2.0 ** int(rng.integers(-3, 4))
        J[s - 1] = 1.0 if k % 2 == 0 else -1.0
    D = (w[:, None] * (S + shift * np.diag(J).astype(dtype)) * w[None, :]).astype(dtype)
    P = (w[:, None] * (S + shift * np.eye(NCG, dtype=dtype)) * w[None, :]).astype(dtype)
    B = np.asfortranarray(uniform(rng, (NCG, NB), dtype))
    _problems[key] = (cut_operator(kind, D, sets), cut_operator(kind, P, sets), sets, D, P, B)
    return _problems[key]


def indef_problem(rng, n, dtype, bs=8, shift=8):
    """-> (vbcrs problem, BlockDiagonal, vbcrs problem of the definite sibling, its BlockDiagonal): diagonal blocks
    +-(T^H T + shift I) of order bs (the last one n mod bs), T uniform, the sign alternating by block; the sibling has all
    signs +.  (shift = 1 gave the twin 155 .. 242 iterations with counts moving by 2 under permuted sums: not used)"""
    nb, t = n // bs, n % bs
    T = uniform(rng, (nb, bs, bs), dtype)
    main = (np.einsum("bki,bkj->bij", T.conj(), T) + shift * np.eye(bs, dtype=dtype)).astype(dtype)
    Tt = uniform(rng, (t, t), dtype)
    tail = (Tt.conj().T @ Tt + shift * np.eye(t, dtype=dtype)).astype(dtype)
    main = ((main + main.conj().transpose(0, 2, 1)) / 2).astype(dtype)
    tail = ((tail + tail.conj().T) / 2).astype(dtype)
    sign = np.where(np.arange(nb) % 2 == 0, 1, -1).astype(real_of(dtype))
    smain, stail = (main * sign[:, None, None]).astype(dtype), (tail * (1 if nb % 2 == 0 else -1)).astype(dtype)
    starts = np.arange(nb + (1 if t else 0), dtype=np.int64) * bs + 1

    def problem(m, tl):
        blocks = [np.asfortranarray(m[b]) for b in range(nb)] + ([np.asfortranarray(tl)] if t else [])
        return dict(kind="vbcrs", blocks=blocks, rowstart=starts, colstart=starts.copy(), size=(n, n))
    return problem(smain, stail), BlockDiagonal(smain, stail), problem(main, tail), BlockDiagonal(main, tail)


_cases = {}


def indef_case(n, dtype):
    """-> (problem, BlockDiagonal, sibling problem, sibling BlockDiagonal, B of MAX_RHS uniform columns) from rng =
    default_rng(9100 + n), computed once per (n, dtype) and not to be written to"""
    key = (n, np.dtype(dtype).name)
    if key not in _cases:
        rng = np.random.default_rng(9100 + n)
        p, Dop, ps, Dsib = indef_problem(rng, n, dtype)
        _cases[key] = (p, Dop, ps, Dsib, np.asfortranarray(uniform(rng, (n, MAX_RHS), dtype)))
    return _cases[key]


# ---- what the GPU suite accepts (test_gpu_minres.py; the solver table of _lockstep.py) --------------------------------------
def check_columns(info, runs, D, x, B, tols, what):
    """every column: status 0, the twin's count (+-1: the multi-column product rounds differently from one column, the
    twin's count is stable under permuted sums -- test_minres_cpu.py), true residual <= 2 tol evaluated in complex128"""
    x = np.asarray(x).reshape(D.shape[0], -1)
    for c, run in enumerate(runs):
        true = true_residual(D, x[:, c], B[:, c])
        print(f"MRSTAT {what} column {c}: {info.column_iterations[c]} iterations, twin {run.iterations}, true residual / tol "
              f"{true / tols[c] if tols[c] else 0:.3f}")
        assert run.status == 0, (what, c, "the twin did not converge")
        assert info.column_status[c] == 0, (what, c, info.column_status[c])
        assert abs(int(info.column_iterations[c]) - run.iterations) <= 1, (what, c, info.column_iterations[c], run.iterations)
        assert true <= 2 * tols[c], (what, c, true, tols[c])
    assert info.iterations == max(info.column_iterations) and info.status == 0 and info.columns_converged == len(runs)


def check_products(info, has_m, use_x0=False):
    assert info.a_products == info.iterations + (1 if use_x0 else 0)
    assert info.m_products == (info.iterations + 1 if has_m else 0)


# ---- raw ctypes drivers --------------------------------------------------------------------------------------------------
def raw_minres_create(A, opA, M, opM, code, nrhs_max):
    """bsm_minres_create as C sees it -> (return code, solver pointer); a created solver is destroyed by the caller"""
    from bsm_amd import _lib as L
    out = C.c_void_p()
    rc = L.lib().bsm_minres_create(None if A is None else A._h.ptr, opA, None if M is None else M._h.ptr, opM, code, nrhs_max, C.byref(out))
    return rc, out


def raw_minres_destroy(ptr):
    from bsm_amd import _lib as L
    return L.lib().bsm_minres_destroy(ptr)


def raw_minres_solve(ptr, nrhs, B, ldb, X, ldx, rtol=1e-8, atol=0.0, maxiter=100, use_x0=0, capacity=None, memspace=1, stream=None,
                     struct_size=None, want_cols=True):
    """bsm_minres_solve as C sees it (B, X: addresses) -> (return code, info, columns, history of `capacity` rows prefilled
    with -1)"""
    from bsm_amd import _lib as L
    cap = maxiter if capacity is None else capacity
    p = L.BsmCgParams(C.sizeof(L.BsmCgParams) if struct_size is None else struct_size, use_x0, rtol, atol, maxiter, cap)
    info = L.BsmCgInfo()
    cols = (L.BsmCgColumn * max(nrhs, 1))() if want_cols else None
    hist = np.full((max(cap, 1), max(nrhs, 1)), -1.0)
    rc = L.lib().bsm_minres_solve(ptr, nrhs, B, ldb, X, ldx, C.byref(p), C.byref(info), cols, hist.ctypes.data_as(C.POINTER(C.c_double)),
                                  memspace, stream)
    return rc, info, cols, hist
