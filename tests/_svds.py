"""What the svds suites (test_svds_cpu.py, test_gpu_svds.py) share: the numpy twin of bsm_svds_solve, the test problems, the
acceptance of a converged device solve (accept) and raw ctypes drivers of bsm_svds_create / _solve / _destroy and of the test
hooks bsm_debug_svds_jacobi / _select / _keep / _cycles.  Test code only.

The twin.  svds_twin is thick-restart Golub-Kahan-Lanczos bidiagonalisation as include/bsm_rocm.h states it: the recurrence
started in the SHORT space (on B = op(A) if m >= n, on op(A)^H otherwise, U and V exchanged on the way out), the same step
order (product, two classical Gram-Schmidt passes, norm, guarded scale, on either side), the projected matrix Bp kept in
double with the analytic arrow entries beta_m X[m - 1, i] after a restart, the same selection and keep rules, anorm = the
largest sigma seen, the same statuses.  Every vector and product is rounded to `dtype`.  Bp is decomposed by
numpy.linalg.svd (LAPACK), not by the library's Jacobi method: it shares no code with the library.

The problem.  600 x 400.  Singular values: LOW = 0.1, 0.4, 0.7, 1.0, 1.3, then 390 values uniform in [2, 3], then HIGH = 4.0,
4.5, 5.1, 5.8, 6.6.  rng = default_rng(3900): the row sets cut(rng, 600), the column sets cut(rng, 400), the bulk, G1 Gaussian
600 x 400, G2 Gaussian 400 x 400 (complex types: real part, then imaginary part, of each), A = Q1 diag(s) Q2^H with Q1, Q2 the
(reduced) Q of qr(G1), qr(G2), rounded to the type; v0 = uniform(-1, 1, 400) from default_rng(1).  A is cut the way
_lsqr.lsqr_problem cuts its A: a 6 x 4 grid of 100 x 100 blocks (vbcrs) or one block per pair of a row set and a column set
(blocksparse).  The reference is numpy.linalg.svd of the matrix AS STORED, widened.

The grid problem (grid_svd_problem).  m x n with krylov_grid(m) = 3 and krylov_grid(n) = 2 (_eigsh.grid_sizes).  Block
diagonal and rectangular, so that the twin and the acceptance need no dense array: the columns are cut into blocks of 8 (the
last one n mod 8), the rows dealt out evenly to them (_lsqr.tall_problem's layout); the designed singular values -- LOW, a
bulk uniform in [2, 3], HIGH20 = 4.0 + 0.4 i, i < 20 -- are dealt to the columns by a random permutation, block j is Q1_j
diag(s_j) Q2_j^H rounded to the type; the reference spectrum is svd of the blocks as stored, widened, block by block."""
import ctypes as C

import numpy as np

from _eigsh import combine_reference, grid_sizes, keep_of
from _jacobi import CODE  # noqa: F401
from _krylov import ERR_DEVICE, ERR_INVALID, ERR_UNSUPPORTED, real_of, wide_of  # noqa: F401
from _lsqr import BlockTall, Dense, _as_op
from _submat import cut

M600, N400 = 600, 400
MAX_NCV = 128  # BSM_GMRES_MAX_RESTART
LM, SM = 0, 1
WHICH = {"LM": LM, "SM": SM}
LOW = np.array([0.1, 0.4, 0.7, 1.0, 1.3])
HIGH = np.array([4.0, 4.5, 5.1, 5.8, 6.6])
HIGH20 = 4.0 + 0.4 * np.arange(20)
DTYPES = [np.float32, np.float64, np.complex64, np.complex128]
# (nsv, ncv) per `which`; SM with (1, 3) does not converge in 300 cycles: it is the status-1 case only
CASES = {"LM": [(4, 20), (5, 12), (1, 3), (4, 128)], "SM": [(4, 20), (5, 12), (4, 128)]}
SIDES = ("A", "adjoint")


def is_complex(dtype):
    return np.dtype(dtype).kind == "c"


def svd_rtol(dtype):
    return 2e-5 if np.finfo(dtype).eps > 1e-10 else 1e-10


def select(which, d, count):
    """the `count` of d DESCENDING values that `which` wants, in the order it reports them (0-based indices)"""
    count = min(count, d)
    return list(range(count)) if WHICH.get(which, which) == LM else [d - 1 - i for i in range(count)]


def steps_of(nsv, ncv, cycles):
    return ncv + (cycles - 1) * (ncv - keep_of(nsv, ncv))


# ---- the problems -------------------------------------------------------------------------------------------------------------
_problems, _refs, _grid = {}, {}, {}


def gaussian(rng, shape, dtype):
    G = rng.standard_normal(shape)
    return G + 1j * rng.standard_normal(shape) if is_complex(dtype) else G


def svd_dense(dtype):
    """-> (A of `dtype` (600 x 400), row sets, column sets, s as designed (ascending), v0); computed once, not to be written to"""
    key = np.dtype(dtype).name
    if key not in _problems:
        rng = np.random.default_rng(3900)
        rsets, csets = cut(rng, M600), cut(rng, N400)
        s = np.concatenate([LOW, np.sort(rng.uniform(2, 3, N400 - 10)), HIGH])
        Q1, _ = np.linalg.qr(gaussian(rng, (M600, N400), dtype))
        Q2, _ = np.linalg.qr(gaussian(rng, (N400, N400), dtype))
        A = ((Q1 * s) @ Q2.conj().T).astype(dtype)
        v0 = np.random.default_rng(1).uniform(-1, 1, N400).astype(dtype)
        _problems[key] = (A, rsets, csets, s, v0)
    return _problems[key]


def cut_rect(kind, A, rsets, csets):
    """the dense A as a constructor dictionary of `kind` (the cuts of _lsqr.lsqr_problem)"""
    m, n = A.shape
    if kind == "vbcrs":
        blocks, rs, cs = [], [], []
        for a in range(0, m, 100):
            for b in range(0, n, 100):
                blocks.append(np.asfortranarray(A[a:a + 100, b:b + 100]))
                rs.append(a + 1)
                cs.append(b + 1)
        return dict(kind="vbcrs", blocks=blocks, rowstart=np.array(rs, np.int64), colstart=np.array(cs, np.int64), size=(m, n))
    assert kind == "blocksparse"
    blocks, ri, ci = [], [], []
    for a in rsets:
        for b in csets:
            blocks.append(np.asfortranarray(A[np.ix_(a - 1, b - 1)]))
            ri.append(a)
            ci.append(b)
    return dict(kind="blocksparse", blocks=blocks, rowindices=ri, colindices=ci, size=(m, n))


def svd_problem(kind, dtype):
    """-> (problem, A, v0)"""
    A, rsets, csets, _, v0 = svd_dense(dtype)
    return cut_rect(kind, A, rsets, csets), A, v0


def side_of(A, side):
    """the operator a solve on A ("A") or on adjoint(A) / transpose(A) of a real A ("adjoint") sees, for the twin"""
    return Dense(A) if side == "A" else Dense(A).H


def stored_singular_values(op):
    """svd of the operator AS STORED (the type's values, widened), DESCENDING, min(m, n) values; cached by identity of op"""
    key = id(op)
    if key not in _refs:
        op_ = _as_op(op)
        wide = wide_of(op_.dtype)
        if isinstance(op_, BlockTall):
            s = np.sort(np.concatenate([np.linalg.svd(S.astype(wide), compute_uv=False).ravel() for _, _, S in op_.groups]))[::-1]
        else:
            s = np.linalg.svd(op_.dense().astype(wide), compute_uv=False)
        _refs[key] = (op, s)
    return _refs[key][1]


def grid_svd_problem(dtype):
    """-> (vbcrs problem, BlockTall of size (m, n), v0 of n entries) (module docstring); computed once, not to be written to"""
    dtype = np.dtype(dtype)
    if dtype.name not in _grid:
        n, m = grid_sizes(dtype)
        rng = np.random.default_rng(4300 + m + n)
        bs = 8
        widths = [bs] * (n // bs) + ([n % bs] if n % bs else [])
        nb = len(widths)
        heights = [m // nb + (1 if j < m % nb else 0) for j in range(nb)]
        assert min(heights) >= bs
        r0 = np.concatenate([[0], np.cumsum(heights)[:-1]]).astype(np.int64)
        c0 = np.concatenate([[0], np.cumsum(widths)[:-1]]).astype(np.int64)
        s = np.concatenate([LOW, rng.uniform(2, 3, n - len(LOW) - len(HIGH20)), HIGH20])[rng.permutation(n)]
        groups, blocks = [], [None] * nb
        for h, w in sorted(set(zip(heights, widths))):
            idx = np.array([j for j in range(nb) if (heights[j], widths[j]) == (h, w)])
            Q1, _ = np.linalg.qr(gaussian(rng, (len(idx), h, w), dtype))
            Q2, _ = np.linalg.qr(gaussian(rng, (len(idx), w, w), dtype))
            sj = np.stack([s[c0[j]:c0[j] + w] for j in idx])
            S = ((Q1 * sj[:, None, :]) @ np.conj(np.swapaxes(Q2, 1, 2))).astype(dtype)
            groups.append((r0[idx], c0[idx], S))
            for k, j in enumerate(idx):
                blocks[j] = np.asfortranarray(S[k])
        p = dict(kind="vbcrs", blocks=blocks, rowstart=r0 + 1, colstart=c0 + 1, size=(m, n))
        _grid[dtype.name] = (p, BlockTall((m, n), groups), rng.uniform(-1, 1, n).astype(dtype))
    return _grid[dtype.name]


def diagonal_problem(dtype, d):
    """-> (vbcrs problem of order len(d), D): diag(d) as one block; every product of the recurrence from e_1 is exact"""
    D = np.diag(np.asarray(d, dtype=float)).astype(dtype)
    n = len(D)
    return dict(kind="vbcrs", blocks=[np.asfortranarray(D)], rowstart=np.array([1], np.int64), colstart=np.array([1], np.int64), size=(n, n)), D


def bordered_problem(dtype):
    """-> (vbcrs problem of order 12, D): an 11 x 11 block of full rank over rows and columns 1 .. 11; row 12 and column 12 lie in
    no block: sigma_min = 0 with u = v = e_12"""
    rng = np.random.default_rng(12)
    Q1, _ = np.linalg.qr(gaussian(rng, (11, 11), dtype))
    Q2, _ = np.linalg.qr(gaussian(rng, (11, 11), dtype))
    D = np.zeros((12, 12), dtype)
    D[:11, :11] = ((Q1 * np.linspace(1, 3, 11)) @ Q2.conj().T).astype(dtype)
    p = dict(kind="vbcrs", blocks=[np.asfortranarray(D[:11, :11])], rowstart=np.array([1], np.int64), colstart=np.array([1], np.int64), size=(12, 12))
    return p, D


# ---- the twin -----------------------------------------------------------------------------------------------------------------
class SvdTwin:
    pass


def apply_columns(f, M):
    """f column by column on the matrix M"""
    return np.stack([f(M[:, c]) for c in range(M.shape[1])], axis=1)


def svds_twin(A, v0, nsv, ncv, which, rtol, atol=0.0, maxcycles=300, dtype=None):
    """numpy twin of bsm_svds_solve (module docstring).  A: dense (m x n) array, Dense or BlockTall -> SvdTwin: status, nconv,
    cycles, steps, anorm, value, estimate, residual_av, residual_ahu (in `dtype` arithmetic, norms in double), U (m x nconv), V
    (n x nconv), orth = max(max |U^H U - I|, max |V^H V - I|), first = (alpha, beta) of the first cycle"""
    op = _as_op(A)
    dtype = np.dtype(op.dtype if dtype is None else dtype)
    real = real_of(dtype)
    which = WHICH.get(which, which)
    op = op.astype(dtype)
    m, n = op.shape
    tall = m >= n
    fwd, bwd = (op.times, op.adj) if tall else (op.adj, op.times)  # B and B^H
    l, s = max(m, n), min(m, n)
    assert 1 <= nsv and nsv + 2 <= ncv <= s
    P, Q = np.zeros((s, ncv + 1), dtype), np.zeros((l, ncv), dtype)
    out = SvdTwin()
    out.status, out.nconv, out.cycles, out.steps, out.anorm = None, 0, 0, 0, 0.0
    out.value = out.estimate = out.residual_av = out.residual_ahu = np.zeros(0)
    out.U, out.V, out.orth = np.zeros((m, 0), dtype), np.zeros((n, 0), dtype), 0.0

    def norm(v):
        return real.type(np.linalg.norm(v))

    def scaled(w, b):
        if not (b > 0 and np.isfinite(b)):
            return np.zeros_like(w)
        return (w * real.type(1 / b)).astype(dtype)

    def orth(W, k, w):
        for _ in range(2):
            if k:
                h = (W[:, :k].conj().T @ w).astype(dtype)
                w = (w - W[:, :k] @ h).astype(dtype)
        return w

    with np.errstate(all="ignore"):
        v0 = np.asarray(v0).astype(dtype)
        b0 = norm(v0)
        P[:, 0] = scaled(v0, b0)
        start, kept, arrow = 0, np.zeros(0), np.zeros(0)
        alpha, beta = np.zeros(ncv), np.zeros(ncv)
        idx, beta_m, sig, X, Y, d = [], 0.0, np.zeros(0), np.zeros((0, 0)), np.zeros((0, 0)), 0
        while True:
            out.cycles += 1
            for j in range(start, ncv):
                q = orth(Q, j, fwd(P[:, j]).astype(dtype))
                alpha[j] = float(norm(q))
                Q[:, j] = scaled(q, real.type(alpha[j]))
                r = orth(P, j + 1, bwd(Q[:, j]).astype(dtype))
                beta[j] = float(norm(r))
                P[:, j + 1] = scaled(r, real.type(beta[j]))
                out.steps += 1
            if out.cycles == 1:
                out.first = (alpha.copy(), beta.copy())  # what the library's bookkeeping is fed in test_svds_cpu.py
            if not np.isfinite(b0):
                out.status = 2
                break
            if b0 == 0:
                out.status, d = 3, 0
                break
            d = ncv
            for j in range(start, ncv):
                if beta[j] == 0:
                    d = j + 1
                    break
            if not (np.all(np.isfinite(alpha[start:d])) and np.all(np.isfinite(beta[start:d]))):
                out.status = 2
                break
            Bp = np.zeros((d, d))
            for i in range(start):
                Bp[i, i] = kept[i]
                Bp[i, start] = arrow[i]
            for j in range(start, d):
                Bp[j, j] = alpha[j]
                if j + 1 < d:
                    Bp[j, j + 1] = beta[j]
            X, sig, Yt = np.linalg.svd(Bp)
            Y = Yt.T
            if not np.all(np.isfinite(sig)):
                out.status = 2
                break
            out.anorm = max(out.anorm, float(np.max(sig)))
            beta_m = beta[d - 1]
            if d < ncv:
                out.nconv = min(nsv, d)
                out.status = 0 if d >= nsv else 3
                idx = select(which, d, out.nconv)
                break
            idx = select(which, d, nsv)
            tol = max(rtol * out.anorm, atol)
            done = all(abs(beta_m * X[d - 1, i]) <= tol for i in idx)
            if done or out.cycles >= maxcycles:
                out.status, out.nconv = (0 if done else 1), nsv
                break
            keep = keep_of(nsv, ncv)
            idx = select(which, d, keep)
            carried = P[:, ncv].copy()
            P[:, :keep] = combine_reference(P[:, :ncv], Y[:, idx].astype(real), dtype)
            P[:, keep] = carried
            Q[:, :keep] = combine_reference(Q[:, :ncv], X[:, idx].astype(real), dtype)
            kept, arrow, start = sig[idx], beta_m * X[d - 1, idx], keep
        if out.nconv:
            out.value = sig[idx]
            out.estimate = np.abs(beta_m * X[d - 1, idx])
            right = combine_reference(P[:, :d], Y[:, idx].astype(real), dtype)
            left = combine_reference(Q[:, :d], X[:, idx].astype(real), dtype)
            right = np.stack([scaled(right[:, c], norm(right[:, c])) for c in range(out.nconv)], axis=1)
            left = np.stack([scaled(left[:, c], norm(left[:, c])) for c in range(out.nconv)], axis=1)
            out.U, out.V = (left, right) if tall else (right, left)
            wide = wide_of(dtype)
            sg = out.value.astype(real)
            Rav = apply_columns(op.times, out.V).astype(dtype) - (out.U * sg).astype(dtype)
            Rahu = apply_columns(op.adj, out.U).astype(dtype) - (out.V * sg).astype(dtype)
            out.residual_av = np.linalg.norm(Rav.astype(wide), axis=0)
            out.residual_ahu = np.linalg.norm(Rahu.astype(wide), axis=0)
            Uw, Vw = out.U.astype(wide), out.V.astype(wide)
            eye = np.eye(out.nconv)
            out.orth = float(max(np.max(np.abs(Uw.conj().T @ Uw - eye)), np.max(np.abs(Vw.conj().T @ Vw - eye))))
    return out


_twins = {}


def twin_of(dtype, side, nsv, ncv, which, maxcycles=300):
    """the twin on the 600 x 400 problem of `dtype` (side "A") or on its adjoint at svd_rtol(dtype) from the problem's v0;
    computed once"""
    key = (np.dtype(dtype).name, side, nsv, ncv, which, maxcycles)
    if key not in _twins:
        A, _, _, _, v0 = svd_dense(dtype)
        _twins[key] = svds_twin(side_of(A, side), v0, nsv, ncv, which, svd_rtol(dtype), 0.0, maxcycles, dtype)
    return _twins[key]


# ---- what both suites accept ----------------------------------------------------------------------------------------------
def wanted_reference(ref, which, count):
    """the `count` values of the DESCENDING reference spectrum `which` wants, in its order"""
    return ref[select(which, len(ref), count)]


def check_triplets(value, estimate, r_av, r_ahu, anorm, ref, which, shape, ncv, dtype, what):
    """per triplet: |sigma_i - s_i| <= sqrt((r_av^2 + r_ahu^2) / 2) + max(m, n) eps anorm -- the Hermitian residual bound on [[0, A],
    [A^H, 0]] with the vector [u; v] / sqrt(2), plus the backward error of the dense reference -- and |hypot(r_av, r_ahu) -
    estimate| <= 2 (max(m, n) + ncv + 2) eps anorm, the argument of _eigsh.accept's gap bound applied on both sides (forming
    U = Q X and V = P Y, and the two products).  -> the largest gap / (eps anorm)"""
    eps = float(np.finfo(dtype).eps)
    big = max(shape)
    s = wanted_reference(ref, which, len(value))
    gap = 0.0
    for i in range(len(value)):
        err, bound = abs(value[i] - s[i]), float(np.sqrt((r_av[i] ** 2 + r_ahu[i] ** 2) / 2)) + big * eps * anorm
        g = abs(float(np.hypot(r_av[i], r_ahu[i])) - estimate[i]) / (eps * anorm)
        gap = max(gap, g)
        print(f"SVDSTAT {what} triplet {i}: sigma {value[i]:.12f} ref {s[i]:.12f} |sigma - ref| {err:.3e} bound {bound:.3e} "
              f"r_av {r_av[i]:.3e} r_ahu {r_ahu[i]:.3e} estimate {estimate[i]:.3e} gap / (eps anorm) {g:.2f}")
        assert err <= bound, (what, i, err, bound)
    gap_bound = 2 * (big + ncv + 2)
    assert gap <= gap_bound, (what, gap, gap_bound)
    return gap


def accept(s, U, V, info, op, twin, nsv, ncv, which, dtype, what, ref=None, rtol=None):
    """the acceptance of a converged device solve (docstring of test_gpu_svds.py).  op: the operator the solve saw (m x n), a dense
    array, Dense or BlockTall; U, V: torch tensors or numpy arrays"""
    from _gpu import TOL
    dtype = np.dtype(dtype)
    eps = float(np.finfo(dtype).eps)
    wide = wide_of(dtype)
    op = _as_op(op)
    m, n = op.shape
    ref = stored_singular_values(op) if ref is None else ref
    assert twin.status == 0, (what, "the twin did not converge")
    assert info.status == 0 and info.nconv == nsv == len(s), (what, info)
    tol = (svd_rtol(dtype) if rtol is None else rtol) * info.anorm
    assert np.all(info.estimate <= tol), (what, info.estimate, tol)
    check_triplets(s, info.estimate, info.residual_av, info.residual_ahu, info.anorm, ref, which, (m, n), ncv, dtype, what)
    Uh = (U if isinstance(U, np.ndarray) else U.cpu().numpy()).astype(wide)
    Vh = (V if isinstance(V, np.ndarray) else V.cpu().numpy()).astype(wide)
    assert Uh.shape == (m, nsv) and Vh.shape == (n, nsv)
    opw = op.astype(wide)
    true_av = np.linalg.norm(apply_columns(opw.times, Vh) - Uh * s, axis=0)
    true_ahu = np.linalg.norm(apply_columns(opw.adj, Uh) - Vh * s, axis=0)
    print(f"SVDSTAT {what}: max |true - reported| / anorm: av {np.max(np.abs(true_av - info.residual_av)) / info.anorm:.3e}, ahu "
          f"{np.max(np.abs(true_ahu - info.residual_ahu)) / info.anorm:.3e} of {TOL[dtype]:.0e}; max estimate / tol {np.max(info.estimate) / tol:.3e}")
    assert np.all(np.abs(true_av - info.residual_av) <= TOL[dtype] * info.anorm), (what, true_av, info.residual_av)
    assert np.all(np.abs(true_ahu - info.residual_ahu) <= TOL[dtype] * info.anorm), (what, true_ahu, info.residual_ahu)
    eye = np.eye(nsv)
    orth = float(max(np.max(np.abs(Uh.conj().T @ Uh - eye)), np.max(np.abs(Vh.conj().T @ Vh - eye))))
    print(f"SVDSTAT {what}: cycles {info.cycles} (twin {twin.cycles}), orth / eps {orth / eps:.2f} (twin {twin.orth / eps:.2f}, margin used "
          f"{orth / twin.orth if twin.orth else float('inf'):.2f} of 8), anorm {info.anorm:.6f}, a_products {info.a_products}")
    assert orth <= 8 * twin.orth, (what, orth / eps, twin.orth / eps)
    assert info.cycles <= twin.cycles + 1, (what, info.cycles, twin.cycles)
    assert info.a_products == 2 * steps_of(nsv, ncv, info.cycles) + 2 * nsv, (what, info.a_products)
    assert info.anorm <= float(ref[0]) * (1 + max(m, n) * eps)  # a lower bound of ||A||_2, up to the error of both sides


# ---- raw ctypes drivers --------------------------------------------------------------------------------------------------
def raw_svds_create(A, opA, code, nsv, ncv, null_out=False):
    """bsm_svds_create as C sees it -> (return code, solver pointer); a created solver is destroyed by the caller"""
    from bsm_amd import _lib as L
    out = C.c_void_p(0xdead)
    rc = L.lib().bsm_svds_create(None if A is None else A._h.ptr, opA, code, nsv, ncv, None if null_out else C.byref(out))
    return rc, out


def raw_svds_destroy(ptr):
    from bsm_amd import _lib as L
    return L.lib().bsm_svds_destroy(ptr)


def raw_svds_solve(ptr, nsv, v0, U, ldu, V, ldv, which=LM, rtol=1e-10, atol=0.0, maxcycles=300, vectors=1, memspace=1, stream=None,
                   struct_size=None, null=()):
    """bsm_svds_solve as C sees it (v0, U, V: addresses) -> (return code, info, triplets); null: names of p / info / triplets to
    pass as NULL"""
    from bsm_amd import _lib as L
    p = L.BsmSvdsParams(C.sizeof(L.BsmSvdsParams) if struct_size is None else struct_size, which, rtol, atol, maxcycles, vectors)
    info = L.BsmSvdsInfo()
    trip = (L.BsmSvdsTriplet * max(nsv, 1))()
    rc = L.lib().bsm_svds_solve(ptr, v0, U, ldu, V, ldv, None if "p" in null else C.byref(p), None if "info" in null else C.byref(info),
                                None if "triplets" in null else trip, memspace, stream)
    return rc, info, trip


def raw_svd_jacobi(B):
    """the unexported test hook bsm_debug_svds_jacobi (csrc/bsm_svds.cpp) -> (sigma descending, X, Y, sweeps)"""
    from bsm_amd import _lib as L
    fn = L.lib().bsm_debug_svds_jacobi
    dp = C.POINTER(C.c_double)
    fn.argtypes = [C.c_int32, dp, C.c_int64, dp, dp, dp, C.POINTER(C.c_int32)]
    fn.restype = C.c_int
    B = np.asfortranarray(B, dtype=np.float64)
    m = len(B)
    sigma, X, Y, sw = np.zeros(m), np.zeros((m, m), order="F"), np.zeros((m, m), order="F"), C.c_int32(-1)
    rc = fn(m, B.ctypes.data_as(dp), m, sigma.ctypes.data_as(dp), X.ctypes.data_as(dp), Y.ctypes.data_as(dp), C.byref(sw))
    assert rc == 0
    return sigma, X, Y, sw.value


def raw_select(which, m, count):
    """the unexported test hook bsm_debug_svds_select -> 0-based indices"""
    from bsm_amd import _lib as L
    fn = L.lib().bsm_debug_svds_select
    fn.argtypes = [C.c_int, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]
    fn.restype = C.c_int
    idx = np.full(max(count, 1), -1, dtype=np.int32)
    rc = fn(which, m, count, idx.ctypes.data_as(C.POINTER(C.c_int32)))
    assert rc == 0
    return idx[:count].tolist()


def raw_keep(nsv, ncv):
    from bsm_amd import _lib as L
    fn = L.lib().bsm_debug_svds_keep
    fn.argtypes = [C.c_int32, C.c_int32]
    fn.restype = C.c_int
    return fn(nsv, ncv)


def raw_cycles(which, nsv, ncv, alpha, beta):
    """the unexported test hook bsm_debug_svds_cycles: the library's bookkeeping of the projected matrix over the cycles whose
    alpha / beta are the rows of the two (cycles x ncv) arrays -> (d, sigma, estimate, kept, arrow) of the last one"""
    from bsm_amd import _lib as L
    fn = L.lib().bsm_debug_svds_cycles
    dp = C.POINTER(C.c_double)
    fn.argtypes = [C.c_int, C.c_int32, C.c_int32, C.c_int32, dp, dp, C.POINTER(C.c_int32), dp, dp, dp, dp]
    fn.restype = C.c_int
    alpha, beta = np.ascontiguousarray(alpha, dtype=np.float64), np.ascontiguousarray(beta, dtype=np.float64)
    cycles = alpha.shape[0]
    d = C.c_int32(-7)
    sigma, est, kept, arrow = np.zeros(ncv), np.zeros(ncv), np.zeros(ncv), np.zeros(ncv)
    rc = fn(which, nsv, ncv, cycles, alpha.ctypes.data_as(dp), beta.ctypes.data_as(dp), C.byref(d), sigma.ctypes.data_as(dp),
            est.ctypes.data_as(dp), kept.ctypes.data_as(dp), arrow.ctypes.data_as(dp))
    assert rc == 0
    k = keep_of(nsv, ncv) if cycles > 1 else 0
    return d.value, sigma[:max(d.value, 0)], est[:max(d.value, 0)], kept[:k], arrow[:k]
