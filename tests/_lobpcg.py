"""What the LOBPCG suites (test_lobpcg_cpu.py, test_gpu_lobpcg.py) share: the numpy twin of bsm_lobpcg_solve, the test problems,
the acceptance of a device solve (accept) and raw ctypes drivers of bsm_block_gram, bsm_block_combine, bsm_lobpcg_create /
_solve / _destroy and the test hooks bsm_debug_lobpcg_rr / bsm_debug_eig_jacobi_h.  Test code only.

The twin.  lobpcg_twin is the recurrence include/bsm_rocm.h states: the start on X0 alone, then per iteration the residual
block, the preconditioner, the product, ONE Gram matrix of S = [X | P | W] against [S | AS], the decision (live columns,
convergence of the first nev), the Rayleigh-Ritz step on the columns in use (rr_twin) and the two combinations; the iteration
that found the block converged is followed by the carried norms of the X it left, which confirm the convergence or send the
solve on.  Every vector and product is rounded to `dtype`, the Gram matrix is the wide product of the rounded arrays, the
small problems are numpy.linalg.eigh's: it shares no code with the library.

The problems.  The order-400 problem of _eigsh.eig_dense; the multiplicity problem (the same construction from
default_rng(3737) with the spectrum -2, -2, -2, -1, -0.5, 390 values uniform in [1, 2], HIGH); _cg.cg_problem (herm=True for
complex types) with the exact block-Jacobi inverse as M; the grid problems of _eigsh.grid_problem."""
import ctypes as C

import numpy as np

from _cg import BlockDiagonal, cg_problem
from _eigsh import HIGH, LA, NEIG, SA, WHICH, cut_dense, eig_dense, eig_rtol, is_complex, stored_eigenvalues, wanted_reference  # noqa: F401
from _jacobi import CODE  # noqa: F401
from _krylov import ERR_DEVICE, ERR_INVALID, ERR_UNSUPPORTED, exact_minv, real_of, wide_of  # noqa: F401
from _submat import cut

DTYPES = [np.float32, np.float64, np.complex64, np.complex128]
# (which, nev, block) on the order-400 problem
CASES = [("SA", 4, 6), ("LA", 4, 6), ("SA", 5, 5), ("LA", 1, 3), ("SA", 5, 16)]
MULT_CASE = ("SA", 4, 6)
CG_CASE = ("SA", 3, 5)
GRID_CASES = [("SA", 3, 5), ("LA", 5, 7)]
MULT_LOW = np.array([-2.0, -2.0, -2.0, -1.0, -0.5])
X0_SEED = 5


def start_block(n, block, dtype, seed=X0_SEED):
    X0 = np.random.default_rng(seed).uniform(-1, 1, (n, block))
    return np.asfortranarray(X0.astype(dtype))


# ---- the Rayleigh-Ritz step ---------------------------------------------------------------------------------------------------
def rr_twin(GB, GA, use, k, which, tau):
    """the host step of one iteration on wide p x p matrices -> (status, theta (k), C (p x k), drops, max |Ritz value|)"""
    which = WHICH.get(which, which)
    p = len(GB)
    at = np.flatnonzero(use)
    m = len(at)
    if m < k:
        return 3, None, None, 0, 0.0
    B = GB[np.ix_(at, at)]
    A = GA[np.ix_(at, at)]
    B, A = (B + B.conj().T) / 2, (A + A.conj().T) / 2
    if not (np.all(np.isfinite(B)) and np.all(np.isfinite(A))):
        return 2, None, None, 0, 0.0
    bii = np.real(np.diag(B))
    if not np.all(bii > 0):
        return 3, None, None, 0, 0.0
    d = 1 / np.sqrt(bii)
    B, A = B * np.outer(d, d), A * np.outer(d, d)
    lam, Q = np.linalg.eigh(B)
    keep = lam > tau * lam[-1]
    drops = int(m - np.count_nonzero(keep))
    if np.count_nonzero(keep) < k:
        return 3, None, None, drops, 0.0
    Lm = Q[:, keep] / np.sqrt(lam[keep])
    H = Lm.conj().T @ A @ Lm
    mu, Zs = np.linalg.eigh((H + H.conj().T) / 2)
    if not np.all(np.isfinite(mu)):
        return 2, None, None, drops, 0.0
    sel = np.arange(k) if which == SA else len(mu) - 1 - np.arange(k)
    Cm = np.zeros((p, k), GB.dtype)
    Cm[at] = d[:, None] * (Lm @ Zs[:, sel])
    return 0, mu[sel], Cm, drops, float(np.max(np.abs(mu)))


def combine_twin(V, Cm, dtype):
    """V C with the sum over j ascending, every term rounded to `dtype` (the device fuses the multiply-adds: its result differs
    within the bound the GPU test derives)"""
    dtype = np.dtype(dtype)
    Cm = Cm.astype(dtype)
    out = np.zeros((V.shape[0], Cm.shape[1]), dtype)
    for j in range(V.shape[1]):
        out = (out + V[:, j:j + 1] * Cm[j:j + 1, :]).astype(dtype)
    return out


class LobTwin:
    pass


def lobpcg_twin(D, X0, nev, block, which, rtol, atol=0.0, maxiter=200, Minv=None, dtype=None):
    """numpy twin of bsm_lobpcg_solve (module docstring) on a dense array or a BlockDiagonal operator; Minv: a dense array (or
    operator) applied as the preconditioner -> LobTwin: status, iterations, nconv, drops, anorm, a_products, m_products, value,
    carried, history, X (n x nev, unit columns), true (||D x - theta x|| in wide arithmetic), orth = max |X^H X - I|"""
    dtype = np.dtype(D.dtype if dtype is None else dtype)
    real, wide = real_of(dtype), wide_of(dtype)
    eps = float(np.finfo(dtype).eps)
    which = WHICH.get(which, which)
    D = D.astype(dtype) if isinstance(D, BlockDiagonal) else np.asarray(D).astype(dtype)
    n, k = X0.shape[0], block
    p = 3 * k
    tau = 64 * p * eps
    S, AS = np.zeros((n, p), dtype), np.zeros((n, p), dtype)
    out = LobTwin()
    out.status, out.iterations, out.nconv, out.drops, out.anorm, out.a_products, out.m_products = None, 0, 0, 0, 0.0, 0, 0
    out.value = out.carried = out.true = np.full(nev, np.nan)
    out.history, out.X, out.orth = [], None, 0.0
    theta = np.zeros(k)

    def times(Op, V):
        return (Op.times(V) if isinstance(Op, BlockDiagonal) else Op @ V).astype(dtype)

    def gram():
        Sw = S.astype(wide)
        return Sw.conj().T @ Sw, Sw.conj().T @ AS.astype(wide)

    def ritz(use):
        nonlocal theta
        GB, GA = gram()
        st, th, Cm, drops, big = rr_twin(GB, GA, use, k, which, tau)
        out.drops += drops
        if st != 0:
            return st
        theta = th
        out.anorm = max(out.anorm, big)
        CP = Cm.copy()
        CP[:k] = 0
        CC = np.concatenate([Cm, CP], axis=1)
        S[:, :2 * k] = combine_twin(S, CC, dtype)
        AS[:, :2 * k] = combine_twin(AS, CC, dtype)
        return 0

    def resid():
        R = (AS[:, :k] - (S[:, :k] * theta.astype(real)).astype(dtype)).astype(dtype)
        return R, np.linalg.norm(R.astype(wide), axis=0)

    def decide(nrm):
        live = nrm > max(rtol * out.anorm, atol)
        return live, not np.any(live[:nev])

    with np.errstate(all="ignore"):
        S[:, :k] = np.asarray(X0).astype(dtype)
        AS[:, :k] = times(D, S[:, :k])
        out.a_products = 1
        use = np.zeros(p, bool)
        use[:k] = True
        status = ritz(use)
        it, have_p, pending, wlive = 0, False, False, np.zeros(k, bool)
        last = np.full(k, np.nan)
        if status == 0:
            status = None
            while True:
                R, nrm = resid()
                if pending or it >= maxiter:
                    if not np.all(np.isfinite(nrm)):
                        status = 2
                        break
                    _, conv = decide(nrm)
                    if conv or it >= maxiter:
                        out.history.append(nrm[:nev].copy())
                        last, status = nrm, (0 if conv else 1)
                        break
                    pending = False
                if Minv is not None:
                    S[:, 2 * k:] = times(Minv, R)
                    out.m_products += 1
                else:
                    S[:, 2 * k:] = R
                AS[:, 2 * k:] = times(D, S[:, 2 * k:])
                out.a_products += 1
                if not np.all(np.isfinite(nrm)):
                    status = 2
                    break
                out.history.append(nrm[:nev].copy())
                live, pending = decide(nrm)
                use[k:2 * k] = wlive if have_p else False
                use[2 * k:] = live
                st = ritz(use)
                if st != 0:
                    status = st
                    break
                wlive, have_p = live, True
                it += 1
        out.status, out.iterations = status, it
        out.history = np.array(out.history).reshape(-1, nev)
        if status <= 1:
            tol = max(rtol * out.anorm, atol)
            out.value, out.carried = theta[:nev].copy(), last[:nev].copy()
            out.nconv = int(np.count_nonzero(out.carried <= tol))
            X = S[:, :nev].copy()
            X = (X * (1 / np.linalg.norm(X.astype(wide), axis=0)).astype(real)).astype(dtype)
            out.X = X
            out.a_products += 1
            Xw = X.astype(wide)
            DX = D.astype(wide).times(Xw) if isinstance(D, BlockDiagonal) else D.astype(wide) @ Xw
            out.true = np.linalg.norm(DX - Xw * out.value, axis=0)
            out.orth = float(np.max(np.abs(Xw.conj().T @ Xw - np.eye(nev))))
    return out


# ---- the problems -------------------------------------------------------------------------------------------------------------
_mult = {}


def mult_dense(dtype):
    """-> (D, sets, lam): the multiplicity problem (module docstring); computed once, not to be written to"""
    key = np.dtype(dtype).name
    if key not in _mult:
        rng = np.random.default_rng(3737)
        sets = cut(rng, NEIG)
        lam = np.concatenate([MULT_LOW, np.sort(rng.uniform(1, 2, NEIG - 10)), HIGH])
        G = rng.standard_normal((NEIG, NEIG))
        if is_complex(dtype):
            G = G + 1j * rng.standard_normal((NEIG, NEIG))
        Q, _ = np.linalg.qr(G)
        D = (Q * lam) @ Q.conj().T
        _mult[key] = (((D + D.conj().T) / 2).astype(dtype), sets, lam)
    return _mult[key]


_cgp = {}


def cg_dense(dtype):
    """-> (problem (blocksparse), sets, D, Minv): _cg.cg_problem, Hermitian for complex types, with the exact block-Jacobi
    inverse; computed once"""
    key = np.dtype(dtype).name
    if key not in _cgp:
        p, sets, D, _ = cg_problem("blocksparse", np.dtype(dtype).type, herm=is_complex(dtype))
        _cgp[key] = (p, sets, D, exact_minv(D, sets))
    return _cgp[key]


_twins = {}


def twin_of(problem, dtype, which, nev, block, maxiter=200):
    """the twin at eig_rtol(dtype) from start_block; problem: "eig", "mult", "cg" (with the exact block-Jacobi inverse), "cg-plain";
    computed once"""
    key = (problem, np.dtype(dtype).name, which, nev, block, maxiter)
    if key not in _twins:
        Minv = None
        if problem == "eig":
            D = eig_dense(dtype)[0]
        elif problem == "mult":
            D = mult_dense(dtype)[0]
        else:
            _, _, D, Minv = cg_dense(dtype)
            Minv = Minv if problem == "cg" else None
        _twins[key] = lobpcg_twin(D, start_block(len(D), block, dtype), nev, block, which, eig_rtol(dtype), 0.0, maxiter, Minv, dtype)
    return _twins[key]


# ---- what a converged device solve must satisfy -------------------------------------------------------------------------------
def accept(torch, w, X, info, D, twin, nev, block, which, dtype, what, ref=None, rtol=None, has_m=False):
    """the acceptance of the issue.  D: the operator, a dense array or a BlockDiagonal with its spectrum `ref`; X: a torch tensor
    or numpy array.  Status 0 with nconv == nev; every carried residual <= rtol anorm; Kahan's block bound on the values plus
    the backward error of the dense reference; the reported true residual against numpy's; drift and orthogonality within 8 x
    the twin's (the twin's taken as at least 3 block eps); at most twice the twin's iterations; the product counts."""
    from _gpu import TOL
    dtype = np.dtype(dtype)
    eps = float(np.finfo(dtype).eps)
    wide = wide_of(dtype)
    n = len(D) if not isinstance(D, BlockDiagonal) else X.shape[0]
    ref = stored_eigenvalues(D) if ref is None else ref
    assert twin.status == 0, (what, "the twin did not converge", twin.status)
    Xh = (X.cpu().numpy() if hasattr(X, "cpu") else np.asarray(X)).astype(wide)
    Dw = D.astype(wide)
    DX = Dw.times(Xh) if isinstance(D, BlockDiagonal) else Dw @ Xh
    true = np.linalg.norm(DX - Xh * w, axis=0)
    orth = float(np.max(np.abs(Xh.conj().T @ Xh - np.eye(nev))))
    floor = 3 * block * eps
    drift = float(np.max(np.abs(true - info.estimate))) / (eps * info.anorm) if info.status <= 1 else float("nan")
    tdrift = max(float(np.max(np.abs(twin.true - twin.carried))) / (eps * twin.anorm), 3 * block)
    torth = max(twin.orth, floor)
    print(f"LOBSTAT {what}: status {info.status} iterations {info.iterations} (twin {twin.iterations}) drops {info.drops} (twin {twin.drops}) "
          f"a_products {info.a_products} m_products {info.m_products} anorm {info.anorm:.6f} drift / (eps anorm) {drift:.2f} (twin "
          f"{tdrift:.2f}, margin used {drift / tdrift:.2f} of 8) orth / eps {orth / eps:.2f} (twin {torth / eps:.2f}, margin used "
          f"{orth / torth:.2f} of 8) max carried / tol {np.max(info.estimate) / ((eig_rtol(dtype) if rtol is None else rtol) * info.anorm):.3e}")
    assert info.status == 0 and info.nconv == nev == len(w), (what, info)
    tol = (eig_rtol(dtype) if rtol is None else rtol) * info.anorm
    assert np.all(info.estimate <= tol), (what, info.estimate, tol)
    lam = wanted_reference(ref, which, nev)
    bound = np.sqrt(nev) * float(np.max(info.residual)) + n * eps * info.anorm
    for i in range(nev):
        print(f"LOBSTAT {what} pair {i}: theta {w[i]:+.12f} lam {lam[i]:+.12f} |theta - lam| {abs(w[i] - lam[i]):.3e} bound {bound:.3e} "
              f"carried {info.estimate[i]:.3e} true {info.residual[i]:.3e}")
    assert np.all(np.abs(w - lam) <= bound), (what, w, lam, bound)
    assert np.all(np.abs(true - info.residual) <= TOL[dtype] * info.anorm), (what, true, info.residual)
    assert drift <= 8 * tdrift, (what, drift, tdrift)
    assert orth <= 8 * torth, (what, orth / eps, torth / eps)
    assert info.iterations <= 2 * twin.iterations, (what, info.iterations, twin.iterations)
    assert info.a_products == info.iterations + 2 and info.m_products == (info.iterations if has_m else 0), (what, info)
    assert info.history.shape == (info.iterations + 1, nev) and np.array_equal(info.history[-1], info.estimate)
    assert info.anorm <= float(np.max(np.abs(ref))) * (1 + n * eps)


# ---- raw ctypes drivers -------------------------------------------------------------------------------------------------------
def raw_gram(code, n, p, U, ldu, q, W, ldw, G, ldg, work, stream=None):
    from bsm_amd import _lib as L
    return L.lib().bsm_block_gram(code, n, p, U, ldu, q, W, ldw, G, ldg, work, stream)


def raw_block_combine(code, n, p, q, V, ldv, Cm, ldc, Out, ldo, stream=None):
    from bsm_amd import _lib as L
    return L.lib().bsm_block_combine(code, n, p, q, V, ldv, Cm, ldc, Out, ldo, stream)


def raw_lobpcg_create(A, opA, M, opM, code, nev, block, null_out=False):
    """bsm_lobpcg_create as C sees it -> (return code, solver pointer); a created solver is destroyed by the caller"""
    from bsm_amd import _lib as L
    out = C.c_void_p(0xdead)
    rc = L.lib().bsm_lobpcg_create(None if A is None else A._h.ptr, opA, None if M is None else M._h.ptr, opM, code, nev, block,
                                   None if null_out else C.byref(out))
    return rc, out


def raw_lobpcg_destroy(ptr):
    from bsm_amd import _lib as L
    return L.lib().bsm_lobpcg_destroy(ptr)


def raw_lobpcg_solve(ptr, nev, X0, ldx0, X, ldx, which=SA, rtol=1e-10, atol=0.0, maxiter=200, capacity=0, memspace=1, stream=None,
                     struct_size=None, null=(), history=None):
    """bsm_lobpcg_solve as C sees it (X0, X: addresses) -> (return code, info, pairs); null: names of p / info / pairs to pass as
    NULL"""
    from bsm_amd import _lib as L
    p = L.BsmLobpcgParams(C.sizeof(L.BsmLobpcgParams) if struct_size is None else struct_size, which, rtol, atol, maxiter, 0)
    info = L.BsmLobpcgInfo()
    pairs = (L.BsmEigshPair * max(nev, 1))()
    rc = L.lib().bsm_lobpcg_solve(ptr, X0, ldx0, X, ldx, None if "p" in null else C.byref(p), None if "info" in null else C.byref(info),
                                  None if "pairs" in null else pairs, history, capacity, memspace, stream)
    return rc, info, pairs


def raw_jacobi_h(A):
    """the unexported test hook bsm_debug_eig_jacobi_h -> (theta ascending, Q, sweeps)"""
    from bsm_amd import _lib as L
    fn = L.lib().bsm_debug_eig_jacobi_h
    fn.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]
    fn.restype = C.c_int
    cplx = np.iscomplexobj(A)
    A = np.asfortranarray(A, dtype=np.complex128 if cplx else np.float64)
    m = len(A)
    theta, Q, sw = np.zeros(m), np.zeros((m, m), A.dtype, order="F"), C.c_int32(-1)
    assert fn(int(cplx), m, A.ctypes.data, m, theta.ctypes.data, Q.ctypes.data, C.byref(sw)) == 0
    return theta, Q, sw.value


def raw_rr(GB, GA, use, k, which, tau):
    """the unexported test hook bsm_debug_lobpcg_rr -> (status, theta, C, drops)"""
    from bsm_amd import _lib as L
    fn = L.lib().bsm_debug_lobpcg_rr
    fn.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.POINTER(C.c_int32),
                   C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]
    fn.restype = C.c_int
    cplx = np.iscomplexobj(GB)
    dt = np.complex128 if cplx else np.float64
    GB, GA = np.asfortranarray(GB, dtype=dt), np.asfortranarray(GA, dtype=dt)
    p = len(GB)
    flags = np.ascontiguousarray(use, dtype=np.uint8)
    theta, Cm = np.full(k, np.nan), np.full((p, k), np.nan, dt, order="F")
    status, drops = C.c_int32(-1), C.c_int32(-1)
    assert fn(int(cplx), p, k, WHICH.get(which, which), GB.ctypes.data, GA.ctypes.data, flags.ctypes.data, tau, C.byref(status),
              theta.ctypes.data, Cm.ctypes.data, C.byref(drops)) == 0
    return status.value, theta, Cm, drops.value
