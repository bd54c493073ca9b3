"""What the suites of bsm_eigh_blocks / bsm_spectral_blocks and of the spectral block-Jacobi preconditioner share
(test_eigh_blocks_cpu.py, test_gpu_eigh_blocks.py, test_gpu_spectral_jacobi.py): the numpy twin of the rotation sequence
include/bsm_rocm.h fixes, the test matrices, the accuracy figures, references for V f(w) V^H and raw ctypes drivers.  Test
code only; the twin shares no code with the library.

The twin.  eigh_twin runs the two-sided round-robin Jacobi method in the block's own type: m = n rounded up to even, m - 1
steps per sweep, step t holds the pairs (t, m-1) and ((t + k) mod (m-1), (t - k) mod (m-1)), every pair derives its rotation
from the entries before the step, then the column phase of all pairs, the row phase of all pairs, the three fixed entries.

Matrices (CLASSES), all Hermitian up to what `asym` adds:
  uniform   (G + G^H) / 2, G uniform in (-1, 1);
  cluster   Q diag(d) Q^H, d = a triple eigenvalue 1, five values 2 + k 1e-6, the rest uniform in (-3, 3);
  rank3     X X^H, X of three uniform columns;
  scaled    W (S + 24 I) W, S uniform Hermitian, W = diag(2^k), k uniform in -10 .. 10;
  diagonal  a diagonal with repeated entries;   zero   all zeros.

Figures, in float64 / complex128 against numpy.linalg.eigvalsh of the symmetrised block, eps that of the block's real type,
||.|| the Frobenius norm:  rho_w = max|w - lambda| / (n eps ||H||),  rho_r = ||H V - V diag(w)|| / (2 n eps ||H||),
rho_o = ||V^H V - I|| / (2 n^1.5 eps).  The twin stays <= 1.0 (test_eigh_blocks_cpu.py asserts it on the inputs of the GPU
suite); the kernel and the host route must stay <= RHO_MAX = 4 (FMA contraction, the reciprocal square root, the update order:
the factor of _jacobi.py)."""
import ctypes as C

import numpy as np

from _jacobi import CODE, DTYPES, RHO_MAX, dense_of, set_blocks, uniform  # noqa: F401
from _minres import cut_operator, minres_problem

CLASSES = ("uniform", "cluster", "rank3", "scaled", "diagonal", "zero")
BASE_ORDERS = (0, 1, 2, 3, 8, 9, 17, 64, 65, 129)
# the class of every block of batch(): BASE_ORDERS, then the seam pair (both regimes get a full matrix)
BATCH_CLASSES = ("uniform", "scaled", "uniform", "cluster", "diagonal", "zero", "uniform", "cluster", "rank3", "scaled", "uniform", "cluster")
MAX_SWEEPS = 60
LDS_BYTES = 131072


def real_of(dtype):
    return np.dtype(np.float32) if np.dtype(dtype) in (np.dtype(np.float32), np.dtype(np.complex64)) else np.dtype(np.float64)


def wide_of(dtype):
    return np.complex128 if np.dtype(dtype).kind == "c" else np.float64


def eigh_seam(dtype):
    """largest order whose 2 n^2 sizeof(T) fits BSM_EIGH_LDS_BYTES: A and V resident in LDS, seam + 1 in device memory"""
    n = int(np.sqrt(LDS_BYTES // (2 * np.dtype(dtype).itemsize)))
    assert 2 * n * n * np.dtype(dtype).itemsize <= LDS_BYTES < 2 * (n + 1) ** 2 * np.dtype(dtype).itemsize
    return n


def spectral_seam(dtype):
    """largest order whose n^2 sizeof(T) fits BSM_EIGH_LDS_BYTES: V staged in LDS"""
    n = int(np.sqrt(LDS_BYTES // np.dtype(dtype).itemsize))
    assert n * n * np.dtype(dtype).itemsize <= LDS_BYTES < (n + 1) ** 2 * np.dtype(dtype).itemsize
    return n


def herm(G):
    return (G + G.conj().T) / 2


def matrix(rng, cls, n, dtype):
    """one test matrix of class cls, column-major, in dtype"""
    dtype = np.dtype(dtype)
    wide = wide_of(dtype)
    if cls == "uniform":
        H = herm(uniform(rng, (n, n), wide))
    elif cls == "cluster":
        Q, _ = np.linalg.qr(uniform(rng, (n, n), wide))
        d = rng.uniform(-3, 3, n)
        d[:3] = 1.0
        d[3:8] = 2.0 + 1e-6 * np.arange(len(d[3:8]))
        H = herm((Q * d) @ Q.conj().T)
    elif cls == "rank3":
        X = uniform(rng, (n, min(n, 3)), wide)
        H = herm(X @ X.conj().T)
    elif cls == "scaled":
        w = 2.0 ** rng.integers(-10, 11, n)
        H = w[:, None] * (herm(uniform(rng, (n, n), wide)) + 24 * np.eye(n)) * w[None, :]
    elif cls == "diagonal":
        H = np.diag(rng.integers(-2, 3, n).astype(np.float64)).astype(wide)
    else:
        assert cls == "zero"
        H = np.zeros((n, n), wide)
    H = H.astype(dtype)
    H = ((H + H.conj().T) / 2).astype(dtype)  # Hermitian to the bit in dtype; the tests of asymmetry add their own
    return np.asfortranarray(H)


_batches = {}


def batch(dtype):
    """the blocks of the GPU suite's one call, per dtype: BASE_ORDERS and the seam pair of the type, the classes spread over
    them; computed once per dtype and not to be written to -> list of (class, block)"""
    key = np.dtype(dtype).name
    if key not in _batches:
        rng = np.random.default_rng(3800 + CODE[np.dtype(dtype)])
        s = eigh_seam(dtype)
        orders = list(BASE_ORDERS) + [s, s + 1]
        _batches[key] = [(c, matrix(rng, c, n, dtype)) for c, n in zip(BATCH_CLASSES, orders)]
    return _batches[key]


# ---- the twin ---------------------------------------------------------------------------------------------------------------
def eigh_twin(B, vectors=True):
    """-> (w ascending, V or None, sweeps that rotated, info) of (B + B^H) / 2 in B's own type (module docstring)"""
    B = np.asarray(B)
    dtype, real = B.dtype, real_of(B.dtype)
    R = real.type
    n = B.shape[0]
    if n == 0:
        return np.zeros(0, real), np.zeros((0, 0), dtype), 0, 0
    if not np.all(np.isfinite(B)):
        return np.full(n, np.nan, real), None, 0, 1
    with np.errstate(all="ignore"):
        H = ((B + B.conj().T) / R(2)).astype(dtype)
        H[np.arange(n), np.arange(n)] = H.diagonal().real
        V = np.eye(n, dtype=dtype)
        m = n + (n & 1)
        ks = np.arange(m // 2)
        sweeps, info = 0, 2
        while sweeps < MAX_SWEEPS:
            rotated = 0
            for t in range(m - 1):
                a = np.where(ks == 0, t, (t + ks) % max(m - 1, 1))
                b = np.where(ks == 0, m - 1, (t - ks) % max(m - 1, 1))
                p, q = np.minimum(a, b), np.maximum(a, b)
                live = q < n
                p, q = p[live], q[live]
                apq = H[p, q]
                app, aqq = H[p, p].real.astype(real), H[q, q].real.astype(real)
                g = np.abs(apq).astype(real)
                nz = g != 0
                skip = nz & (np.abs(app) + g == np.abs(app)) & (np.abs(aqq) + g == np.abs(aqq))
                rot = nz & ~skip & np.isfinite(g) & np.isfinite(app) & np.isfinite(aqq)
                H[p[skip], q[skip]] = 0
                H[q[skip], p[skip]] = 0
                if not rot.any():
                    continue
                P, Q, g, app, aqq, apq = p[rot], q[rot], g[rot], app[rot], aqq[rot], apq[rot]
                tau = ((aqq - app) / (R(2) * g)).astype(real)
                tt = (np.where(tau >= 0, R(1), R(-1)) / (np.abs(tau) + np.sqrt(R(1) + tau * tau))).astype(real)
                c = (R(1) / np.sqrt(R(1) + tt * tt)).astype(real)
                s = (tt * c).astype(real)
                w = (apq / g).astype(dtype)
                for M in (H, V) if vectors else (H,):
                    X, Y = M[:, P], (np.conj(w) * M[:, Q]).astype(dtype)
                    M[:, P], M[:, Q] = (c * X - s * Y).astype(dtype), (s * X + c * Y).astype(dtype)
                X, Y = H[P, :], (w[:, None] * H[Q, :]).astype(dtype)
                H[P, :], H[Q, :] = (c[:, None] * X - s[:, None] * Y).astype(dtype), (s[:, None] * X + c[:, None] * Y).astype(dtype)
                H[P, P], H[Q, Q] = (app - tt * g).astype(real), (aqq + tt * g).astype(real)
                H[P, Q] = 0
                H[Q, P] = 0
                rotated += len(P)
            if not rotated:
                info = 0
                break
            sweeps += 1
        d = H.diagonal().real.astype(real)
        order = np.argsort(d, kind="stable")
    return d[order], (np.asfortranarray(V[:, order]) if vectors else None), sweeps, info


# ---- figures ----------------------------------------------------------------------------------------------------------------
def figures(B, w, V=None):
    """-> (rho_w, rho_r, rho_o) of the pairs (w, V) of block B (module docstring); V None: rho_r = rho_o = 0"""
    n = B.shape[0]
    if n == 0:
        return 0.0, 0.0, 0.0
    wide = wide_of(B.dtype)
    eps = float(np.finfo(real_of(B.dtype)).eps)
    H = herm(np.asarray(B).astype(wide))
    lam = np.linalg.eigvalsh(H)
    nrm = float(np.linalg.norm(H))
    w64 = np.asarray(w).astype(np.float64)

    def ratio(num, den):
        if not np.isfinite(num):
            return float("inf")
        return 0.0 if num == 0 else (float("inf") if den == 0 else float(num / den))
    rho_w = ratio(np.max(np.abs(w64 - lam)), n * eps * nrm)
    if V is None:
        return rho_w, 0.0, 0.0
    V64 = np.asarray(V).astype(wide)
    rho_r = ratio(np.linalg.norm(H @ V64 - V64 * w64[None, :]), 2 * n * eps * nrm)
    rho_o = ratio(np.linalg.norm(V64.conj().T @ V64 - np.eye(n)), 2 * n ** 1.5 * eps)
    return rho_w, rho_r, rho_o


# ---- V f(w) V^H ---------------------------------------------------------------------------------------------------------------
FUNC = {"values": 0, "inv": 1, "absinv": 2, "pinv": 3}


def f_of(w, func, rcond):
    """f(w) in float64 as include/bsm_rocm.h states it (finite w)"""
    w = np.asarray(w).astype(np.float64)
    bound = rcond * np.max(np.abs(w)) if len(w) and rcond > 0 else 0.0
    with np.errstate(all="ignore"):
        if func == "values":
            return w
        if func == "inv":
            return 1.0 / w
        if func == "absinv":
            return 1.0 / np.maximum(np.abs(w), bound)
        return np.where(np.abs(w) > bound, 1.0 / np.where(w == 0, 1.0, w), 0.0)


def spectral_ref(V, f):
    """-> (V diag(f) V^H, sum_k |f_k| |V_ik| |V_jk|) in float64 / complex128: the value and the scale of the fma bound"""
    V64 = np.asarray(V).astype(wide_of(np.asarray(V).dtype))
    f = np.asarray(f, dtype=np.float64)
    return (V64 * f[None, :]) @ V64.conj().T, (np.abs(V64) * np.abs(f)[None, :]) @ np.abs(V64).T


def fma_factor(n, dtype):
    """entries of out lie within fma_factor * eps * scale of the exact sum: n + 2 roundings per real entry, 2n + 4 per complex"""
    return (2 * n + 4 if np.dtype(dtype).kind == "c" else n + 2) * float(np.finfo(real_of(dtype)).eps)


def check_spectral(out, V, f, what, extra=0.0):
    """out against V diag(f) V^H within the fma bound (+ extra * scale), Hermitian to the bit, real diagonal"""
    out = np.asarray(out)
    n = out.shape[0]
    if n == 0:
        return 0.0
    want, scale = spectral_ref(V, f)
    err = np.abs(out.astype(want.dtype) - want)
    tol = (fma_factor(n, out.dtype) + extra) * scale
    worst = float(np.max(err / np.where(tol == 0, 1.0, tol)))
    assert np.all(err <= tol), (what, n, worst)
    assert np.array_equal(out, out.conj().T), (what, "not Hermitian to the bit")
    if out.dtype.kind == "c":
        assert not out.diagonal().imag.any(), (what, "diagonal not real")
    return worst


# ---- the spectral block-Jacobi preconditioner ----------------------------------------------------------------------------------
# the twin's MINRES iterations on the five columns of the order-400 indefinite problem of _minres.py, M = the abs block inverse
# of D itself (numpy.linalg.eigh in the wide type, rounded to dtype), rtol_of(dtype), maxiter 200
ABS_COUNTS = {"float32": [24, 24, 22, 22, 22], "float64": [50] * 5, "complex64": [21, 22, 21, 21, 21], "complex128": [48] * 5}


def abs_minv(D, sets, dtype=None, func="absinv", rcond=0.0):
    """sum_s E_s f(D[I_s, I_s]) E_s^T with numpy.linalg.eigh in float64 / complex128, rounded to dtype"""
    dtype = D.dtype if dtype is None else dtype
    blocks = []
    for blk in set_blocks(D, sets):
        w, V = np.linalg.eigh(((blk + blk.conj().T) / 2).astype(wide_of(D.dtype)))
        blocks.append(((V * f_of(w, func, rcond)[None, :]) @ V.conj().T).astype(dtype))
    return dense_of(blocks, sets, D.shape[0], dtype), blocks


def decomposition_tol(H, M, n, dtype):
    """Frobenius bound of || M_got - f(H) ||, f = 1 / |.| or the pseudo-inverse, for eigenpairs with figures <= RHO_MAX: they are
    the exact pairs of H + E, ||E|| <= RHO_MAX 2 n eps ||H||, up to V = V'(I + F), ||F|| <= RHO_MAX 2 n^1.5 eps, so the error is
    within 3 ||M||_2^2 ||E|| (the perturbation bound of a pseudo-inverse of unchanged rank; 1 would do for an inverse) plus
    ||F|| ||M||_F ... 2 n eps RHO_MAX (3 ||H|| ||M||_2^2 + sqrt(n) ||M||) -- plus the fma bound of the product itself"""
    eps = float(np.finfo(real_of(dtype)).eps)
    return RHO_MAX * 2 * n * eps * (3 * np.linalg.norm(H) * np.linalg.norm(M, 2) ** 2 + np.sqrt(n) * np.linalg.norm(M)) + \
        fma_factor(n, dtype) * np.linalg.norm(M) * np.sqrt(n)


def check_spectral_jacobi(bsm, M, D, sets, func, rcond, what):
    _, want = abs_minv(D, sets, wide_of(D.dtype), func, rcond)
    worst = 0.0
    for s, (H, ref) in enumerate(zip(set_blocks(D, sets), want)):
        got = bsm.block(M, s + 1)
        got = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
        assert got.dtype == D.dtype and np.array_equal(got, got.conj().T), (what, s)
        err = np.linalg.norm(got.astype(ref.dtype) - ref)
        tol = decomposition_tol(H.astype(ref.dtype), ref, len(sets[s]), D.dtype)
        worst = max(worst, err / tol)
        assert err <= tol, (what, s, len(sets[s]), err, tol)
    print(f"EIGHSTAT block_jacobi {what}: worst error / bound {worst:.3f}")


def rank_deficient(kind, dtype):
    """minres_problem's D with the block of its 8-set replaced by X X^H of rank 5 -> (problem, sets, D, index of the set)"""
    _, _, sets, D, _, _ = minres_problem(kind, dtype)
    k = [i for i, s in enumerate(sets) if len(s) == 8][0]
    X = uniform(np.random.default_rng(3870), (8, 5), dtype)
    D = D.copy()
    D[np.ix_(sets[k] - 1, sets[k] - 1)] = (X @ X.conj().T).astype(dtype)
    D[np.ix_(sets[k] - 1, sets[k] - 1)] = ((D[np.ix_(sets[k] - 1, sets[k] - 1)] + D[np.ix_(sets[k] - 1, sets[k] - 1)].conj().T) / 2)
    return cut_operator(kind, D, sets), sets, D, k


# ---- raw ctypes drivers --------------------------------------------------------------------------------------------------
def _ptr_array(items):
    out = (C.c_void_p * max(len(items), 1))()
    for k, b in enumerate(items):
        out[k] = b.ctypes.data if isinstance(b, np.ndarray) else b
    return out


def raw_eigh(code, blocks, n, ld, ws, vectors=1, info=True, sweeps=True, memspace=0, stream=None, nblocks=None, null=()):
    """bsm_eigh_blocks as C sees it -> (return code, info, sweeps), both prefilled with -77.  blocks, ws: numpy buffers, device
    addresses or None; info / sweeps False: NULL; null: names of the host arrays to pass as NULL ("blocks", "n", "ld", "w")"""
    from bsm_amd import _lib as L
    nb = len(blocks) if nblocks is None else nblocks
    nn, ll = np.ascontiguousarray(n, dtype=np.int64), np.ascontiguousarray(ld, dtype=np.int64)
    inf = np.full(max(len(blocks), 1), -77, dtype=np.int64)
    sw = np.full(max(len(blocks), 1), -77, dtype=np.int32)
    P = C.POINTER(C.c_int64)
    rc = L.lib().bsm_eigh_blocks(code, nb, None if "blocks" in null else _ptr_array(blocks), None if "n" in null else nn.ctypes.data_as(P),
                                 None if "ld" in null else ll.ctypes.data_as(P), None if "w" in null else _ptr_array(ws), vectors,
                                 inf.ctypes.data_as(P) if info else None, sw.ctypes.data_as(C.POINTER(C.c_int32)) if sweeps else None,
                                 memspace, stream)
    return rc, inf[:len(blocks)], sw[:len(blocks)]


def raw_spectral(code, V, n, ldv, ws, func, rcond, out, ldo, info=True, memspace=0, stream=None, nblocks=None, null=()):
    """bsm_spectral_blocks as C sees it -> (return code, info prefilled with -77); null: "V", "n", "ldv", "w", "out", "ldo\""""
    from bsm_amd import _lib as L
    nb = len(V) if nblocks is None else nblocks
    nn, lv, lo = (np.ascontiguousarray(a, dtype=np.int64) for a in (n, ldv, ldo))
    inf = np.full(max(len(V), 1), -77, dtype=np.int64)
    P = C.POINTER(C.c_int64)
    rc = L.spectral_blocks_call(code, nb, None if "V" in null else _ptr_array(V), None if "n" in null else nn.ctypes.data_as(P),
                                None if "ldv" in null else lv.ctypes.data_as(P), None if "w" in null else _ptr_array(ws), func, rcond,
                                None if "out" in null else _ptr_array(out), None if "ldo" in null else lo.ctypes.data_as(P),
                                inf.ctypes.data_as(P) if info else None, memspace, stream)
    return rc, inf[:len(V)]
