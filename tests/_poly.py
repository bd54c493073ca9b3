"""What the polynomial-preconditioner suites (test_poly_cpu.py, test_gpu_poly.py) share: the numpy twin of a composed handle's
product (bsm_poly_create), the Chebyshev recurrence in exact rational arithmetic, the dense p(A) a solver's twin takes as
Minv, the inner preconditioners of the grid problems, the acceptance of a product against the twin, and raw ctypes drivers of
bsm_poly_create / bsm_poly_info.  Test code only.

The twin.  poly_twin is the recurrence include/bsm_rocm.h states,
    r_0 = x,  d_0 = b_0 D r_0;   r_{k+1} = r_k - A d_k,  d_{k+1} = a_{k+1} d_k + b_{k+1} D r_{k+1};   p(A) x = d_0 + .. + d_{s-1}
with every array, every product and every scaled vector rounded to `dtype` on its own (numpy rounds each operation; the
coefficients are rounded to the real type of dtype first).  It shares no code with the library.

Units.  A product's deviation is max|got - ref| in eps(dtype) max|ref| (deviation())."""
import ctypes as C
from fractions import Fraction

import numpy as np

from _cg import BlockDiagonal
from _krylov import ERR_DEVICE, ERR_INVALID, ERR_UNSUPPORTED, real_of, wide_of  # noqa: F401
from _lockstep import MARGIN, reference_of

MAX_STEPS = 64  # BSM_POLY_MAX_STEPS
ORDERS = 8      # permuted product orders of the spread, the seeds of _lockstep.spread


# ---- the twin -------------------------------------------------------------------------------------------------------------
def _times(H, v, dtype, order):
    """H v rounded to dtype; H: dense array or BlockDiagonal; order: a permutation the sums of the product run in (None:
    as stored; a BlockDiagonal permutes inside its blocks)"""
    if isinstance(H, BlockDiagonal):
        return H.times(v, order).astype(dtype)
    if order is None:
        return (H @ v).astype(dtype)
    return (np.ascontiguousarray(H[:, order]) @ v[order]).astype(dtype)


def poly_twin(Dop, Dinv, a, b, R, dtype, order=None):
    """numpy twin of M @ R for M = bsm_poly_create(A, D, a, b) (module docstring).  Dop: A, Dinv: D or None (the identity),
    each a dense array or a _cg.BlockDiagonal; R: a vector or a matrix, column by column; order: see _times"""
    dtype = np.dtype(dtype)
    real = real_of(dtype)
    A = Dop.astype(dtype)
    D = None if Dinv is None else Dinv.astype(dtype)
    a, b = np.asarray(a, np.float64).astype(real), np.asarray(b, np.float64).astype(real)
    R = np.asarray(R).astype(dtype)
    if R.ndim == 2:
        return np.asfortranarray(np.stack([poly_twin(Dop, Dinv, a, b, R[:, c], dtype, order) for c in range(R.shape[1])], axis=1))

    def inner(v):
        return v if D is None else _times(D, v, dtype, order)
    with np.errstate(all="ignore"):
        r = R.copy()
        d = (b[0] * inner(r)).astype(dtype)
        acc = None
        for k in range(len(b) - 1):
            acc = d.copy() if acc is None else (acc + d).astype(dtype)
            r = (r - _times(A, d, dtype, order)).astype(dtype)
            d = ((a[k + 1] * d).astype(dtype) + (b[k + 1] * inner(r)).astype(dtype)).astype(dtype)
        return d if acc is None else (acc + d).astype(dtype)


def dense_poly(D, Dinv, a, b, dtype=None):
    """the dense p(A) of the recurrence in float64 / complex128 (dtype: rounded to it at the end): what a solver's twin takes
    as Minv"""
    wide = wide_of(D.dtype)
    P = poly_twin(D.astype(wide), None if Dinv is None else np.asarray(Dinv).astype(wide), a, b, np.eye(D.shape[0], dtype=wide), wide)
    return P if dtype is None else P.astype(dtype)


# ---- the coefficients -----------------------------------------------------------------------------------------------------
def chebyshev_exact(lmin, lmax, steps):
    """the recurrence of bsm.chebyshev_coefficients in exact rational arithmetic -> (a, b), lists of Fractions"""
    lmin, lmax = Fraction(lmin), Fraction(lmax)
    theta, delta = (lmax + lmin) / 2, (lmax - lmin) / 2
    sigma = theta / delta
    rho = 1 / sigma
    a, b = [Fraction(0)], [1 / theta]
    for _ in range(1, steps):
        nxt = 1 / (2 * sigma - rho)
        a.append(nxt * rho)
        b.append(2 * nxt / delta)
        rho = nxt
    return a, b


def residual_polynomial(a, b, lam):
    """1 - lam p(lam) of the recurrence with coefficients a, b on the scalar operator A = lam, D = 1, in the arithmetic of its
    arguments (Fractions: exact)"""
    r = 1
    d = b[0] * r
    total = d
    for k in range(len(b) - 1):
        r = r - lam * d
        d = a[k + 1] * d + b[k + 1] * r
        total = total + d
    return 1 - lam * total


def chebyshev_t(s, x):
    """T_s(x) by the three-term recurrence, in the arithmetic of x"""
    t0, t1 = 1, x
    if s == 0:
        return t0
    for _ in range(s - 1):
        t0, t1 = t1, 2 * x * t1 - t0
    return t1


def neumann_coefficients(omega, steps):
    return np.zeros(steps), np.full(steps, float(omega))


# ---- inner preconditioners of the grid problems ------------------------------------------------------------------------------
def half_inverse(Dop, dtype=None):
    """The block-Jacobi preconditioner of a _cg.BlockDiagonal with blocks of order 8 over _lockstep.half_sets(n) -- the two
    halves of every block, the tail block whole -- as a BlockDiagonal of blocks of order 4: the exact inverses, taken in
    float64 / complex128 and rounded to dtype (default: the operator's)"""
    dtype = Dop.main.dtype if dtype is None else dtype
    wide = wide_of(Dop.main.dtype)
    nb, bs, _ = Dop.main.shape
    h = bs // 2
    halves = np.stack([Dop.main[:, :h, :h], Dop.main[:, h:, h:]], axis=1).reshape(2 * nb, h, h).astype(wide)
    main = np.linalg.inv(halves).astype(dtype) if nb else halves.astype(dtype)
    t = Dop.tail.shape[0]
    tail = np.linalg.inv(Dop.tail.astype(wide)).astype(dtype) if t else Dop.tail.astype(dtype)
    return BlockDiagonal(main, tail)


# ---- the acceptance of a product ------------------------------------------------------------------------------------------------
def deviation(got, ref, dtype):
    """max|got - ref| in eps(dtype) max|ref|"""
    ref = np.asarray(ref)
    return float(np.max(np.abs(np.asarray(got) - ref)) / (np.finfo(dtype).eps * np.max(np.abs(ref))))


def twin_spread(Dop, Dinv, a, b, R, dtype, ref):
    """how far the twin IN dtype moves by itself: its largest deviation from its unpermuted run over ORDERS permuted product
    orders (seeds 0 ..), in eps(dtype) max|ref|; where that is EXACTLY 0 (one step without D has no product at all) one
    rounding unit stands in, as _lsqr.history_unit does"""
    base = poly_twin(Dop, Dinv, a, b, R, dtype)
    unit = np.finfo(dtype).eps * np.max(np.abs(ref))
    s = 0.0
    for seed in range(ORDERS):
        o = np.random.default_rng(seed).permutation(np.shape(R)[0])
        s = max(s, float(np.max(np.abs(poly_twin(Dop, Dinv, a, b, R, dtype, order=o) - base)) / unit))
    return s if s > 0 else 1.0


def accept(got, Dop, Dinv, a, b, R, dtype, what, spread_columns=1):
    """The acceptance of M @ R against the twin: the reference is the twin in _lockstep.reference_of(dtype) on the operators
    as rounded to dtype, the bound MARGIN x the same-precision twin's spread (twin_spread, taken on the first
    `spread_columns` columns), both in eps(dtype) max|reference|.  Prints the figures before it asserts them -> (deviation,
    spread, the reference)."""
    R = np.asarray(R)
    A = Dop.astype(dtype)
    D = None if Dinv is None else Dinv.astype(dtype)
    rt = reference_of(dtype)
    ref = poly_twin(A.astype(rt), None if D is None else D.astype(rt), a, b, R.astype(dtype).astype(rt), rt)
    Rs = R[:, :spread_columns] if R.ndim == 2 else R
    refs = ref[:, :spread_columns] if R.ndim == 2 else ref
    s = twin_spread(A, D, a, b, Rs, dtype, refs)
    dev = deviation(got, ref, dtype)
    print(f"POLYSTAT {what}: deviation {dev:.3f}, spread {s:.3f}, bound {MARGIN * s:.3f} (eps max|ref|)")
    assert np.all(np.isfinite(np.asarray(got))), (what, "not finite")
    assert dev <= MARGIN * s, (what, dev, s)
    return dev, s, ref


# ---- raw ctypes drivers ---------------------------------------------------------------------------------------------------------
def raw_poly_create(A, opA, D, opD, code, nrhs_max, a, b, steps=None, want_out=True):
    """bsm_poly_create as C sees it -> (return code, handle pointer); a created handle is destroyed by the caller
    (raw_destroy).  a, b: sequences or None (a null pointer); steps: default len(b)"""
    from bsm_amd import _lib as L
    dp = C.POINTER(C.c_double)
    av = None if a is None else np.ascontiguousarray(a, dtype=np.float64)
    bv = None if b is None else np.ascontiguousarray(b, dtype=np.float64)
    steps = len(bv) if steps is None else steps
    out = C.c_void_p()
    rc = L.lib().bsm_poly_create(None if A is None else A._h.ptr, opA, None if D is None else D._h.ptr, opD, code, nrhs_max, steps,
                                 None if av is None else av.ctypes.data_as(dp), None if bv is None else bv.ctypes.data_as(dp),
                                 C.byref(out) if want_out else None)
    return rc, out


def raw_destroy(ptr):
    from bsm_amd import _lib as L
    return L.lib().bsm_destroy(ptr)
