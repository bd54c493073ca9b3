"""What the lockstep-grid suites (test_lockstep_grid_cpu.py, test_gpu_lockstep_grid.py) share, and the guarded-buffer solve
that test_gpu_cg.py and test_gpu_bicgstab.py take from here: Python mirrors of the grid rule and of the workspace carve of
bsm_cg_create / bsm_bicgstab_create, the table of row counts that puts several workgroups on a column, the test problems on
those row counts, one calling convention for the twins of _cg.py / _bicgstab.py, and the spread of a twin under permuted
summation orders that the iterate checks take their bound from.  Test code only.

The layout under test (csrc/bsm_cg.h).  Every launch of the two solver units is a (G, K) grid, G = krylov_grid(n, es) row
ranges of 8192 bytes of a column (at most 256 of them) by K columns; a reduction leaves part[(c * G + wg) * NC + k], and
every consumer adds a column's G partials itself, lane-strided (a second pass from G = 65 on), then by xor-shuffles.

The problems.  Block diagonal, blocks of order 8 and one of order n mod 8, so that the twin needs no dense array:
  "cg"        _cg.spd_problem, blocks T^H T + I, rng = default_rng(8000 + n)
  "cocg"      csym_problem, blocks (T^T T + I) + 0.3 i (W + W^T) / 2 with real T, W: complex symmetric, NOT Hermitian,
              rng = default_rng(8500 + n); B = U + 0.3 i V with real uniform U, V (why: at CSYM_IMAG)
  "bicgstab"  nonsym_problem, blocks (T^H T + I) + (W - W^H) / 2: positive real, NOT symmetric, rng = default_rng(8800 + n)
              (why not the blocks T + 8 I of _bicgstab.edge_problem: at nonsym_problem)
T uniform in (-1, 1) (both parts for complex types); B: 16 uniform columns from the same generator.

Units.  An iterate's deviation is max|x - x_ref| in eps max|x_ref|, a history's max|h - h_ref| in eps ||b|| (deviation())."""
import numpy as np

from _bicgstab import bicgstab_twin
from _cg import MAX_RHS, BlockDiagonal, cg_twin, is_complex, spd_problem
from _gpu import dev_mat, outside_bytes
from _jacobi import uniform
from _krylov import real_of, rtol_of, wide_of

METHODS = ["cg", "cocg", "bicgstab"]
RANGE_BYTES = 8192  # of one column, per workgroup: 512 sixteen-byte groups (krylov_grid)
MAX_GRID = 256      # kKrylovMaxGrid
STATE_BYTES = 2 * (16 * 2 * 8 + 16 * 8 + 16 * 4 + 16 * 4) + 16 * 8 + 16 * 4 + (2 * 16 * 8 + 2 * 16 * 4)  # sizeof(CgState)
MARGIN = 4          # the iterate and history bounds are MARGIN x spread, as in test_gpu_bicgstab.py
ITS = 4             # iterations of the iterate checks


def path_rtol(dtype):
    """rtol of the runs to convergence at G = 2, 3: loose enough that the twin's count keeps to +-1 under permuted sums (at
    1e-10 BiCGSTAB's moved by 3 on one column: 56 / 59 iterations)"""
    return 1e-4 if np.finfo(dtype).eps > 1e-10 else 1e-6
# The complex symmetric problem of COCG: a real SPD part plus CSYM_IMAG times a real symmetric part as the imaginary one
# (a lossy medium), and right-hand sides whose imaginary parts are CSYM_IMAG times uniform.  The unconjugated form
# sum u_i v_i of vectors with real and imaginary parts of the SAME size cancels by a factor of about sqrt(n): on uniform
# complex data the twin's fourth iterate moved by 2 .. 350 eps max|x| from column to column under permuted sums, so that
# no spread of one column bounds another.  With the imaginary parts at 0.3 of the real ones the forms are sums of mostly
# positive terms (1.4 .. 6.5 eps over 16 columns), the imaginary share still decides alpha and beta, and the twin neither
# breaks down nor stalls: its counts at rtol 1e-4 / 1e-10 are pinned in test_lockstep_grid_cpu.py.
CSYM_IMAG = 0.3


# ---- the grid rule and what follows from it -----------------------------------------------------------------------------
def krylov_grid(n, es):
    """mirror of krylov_grid (csrc/bsm_krylov.h): row ranges of RANGE_BYTES, 1 .. MAX_GRID"""
    per = RANGE_BYTES // es
    return int(min(max((n + per - 1) // per, 1), MAX_GRID))


def last_range_rows(n, es):
    """rows of the LAST workgroup's range, mirror of wg_range (csrc/bsm_lockstep_device.h) on the 16-byte groups of a column"""
    ve = 16 // es
    ng = (max(n, 1) * es + 15) // 16
    G = krylov_grid(n, es)
    per = (ng + G - 1) // G
    return n - min(per * (G - 1), ng) * ve


# (multiple of R0 = RANGE_BYTES / itemsize, rows more, the G intended, what it exercises)
# (wg_range deals the 16-byte groups out evenly, per = ceil(groups / G) to a workgroup: at R0 + 1 the two ranges hold about
# half a tile each, not a tile and one row)
ROWS = [(1, 1, 2, "two ranges of half a tile, the second one group shorter"),
        (2, 3, 3, "odd n: padding up to a whole 16-byte group in the real double and both single types"),
        (64, 0, 64, "every range exactly one tile"),
        (64, 1, 65, "second lane-strided pass of wave_total: lane 0 adds two shares"),
        (256, 1, 256, "capped grid: per is one group more than a tile, every workgroup walks a second tile of one group")]
SINGLE_ROWS = [0, 3, 4]  # float32 and complex64 take rows 1, 4 and 5


def rows_of(dtype):
    """[(n, intended G)] of the table for `dtype`"""
    r0 = RANGE_BYTES // np.dtype(dtype).itemsize
    take = range(len(ROWS)) if np.finfo(dtype).eps < 1e-10 else SINGLE_ROWS
    return [(ROWS[i][0] * r0 + ROWS[i][1], ROWS[i][2]) for i in take]


TABLE = [(dt, n, G) for dt in (np.complex128, np.float64, np.float32, np.complex64) for n, G in rows_of(dt)]
TABLE_IDS = [f"{np.dtype(dt).name}-n{n}-G{G}" for dt, n, G in TABLE]
COLUMNS = [1, 3, 16]


def workspace_bytes(method, n, dtype, kmax=MAX_RHS, has_m=False, G=None):
    """info.workspace_bytes as bsm_cg_create / bsm_bicgstab_create carve it: the vectors as ld x kmax (ld: n rounded up to
    whole 16-byte groups), kmax * G partials per reduction (elements, or reals for the norms), the state; every piece
    rounded up to 64 bytes.  G: another grid than the mirror's (None: krylov_grid)"""
    es, rs = np.dtype(dtype).itemsize, np.dtype(real_of(dtype)).itemsize
    G = krylov_grid(n, es) if G is None else G
    ld = (max(n, 1) * es + 15) // 16 * 16 // es
    vec, pe, pr = ld * es * kmax, kmax * G * es, kmax * G * rs
    if method == "bicgstab":
        pieces = [vec] * (7 if has_m else 6) + [pe, pr, pe, pr, pr, pe, pr]
    else:
        pieces = [vec] * (5 if has_m else 4) + [pe, pe, pr, pr]
    return sum((b + 63) // 64 * 64 for b in pieces + [STATE_BYTES])


def bnorm_roundings(n, dtype):
    """m: the longest chain of roundings between the entries of b and info.bnorm, counted from start_kernel and dir_kernel
    of both units.  A thread adds the squares of its 16-byte groups by one FMA per real (one rounding each; its groups are
    256 apart in the workgroup's range, so ceil(per / 256) of them); wave_sum: 6 shuffle steps; block_sum: (a + b) + (c + d),
    2; wave_total: ceil(G / 64) lane-strided adds and 6 shuffle steps; the square root.  All terms are >= 0, so the sum is
    off by at most m - 1 relative roundings, and the root halves that and adds its own: <= m eps."""
    es, rs = np.dtype(dtype).itemsize, np.dtype(real_of(dtype)).itemsize
    G = krylov_grid(n, es)
    ng = (max(n, 1) * es + 15) // 16
    per = (ng + G - 1) // G
    return -(-per // 256) * (16 // rs) + 6 + 2 + -(-G // 64) + 6 + 1


# ---- the problems ---------------------------------------------------------------------------------------------------------
def csym_problem(rng, n, dtype, bs=8):
    """-> (vbcrs problem, BlockDiagonal): complex symmetric diagonal blocks (T^T T + I) + CSYM_IMAG i (W + W^T) / 2 of order
    bs (the last one n mod bs), T and W REAL uniform; the sibling of _cg.spd_problem for COCG"""
    assert is_complex(dtype)
    real = real_of(dtype)
    nb, t = n // bs, n % bs

    def blocks(m, k):
        T, W = uniform(rng, (m, k, k), real), uniform(rng, (m, k, k), real)
        S = np.einsum("bki,bkj->bij", T, T) + np.eye(k, dtype=real)
        return ((S + S.transpose(0, 2, 1)) / 2 + 1j * CSYM_IMAG * (W + W.transpose(0, 2, 1)) / 2).astype(dtype)
    main, tail = blocks(nb, bs), blocks(1, t)[0]
    blocks = [np.asfortranarray(main[b]) for b in range(nb)] + ([np.asfortranarray(tail)] if t else [])
    starts = np.arange(len(blocks), dtype=np.int64) * bs + 1
    return dict(kind="vbcrs", blocks=blocks, rowstart=starts, colstart=starts.copy(), size=(n, n)), BlockDiagonal(main, tail)


def nonsym_problem(rng, n, dtype, bs=8):
    """-> (vbcrs problem, BlockDiagonal): diagonal blocks (T^H T + I) + (W - W^H) / 2 of order bs (the last one n mod bs), T
    and W uniform: a Hermitian positive definite part and a skew part of the same size.  BiCGSTAB halves the residual per
    iteration on it (37 .. 74 iterations to 1e-10).  On the blocks T + 8 I of _bicgstab.edge_problem it gains a digit per
    iteration, the residual after four is 1e-4 .. 1e-6 of ||b|| and made of rounding in single precision, and the twin's
    history then moves by 0.02 .. 19 eps ||b|| from column to column under permuted sums, so that no spread of one column
    bounds another; here the 16 columns stay within 0.1 .. 0.9"""
    nb, t = n // bs, n % bs

    def blocks(m, k):
        T, W = uniform(rng, (m, k, k), dtype), uniform(rng, (m, k, k), dtype)
        S = np.einsum("bki,bkj->bij", T.conj(), T) + np.eye(k, dtype=dtype)
        return ((S + S.conj().transpose(0, 2, 1)) / 2 + (W - W.conj().transpose(0, 2, 1)) / 2).astype(dtype)
    main, tail = blocks(nb, bs), blocks(1, t)[0]
    blks = [np.asfortranarray(main[b]) for b in range(nb)] + ([np.asfortranarray(tail)] if t else [])
    starts = np.arange(len(blks), dtype=np.int64) * bs + 1
    return dict(kind="vbcrs", blocks=blks, rowstart=starts, colstart=starts.copy(), size=(n, n)), BlockDiagonal(main, tail)


_cases = {}


def grid_case(method, n, dtype):
    """-> (vbcrs problem, BlockDiagonal, B of MAX_RHS columns) of `method` (module docstring), computed once per
    (method, n, dtype) and not to be written to"""
    key = (method, n, np.dtype(dtype).name)
    if key not in _cases:
        rng = np.random.default_rng({"cg": 8000, "cocg": 8500, "bicgstab": 8800}[method] + n)
        p, Dop = {"cg": spd_problem, "cocg": csym_problem, "bicgstab": nonsym_problem}[method](rng, n, dtype)
        if method == "cocg":
            real = real_of(dtype)
            B = (uniform(rng, (n, MAX_RHS), real) + 1j * CSYM_IMAG * uniform(rng, (n, MAX_RHS), real)).astype(dtype)
        else:
            B = uniform(rng, (n, MAX_RHS), dtype)
        _cases[key] = (p, Dop, np.asfortranarray(B))
    return _cases[key]


def half_sets(n, bs=8):
    """1-based index sets: the two halves of every block of order bs, and the last block (order n mod bs) whole -- a
    block-Jacobi preconditioner over them is not the inverse of a block diagonal operator with blocks of order bs"""
    h = bs // 2
    sets = [np.arange(s, s + h) + 1 for s in range(0, n // bs * bs, h)]
    return sets + ([np.arange(n // bs * bs, n) + 1] if n % bs else [])


def block_solve(Dop, B):
    """diag(blocks)^-1 B in float64 / complex128"""
    nb, bs, _ = Dop.main.shape
    wide = wide_of(Dop.main.dtype)
    shape = np.shape(B)
    B = np.asarray(B).astype(wide).reshape(shape[0], -1)
    X = np.empty_like(B)
    if nb:
        X[:nb * bs] = np.linalg.solve(Dop.main.astype(wide), B[:nb * bs].reshape(nb, bs, -1)).reshape(nb * bs, -1)
    if Dop.tail.shape[0]:
        X[nb * bs:] = np.linalg.solve(Dop.tail.astype(wide), B[nb * bs:])
    return X.reshape(shape)


def staggered6(B, dtype, tau, step):
    """six columns for the decision tests -> (Bs, atol): columns 0 .. 3 are B's scaled by step**-c, so that under the one
    absolute tolerance atol = tau ||b_0|| they finish at different counts; column 4 is zero; column 5 is B's with one NaN in
    the last row, which lies in the LAST workgroup's range"""
    Bs = np.asfortranarray(B[:, :6].copy())
    for c in range(4):
        Bs[:, c] = (B[:, c] * dtype(step ** -c)).astype(dtype)
    Bs[:, 4] = 0
    Bs[-1, 5] = np.nan
    return Bs, tau * float(np.linalg.norm(Bs[:, 0].astype(np.complex128)))


# ---- the twins under one calling convention ----------------------------------------------------------------------------
def run_twin(method, D, b, dtype, rtol, maxiter, atol=0.0, Minv=None, x0=None, order=None, keep=None):
    """cg_twin (method "cg": conjugated form, "cocg": unconjugated) or bicgstab_twin in `dtype`"""
    if method == "bicgstab":
        return bicgstab_twin(D, b, Minv, rtol, atol, maxiter, dtype, x0=x0, order=order, keep=keep)
    return cg_twin(D, b, Minv, method == "cg", rtol, atol, maxiter, dtype, x0=x0, order=order, keep=keep)


def reference_of(dtype):
    """the type the reference of an iterate check runs in: the twin in float64 / complex128 for the single types (its
    rounding is then 2**-29 of the bound's unit), the same-precision twin for the double types"""
    return wide_of(dtype) if np.finfo(dtype).eps > 1e-10 else np.dtype(dtype).type


def reference(method, Dop, b, its, dtype, Minv=None, x0=None):
    """the twin's run of `its` iterations (rtol = 0) on the operator and right-hand side AS ROUNDED to dtype, evaluated in
    reference_of(dtype)"""
    return run_twin(method, Dop, b, reference_of(dtype), 0.0, its, Minv=Minv, x0=x0)


def deviation(x, hist, ref, its, dtype):
    """-> (max|x - ref's iterate `its`| in eps(dtype) max|ref's iterate|, max|hist[:its] - ref's history| in eps(dtype) ||b||).
    ||b|| is the scale the rounding of a recursively updated residual lives on, as max|x| is for the iterate: a residual
    that the iterations have reduced a thousandfold still carries the rounding of the vectors it is the difference of, so
    its error relative to ITSELF says how far the solve got, not how well the sums were formed"""
    xr, hr = ref.iterates[its - 1], ref.history[:its]
    dx = float(np.max(np.abs(np.asarray(x) - xr)) / (np.finfo(dtype).eps * np.max(np.abs(xr))))
    return dx, float(np.max(np.abs(np.asarray(hist, dtype=np.float64)[:its] - hr)) / (np.finfo(dtype).eps * ref.bnorm))


def spread(method, Dop, b, its, dtype, orders=8, Minv=None, x0=None):
    """How far the twin IN dtype moves by itself: the largest deviation() of its iterate number `its` and of its history
    from the unpermuted twin over `orders` permutations (seeds 0 ..) of the order of every form's and norm's sum and of the
    column order inside each diagonal block of the products -> (iterate: eps max|x|, history: relative).  What a device
    adds to this -- tree sums, fused multiply-adds, a multi-column product -- are further summation orders, not another
    method, so a small multiple of it bounds the device; a lost partial is another method"""
    a = run_twin(method, Dop, b, dtype, 0.0, its, Minv=Minv, x0=x0)
    assert a.status == 1 and a.iterations == its, (a.status, a.iterations)
    sx = sh = 0.0
    for seed in range(orders):
        o = np.random.default_rng(seed).permutation(len(b))
        p = run_twin(method, Dop, b, dtype, 0.0, its, Minv=Minv, x0=x0, order=o)
        dx, dh = deviation(p.x, p.history, a, its, dtype)
        sx, sh = max(sx, dx), max(sh, dh)
    return sx, sh


# ---- the solve inside guarded buffers ------------------------------------------------------------------------------------
def solve_in_guarded_buffers(torch, bsm, S, B, kmax, X0=None, **kw):
    """the solve with B at ldb = n + 3 and X one element past a 16-byte boundary (ldx = n + 1, kmax columns of room),
    both inside NaN-filled buffers: padding, guard elements and the columns beyond nrhs must keep their bytes.  X0: an
    initial guess, handed over IN that X buffer; kw: rtol (default rtol_of(B.dtype)), maxiter (200), atol"""
    n, k = B.shape
    bbuf, bview = dev_mat(torch, B, pad=3, guard=5)
    xfill = np.full((n, kmax), np.nan, dtype=B.dtype)
    if X0 is not None:
        xfill[:, :k] = X0
    xbuf, xall = dev_mat(torch, xfill, pad=1, off=1, guard=5)
    xview = xall[:, :k]
    before = (outside_bytes(bbuf, n, n + 3, k), outside_bytes(xbuf, n, n + 1, k, off=1), bbuf.cpu().numpy().tobytes())
    kw.setdefault("rtol", rtol_of(B.dtype))
    kw.setdefault("maxiter", 200)
    X, info = S.solve(bview, X=xview, X0=None if X0 is None else xview, **kw)
    torch.cuda.synchronize()
    assert outside_bytes(bbuf, n, n + 3, k) == before[0], "the padding of B was written"
    assert outside_bytes(xbuf, n, n + 1, k, off=1) == before[1], "X was written outside its n x nrhs window"
    assert bbuf.cpu().numpy().tobytes() == before[2], "B was written"
    return X.cpu().numpy(), info
