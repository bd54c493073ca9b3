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
from _cg import MAX_RHS, BlockDiagonal, cg_twin, column_tol, is_complex, spd_problem
from _gpu import dev_mat, outside_bytes
from _jacobi import uniform
from _krylov import real_of, rtol_of, true_residual, wide_of

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


# ---- the solver table (test_solver_handles_cpu.py, test_gpu_solver_handles.py) -------------------------------------------
# One row per device solver: what a test that runs EVERY solver on some kind of handle needs of it -- the order-400 problem
# of its own suite, its numpy twin, its Python class, the kinds it admits, the acceptance helper of its GPU suite (moved
# into its _*.py module unchanged) and the rtol of that suite's test against the twin.  The rows hide the solvers' calling
# conventions behind case() / runs() / make() / solve() / accept(); nothing here is looser or tighter than the suites.
# D2 = D1 + W diag(SHIFT * J) W of the update legs.  Stale values of A show at any shift (true residuals 1e9 tolerances off);
# a stale M shows in the COUNT only, and a uniform shift mostly rescales the block inverse, which CG does not see: at 8, 16
# and 32 the twins of cg, cocg and bicgstab with the old block inverse stay within +-1 of the fresh ones; at 64 they leave
# it by one, at 128 by 3 .. 5 (MINRES by 17 .. 20, GMRES(20) stagnates).  test_solver_handles_cpu.py asserts the margins.
SHIFT = 128.0
WIDE_TYPES = [np.float64, np.complex128]
SINGLE_TYPES = [np.float32, np.complex64]


class Case:
    """p: the problem of A; pm: the problem M is built from (p itself; MINRES: the definite sibling); sets; D, P: their
    dense forms; B: the right-hand sides (n x NB, GMRES: n x 1); w: the problem's power-of-two row scaling (ones where
    it has none); sign: +-1 per row, the pattern J of the MINRES problem (ones elsewhere)"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def row_scaling(seed, n, dtype):
    """w of _cg.cg_problem / _bicgstab.bicgstab_problem / _minres.minres_problem, which keep it to themselves: their draws
    replayed (the sets, G, then one exponent per set) -> (w, sets)"""
    from _submat import cut
    rng = np.random.default_rng(seed)
    sets = cut(rng, n)
    uniform(rng, (n, n), dtype)
    w = np.ones(n)
    for s in sets:
        w[s - 1] = 2.0 ** int(rng.integers(-3, 4))
    return w, sets


class Solver:
    def __init__(self, name, problem, twin, cls, kinds, accept, rtol, maxiter=100, complex_kinds=None, real=True, nrhs=5,
                 restart=None, method=None, passes=None, m_passes=False):
        self.name, self.problem, self.twin, self.cls, self.kinds, self.check, self.rtol = name, problem, twin, cls, kinds, accept, rtol
        self.maxiter, self.complex_kinds, self.real, self.nrhs = maxiter, kinds if complex_kinds is None else complex_kinds, real, nrhs
        self.restart, self.method = restart, method
        # passes(info, first): info.a_products of a solve cut at the count of the free-running `first`, as the equality of
        # the solver's own pass-count test states it (None: its suite has no such test); m_passes: that test counts M too
        self.passes, self.m_passes = passes, m_passes

    def kinds_of(self, dtype):
        return self.complex_kinds if is_complex(dtype) else (self.kinds if self.real else [])

    def cases(self, types=WIDE_TYPES, kinds=None):
        return [(self.name, k, dt) for dt in types for k in self.kinds_of(dt) if kinds is None or k in kinds]

    def case(self, kind, dtype):
        from _krylov import krylov_problem
        from _submat import Truth
        n = 400
        if self.name in ("gmres", "gmres_multi"):
            from _gmres_multi import columns400
            p, sets, b = krylov_problem(kind, dtype)
            D = Truth(p).D
            B = columns400(kind, dtype) if self.name == "gmres_multi" else np.asfortranarray(b.reshape(-1, 1))
            return Case(p=p, pm=p, sets=sets, D=D, P=D, B=B, w=np.ones(n), sign=np.ones(n))
        if self.name == "minres":
            p, pp, sets, D, P, B = self.problem(kind, dtype)
            w, wsets = row_scaling(4000, n, dtype)
            sign = np.ones(n)
            for k, s in enumerate(sets):
                sign[s - 1] = 1.0 if k % 2 == 0 else -1.0
        else:
            p, sets, D, B = self.problem(kind, dtype, is_complex(dtype)) if self.name == "cg" else self.problem(kind, dtype)
            w, wsets = row_scaling(6000 if self.name == "bicgstab" else 4000, n, dtype)
            pp, P, sign = p, D, np.ones(n)
        assert all(np.array_equal(a, b) for a, b in zip(sets, wsets))
        return Case(p=p, pm=pp, sets=sets, D=D, P=P, B=B, w=w, sign=sign)

    def runs(self, D, B, Minv, dtype, rtol=None):
        """the twin on every column of B"""
        rtol = self.rtol(dtype) if rtol is None else rtol
        cols = [np.ascontiguousarray(B[:, c]) for c in range(B.shape[1])]
        if self.name in ("cg", "cocg"):
            return [self.twin(D, b, Minv, self.name == "cg", rtol, 0.0, self.maxiter, dtype) for b in cols]
        if self.name in ("gmres", "gmres_multi"):
            return [self.twin(D, b, Minv, self.restart, rtol, self.maxiter, dtype) for b in cols]
        return [self.twin(D, b, Minv, rtol, 0.0, self.maxiter, dtype) for b in cols]

    def make(self, bsm, A, M, nrhs=None, dtype=None):
        kw = dict(dtype=dtype)
        if self.restart is not None:
            kw["restart"] = self.restart
        if self.method is not None:
            kw["method"] = self.method
        if self.name != "gmres":
            kw["nrhs"] = self.nrhs if nrhs is None else nrhs
        return getattr(bsm, self.cls)(A, M, **kw)

    def solve(self, S, Bd, **kw):
        """-> (X, info) of S.solve on a column-major device matrix Bd (GMRES: on its one column) at this row's rtol / maxiter"""
        kw.setdefault("rtol", self.rtol(np.dtype(S.dtype)))
        kw.setdefault("maxiter", self.maxiter)
        return S.solve(Bd[:, 0] if self.name == "gmres" else Bd, **kw)

    def slack(self, twin_iterations):
        """(below, above): how far a count may lie from the twin's under this row's acceptance"""
        if self.name in ("gmres", "gmres_multi"):
            return twin_iterations, max(2, twin_iterations // 10)
        return 1, 1

    def accept(self, info, runs, D, X, B, what, rtol=None):
        """the acceptance of this solver's own suite on the columns B.shape[1] of a solve; prints the worst figures first"""
        rtol = self.rtol(np.dtype(B.dtype)) if rtol is None else rtol
        X = np.asarray(X).reshape(D.shape[0], -1)
        k = B.shape[1]
        tols = [column_tol(B[:, c], rtol) for c in range(k)]
        its = [int(info.iterations)] if self.name == "gmres" else [int(v) for v in info.column_iterations]
        worst = max(true_residual(D, X[:, c], B[:, c]) / tols[c] for c in range(k))
        print(f"HANDSTAT {self.name} {what}: worst true residual / tol {worst:.3f}, iterations {its}, twin {[r.iterations for r in runs]}")
        if self.name == "gmres":
            assert info.status == 0 and info.converged
            assert true_residual(D, X[:, 0], B[:, 0]) <= 2 * tols[0], (what, worst)
            self.check(info, runs[0], what)
        elif self.name == "gmres_multi":
            self.check(info, runs, D, X, B, rtol, what)
        else:
            self.check(info, runs, D, X, B, tols, what)
        return worst


_solvers = {}


def solvers():
    """name -> Solver.  Built at the first call: _gmres_multi.py imports this module"""
    if not _solvers:
        import _bicgstab
        import _cg
        import _gmres_multi
        import _krylov
        import _minres
        three, two = ["vbcrs", "blocksparse", "symmetric"], ["vbcrs", "blocksparse"]
        rows = [
            Solver("cg", _cg.cg_problem, _cg.cg_twin, "Cg", three, _cg.check_columns, rtol_of, complex_kinds=two, method="cg",
                   passes=lambda info, first: info.iterations),
            Solver("cocg", _cg.cg_problem, _cg.cg_twin, "Cg", three, _cg.check_columns, rtol_of, real=False, method="cocg",
                   passes=lambda info, first: info.iterations),
            Solver("bicgstab", _bicgstab.bicgstab_problem, _bicgstab.bicgstab_twin, "BiCgStab", two, _bicgstab.check_columns, rtol_of,
                   passes=lambda info, first: 2 * info.iterations),
            Solver("minres", _minres.minres_problem, _minres.minres_twin, "Minres", three, _minres.check_columns, rtol_of, maxiter=200,
                   complex_kinds=two, passes=lambda info, first: info.iterations, m_passes=True),
            Solver("gmres_multi", _krylov.krylov_problem, _gmres_multi.gmres_multi_twin, "GmresMulti", three, _gmres_multi.check_columns,
                   rtol_of, restart=_krylov.RESTART, passes=lambda info, first: first.a_products),
            Solver("gmres", _krylov.krylov_problem, _krylov.gmres_twin, "Gmres", three, _krylov.check_against_twin, rtol_of, nrhs=1,
                   restart=_krylov.RESTART),
        ]
        _solvers.update({r.name: r for r in rows})
    return _solvers


def solver_cases(types=WIDE_TYPES, kinds=None, names=None):
    """[(solver name, kind, dtype)] of the table, solver by solver"""
    return [c for r in solvers().values() if names is None or r.name in names for c in r.cases(types, kinds)]


def case_id(c):
    return "-".join([c[0], c[1], np.dtype(c[2]).name] + [str(v) for v in c[3:]])


def shifted(case, shift=SHIFT):
    """the update legs' second set of values -> Case(ids, new: the 1-based ids and new values of the blocks of p that change;
    mids, mnew: those of pm; p2, pm2: the problems with them in place; D2, P2: their dense forms).  D2 = D + W diag(shift *
    sign) W, P2 = P + W diag(shift) W; only the blocks that hold a diagonal entry change (_values.diagonal_shift)"""
    from _submat import Truth
    from _values import diagonal_shift, src_list, with_values

    def one(p, d):
        ids, new = diagonal_shift(p, d)
        vals = list(src_list(p))
        for i, b in zip(ids, new):
            vals[i - 1] = b
        p2 = with_values(p, vals)
        return ids, new, p2, Truth(p2).D
    ids, new, p2, D2 = one(case.p, shift * case.sign * case.w * case.w)
    if case.pm is case.p:
        return Case(ids=ids, new=new, mids=ids, mnew=new, p2=p2, pm2=p2, D2=D2, P2=D2)
    mids, mnew, pm2, P2 = one(case.pm, shift * case.w * case.w)
    return Case(ids=ids, new=new, mids=mids, mnew=mnew, p2=p2, pm2=pm2, D2=D2, P2=P2)
