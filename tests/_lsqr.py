"""What the LSQR suites (test_lsqr_cpu.py, test_gpu_lsqr.py, test_lsqr_handles_cpu.py, test_gpu_lsqr_handles.py) share: the
numpy twin of bsm_lsqr_solve, the rectangular test problems, the operands and legs of the handle suites (described where they
are defined), the acceptance of a solve, and raw ctypes drivers of bsm_lsqr_create / _solve / _destroy and of the test hook
bsm_debug_lsqr_step.  Test code only.

The twin.  lsqr_twin is LSQR as include/bsm_rocm.h states the recurrences -- unnormalised Lanczos vectors, every scalar real,
the norms the real parts of sum conj(u) u, the two plane rotations, the decision in the header's order --, every array,
product and scalar rounded to `dtype` (scalars to its real type), with the statuses 0 (either stopping rule, or the Krylov
space ended), 1 (maxiter) and 2 (a non-finite estimate).  It shares no code with the library.  The vectors have two lengths,
so `order` is a PAIR of permutations (of the m rows of B, of the n rows of X) and `keep` a pair of counts.

The problems.
  Order 600 x 400 (lsqr_problem): from rng = default_rng(4000), in this order: A (600 x 400) uniform in (-1, 1) (both parts
  for complex types), Xtrue (400 x 5) uniform, Bi (600 x 5) uniform, Bu (400 x 5) uniform, the row sets cut(rng, 600), the
  column sets cut(rng, 400).  Bc = A Xtrue is the consistent right-hand side, Bi the inconsistent one, Bu that of the
  under-determined 400 x 600 system A^H X = Bu.  Cut as vbcrs (6 x 4 grid of 100 x 100 blocks) or blocksparse (one block per
  pair of a row set and a column set).
  Grid (tall_case): m x n, m >= n, block-built so that the twin needs no dense array.  The columns are cut into blocks of 8
  (the last one n mod 8); the m rows are dealt out evenly to the column blocks, block j owning h_j = m // nb or m // nb + 1
  consecutive rows (every h_j >= its width).  Block j is an h_j x w_j matrix whose top w_j x w_j part is T^H T + I (definite:
  full column rank whatever lies below) over h_j - w_j further uniform rows; rng = default_rng(9500 + m + n), B: 16 uniform
  columns from the same generator.  zero_rows > 0 appends that many rows no block covers (zero rows of A)."""
import ctypes as C

import numpy as np

from _cg import MAX_RHS, is_complex
from _jacobi import uniform
from _krylov import real_of
from _lockstep import deviation
from _submat import cut

M600, N400, NB = 600, 400, 5
LSQR_ITS = 4  # iterations of the iterate checks


def lsqr_rtol(dtype):
    """rtol = ntol of the runs to convergence: the values the twin's margins were established at"""
    return 1e-4 if np.finfo(dtype).eps > 1e-10 else 1e-8


# ---- operators the twin multiplies by -------------------------------------------------------------------------------------
class Dense:
    def __init__(self, A):
        self.A = np.asarray(A)
        self.shape = self.A.shape
        self.dtype = self.A.dtype
        self._kept = {}  # the conjugate transpose and the permuted copies: the same arrays at every product of a run

    def astype(self, dtype):
        return Dense(self.A.astype(dtype))

    def _keep(self, key, make):
        if key not in self._kept:
            self._kept[key] = make()
        return self._kept[key]

    def _permuted(self, which, M, perm):
        return self._keep((which, id(perm)), lambda: (perm, np.ascontiguousarray(M[:, perm])))[1]  # (perm is kept: its id stays its own)

    def times(self, v, perm=None):
        return self.A @ v if perm is None else self._permuted("N", self.A, perm) @ v[perm]

    def adj(self, u, perm=None):
        H = self._keep("H", lambda: self.A.conj().T)
        return H @ u if perm is None else self._permuted("H", H, perm) @ u[perm]

    @property
    def H(self):
        return Dense(self.A.conj().T)

    def dense(self):
        return self.A


class BlockTall:
    """non-overlapping dense blocks as the twin's operator where a dense array would not fit.  groups: [(first rows, first
    columns (0-based, one per block), blocks (g, h, w))], the blocks of one shape stacked"""

    def __init__(self, shape, groups, flipped=False):
        self.shape, self.groups, self.flipped = tuple(shape), groups, flipped
        self.dtype = groups[0][2].dtype

    def astype(self, dtype):
        return BlockTall(self.shape, [(r, c, S.astype(dtype)) for r, c, S in self.groups], self.flipped)

    @property
    def H(self):
        return BlockTall(self.shape[::-1], self.groups, not self.flipped)

    def _fwd(self, v, perm):
        out = np.zeros(self.shape[1] if self.flipped else self.shape[0], dtype=np.result_type(self.dtype, v.dtype))
        for r0, c0, S in self.groups:
            _, h, w = S.shape
            ri, ci = r0[:, None] + np.arange(h), c0[:, None] + np.arange(w)
            if perm is None:
                out[ri] = np.einsum("ghw,gw->gh", S, v[ci])
            else:  # the ranks of the permutation's first w entries: the order the columns of every block are summed in
                q = np.argsort(perm[:w])
                out[ri] = np.einsum("ghw,gw->gh", np.ascontiguousarray(S[:, :, q]), np.ascontiguousarray(v[ci][:, q]))
        return out

    def _bwd(self, u, perm):
        out = np.zeros(self.shape[0] if self.flipped else self.shape[1], dtype=np.result_type(self.dtype, u.dtype))
        for r0, c0, S in self.groups:
            _, h, w = S.shape
            ri, ci = r0[:, None] + np.arange(h), c0[:, None] + np.arange(w)
            if perm is None:
                out[ci] = np.einsum("ghw,gh->gw", S.conj(), u[ri])
            else:
                q = np.argsort(perm[:h])
                out[ci] = np.einsum("ghw,gh->gw", np.ascontiguousarray(S[:, q, :].conj()), np.ascontiguousarray(u[ri][:, q]))
        return out

    def times(self, v, perm=None):
        return self._bwd(v, perm) if self.flipped else self._fwd(v, perm)

    def adj(self, u, perm=None):
        return self._fwd(u, perm) if self.flipped else self._bwd(u, perm)

    def dense(self):
        D = np.zeros(self.shape[::-1] if self.flipped else self.shape, self.dtype)
        for r0, c0, S in self.groups:
            for b in range(len(r0)):
                D[r0[b]:r0[b] + S.shape[1], c0[b]:c0[b] + S.shape[2]] = S[b]
        return D.conj().T if self.flipped else D


def _as_op(A):
    return A if hasattr(A, "times") else Dense(A)


# ---- the twin ---------------------------------------------------------------------------------------------------------------
class LsqrTwin:
    """x, history (rnorm after every iteration), status, bnorm, iterates, per column the final estimates rnorm / arnorm / anorm,
    and steps: per iteration (the six scalars before it, beta', alpha', the ten values after it, the status as the library
    codes it: -1 running) for the scalar-step test"""

    def __init__(self, **kw):
        self.__dict__.update(kw)
        self.history = np.array(self.history, dtype=np.float64)
        self.iterations = len(self.history)
        self.residual = self.rnorm


def lsqr_twin(A, b, rtol, atol, ntol, damp, maxiter, dtype, x0=None, order=None, keep=None):
    """numpy twin of one column of bsm_lsqr_solve (module docstring) -> LsqrTwin.  A: dense (m x n) array, Dense or BlockTall;
    order: (permutation of m, permutation of n) the sums of the norms and of the products run in (None: as stored); keep: a
    MUTATION for the tests of the tests -- (km, kn): the norms of the m-vectors / n-vectors sum their first km / kn terms only,
    as a kernel that loses the last workgroup's share would (None: all; not together with order)"""
    dtype = np.dtype(dtype)
    real = real_of(dtype)
    R = real.type
    op = _as_op(A).astype(dtype)
    m, n = op.shape
    b = np.asarray(b).astype(dtype)
    assert order is None or keep is None
    pm, pn = (None, None) if order is None else order
    km, kn = (None, None) if keep is None else keep
    damp = R(damp)

    def norm(v, perm, k):
        t = (v.real.astype(real) ** 2 + v.imag.astype(real) ** 2).astype(real)
        t = t if perm is None else t[perm]
        return R(np.sqrt(np.sum(t if k is None else t[:k], dtype=real)))

    def times(v):
        return op.times(v, pn).astype(dtype)

    def adj(u):
        return op.adj(u, pm).astype(dtype)

    def decide(rnorm, arnorm, anorm, alpha, beta, tol):
        if not np.isfinite(rnorm) or not np.isfinite(arnorm):
            return 2
        if float(rnorm) <= tol or float(arnorm) <= ntol * float(anorm) * float(rnorm):
            return 0
        return 0 if alpha == 0 or beta == 0 else None

    with np.errstate(all="ignore"):
        x = np.zeros(n, dtype) if x0 is None else np.asarray(x0).astype(dtype)
        u = b.copy() if x0 is None else (b - times(x)).astype(dtype)
        beta, bnorm = norm(u, pm, km), norm(b, pm, km)
        tol = max(rtol * float(bnorm), atol)
        v = adj(u)
        if beta > 0 and np.isfinite(beta):
            v = (v * R(R(1) / beta)).astype(dtype)
        alpha = norm(v, pn, kn)
        phibar, rhobar, res2, anorm = beta, alpha, R(0), R(0)
        rnorm, arnorm = beta, R(alpha * beta)
        status = decide(rnorm, arnorm, anorm, alpha, beta, tol)
        w = (v * R(R(1) / alpha)).astype(dtype) if alpha > 0 else v.copy()
        hist, its, steps = [], [], []
        while status is None:
            if len(hist) >= maxiter:
                status = 1
                break
            before = [float(s) for s in (alpha, beta, phibar, rhobar, res2, anorm)]
            u = (R(R(1) / alpha) * times(v) - R(alpha / beta) * u).astype(dtype)
            betan = norm(u, pm, km)
            anorm = R(np.sqrt(R(R(R(anorm * anorm) + R(alpha * alpha)) + R(betan * betan)) + R(damp * damp)))
            if betan == 0:
                v, alphan = np.zeros(n, dtype), R(0)
            else:
                v = (R(R(1) / betan) * adj(u) - R(betan / alpha) * v).astype(dtype)
                alphan = norm(v, pn, kn)
            rhobar1 = R(np.sqrt(R(R(rhobar * rhobar) + R(damp * damp))))
            cs1, sn1 = (R(1), R(0)) if rhobar1 == 0 else (R(rhobar / rhobar1), R(damp / rhobar1))
            psi, phibar = R(sn1 * phibar), R(cs1 * phibar)
            rho = R(np.sqrt(R(R(rhobar1 * rhobar1) + R(betan * betan))))
            c, s = (R(1), R(0)) if rho == 0 else (R(rhobar1 / rho), R(betan / rho))
            theta, rhobar, phi = R(s * alphan), R(-c * alphan), R(c * phibar)
            phibar = R(s * phibar)
            tau = R(s * phi)
            cx, cw = (R(0), R(0)) if rho == 0 else (R(phi / rho), R(theta / rho))
            x = (x + cx * w).astype(dtype)
            w = ((R(R(1) / alphan) * v if alphan != 0 else 0) - cw * w).astype(dtype)
            res2 = R(res2 + R(psi * psi))
            rnorm, arnorm = R(np.sqrt(R(R(phibar * phibar) + res2))), R(alphan * abs(tau))
            alpha, beta = alphan, betan
            status = decide(rnorm, arnorm, anorm, alpha, beta, tol)
            hist.append(float(rnorm))
            its.append(x.copy())
            steps.append((before, float(betan), float(alphan), [float(s) for s in (alpha, beta, phibar, rhobar, res2, anorm, cx, cw, rnorm, arnorm)],
                          -1 if status is None else status))
    return LsqrTwin(x=x, history=hist, status=status, bnorm=float(bnorm), iterates=its, rnorm=float(rnorm), arnorm=float(arnorm),
                    anorm=float(anorm), tol=tol, steps=steps)


def history_unit(sh):
    """the history spread a bound is taken from: lsqr_spread's, and 1 eps ||b|| where that is EXACTLY 0.  rnorm is a number of
    the size of ||b|| after LSQR_ITS iterations, one unit in its last place is up to 1 eps ||b||, and the twin's permuted runs
    can all round to the same one (complex128, 131073 x 513): a bound of 0 is one only bit-identity with the twin would
    meet.  Every other spread is used as it is"""
    return sh if sh > 0 else 1.0


def orders(seed, m, n):
    """the pair of permutations number `seed`"""
    rng = np.random.default_rng(seed)
    return rng.permutation(m), rng.permutation(n)


def lsqr_spread(op, b, its, dtype, norders=8, x0=None, damp=0.0):
    """_lockstep.spread for lsqr_twin: the largest deviation() of the twin IN dtype under `norders` permuted summation orders
    from its unpermuted run -> (iterate: eps max|x|, history: eps ||b||)"""
    op = _as_op(op)
    a = lsqr_twin(op, b, 0.0, 0.0, 0.0, damp, its, dtype, x0=x0)
    assert a.status == 1 and a.iterations == its, (a.status, a.iterations)
    sx = sh = 0.0
    for seed in range(norders):
        p = lsqr_twin(op, b, 0.0, 0.0, 0.0, damp, its, dtype, x0=x0, order=orders(seed, *op.shape))
        dx, dh = deviation(p.x, p.history, a, its, dtype)
        sx, sh = max(sx, dx), max(sh, dh)
    return sx, sh


# ---- the problems -----------------------------------------------------------------------------------------------------------
_problems = {}


def lsqr_problem(kind, dtype):
    """-> (problem of A, A (600 x 400), Xtrue, Bc, Bi, Bu) (module docstring); computed once per (kind, dtype) and not to be
    written to"""
    key = (kind, np.dtype(dtype).name)
    if key in _problems:
        return _problems[key]
    rng = np.random.default_rng(4000)
    A = uniform(rng, (M600, N400), dtype)
    Xtrue = uniform(rng, (N400, NB), dtype)
    Bi = np.asfortranarray(uniform(rng, (M600, NB), dtype))
    Bu = np.asfortranarray(uniform(rng, (N400, NB), dtype))
    rsets, csets = cut(rng, M600), cut(rng, N400)
    Bc = np.asfortranarray((A.astype(np.complex128) @ Xtrue.astype(np.complex128)).astype(dtype) if is_complex(dtype)
                           else (A.astype(np.float64) @ Xtrue.astype(np.float64)).astype(dtype))
    if kind == "vbcrs":
        blocks, rs, cs = [], [], []
        for a in range(0, M600, 100):
            for b in range(0, N400, 100):
                blocks.append(np.asfortranarray(A[a:a + 100, b:b + 100]))
                rs.append(a + 1)
                cs.append(b + 1)
        p = dict(kind="vbcrs", blocks=blocks, rowstart=np.array(rs, np.int64), colstart=np.array(cs, np.int64), size=(M600, N400))
    else:
        assert kind == "blocksparse"
        blocks, ri, ci = [], [], []
        for a in rsets:
            for b in csets:
                blocks.append(np.asfortranarray(A[np.ix_(a - 1, b - 1)]))
                ri.append(a)
                ci.append(b)
        p = dict(kind="blocksparse", blocks=blocks, rowindices=ri, colindices=ci, size=(M600, N400))
    _problems[key] = (p, A, Xtrue, Bc, Bi, Bu)
    return _problems[key]


def tall_problem(rng, m, n, dtype, bs=8, zero_rows=0):
    """-> (vbcrs problem of size (m + zero_rows, n), BlockTall) (module docstring)"""
    widths = [bs] * (n // bs) + ([n % bs] if n % bs else [])
    nb = len(widths)
    assert m // nb >= bs
    heights = [m // nb + (1 if j < m % nb else 0) for j in range(nb)]
    r0 = np.concatenate([[0], np.cumsum(heights)[:-1]]).astype(np.int64)
    c0 = np.concatenate([[0], np.cumsum(widths)[:-1]]).astype(np.int64)
    shapes = sorted(set(zip(heights, widths)))
    groups, blocks = [], [None] * nb
    for h, w in shapes:
        idx = np.array([j for j in range(nb) if (heights[j], widths[j]) == (h, w)])
        T = uniform(rng, (len(idx), w, w), dtype)
        top = (np.einsum("bki,bkj->bij", T.conj(), T) + np.eye(w, dtype=dtype)).astype(dtype)
        S = np.concatenate([top, uniform(rng, (len(idx), h - w, w), dtype)], axis=1).astype(dtype)
        groups.append((r0[idx], c0[idx], S))
        for k, j in enumerate(idx):
            blocks[j] = np.asfortranarray(S[k])
    p = dict(kind="vbcrs", blocks=blocks, rowstart=r0 + 1, colstart=c0 + 1, size=(m + zero_rows, n))
    return p, BlockTall((m + zero_rows, n), groups)


_cases = {}


def tall_case(m, n, dtype, zero_rows=0):
    """-> (problem, BlockTall, B of MAX_RHS uniform columns of m + zero_rows rows, Bt of MAX_RHS uniform columns of n rows: the
    right-hand sides of the system through adjoint(A)) from rng = default_rng(9500 + m + n), computed once and not to be
    written to"""
    key = (m, n, np.dtype(dtype).name, zero_rows)
    if key not in _cases:
        rng = np.random.default_rng(9500 + m + n)
        p, op = tall_problem(rng, m, n, dtype, zero_rows=zero_rows)
        _cases[key] = (p, op, np.asfortranarray(uniform(rng, (m + zero_rows, MAX_RHS), dtype)),
                       np.asfortranarray(uniform(rng, (n, MAX_RHS), dtype)))
    return _cases[key]


def singular_symmetric():
    """-> (D, B): D = Q diag(0 x 10, 30 values 1 .. 3) Q^T of order 40, symmetrised to the bit -- singular by construction, rank 30
    --, and three consistent right-hand sides D X; rng = default_rng(31).  The twin needs 24, 23, 23 iterations to 1e-8 and
    keeps them under permuted sums (test_lsqr_cpu.py)"""
    rng = np.random.default_rng(31)
    Q, _ = np.linalg.qr(rng.uniform(-1, 1, (40, 40)))
    D = (Q * np.concatenate([np.zeros(10), np.linspace(1, 3, 30)])) @ Q.T
    D = (D + D.T) / 2
    return D, np.asfortranarray(D @ rng.uniform(-1, 1, (40, 3)))


# ---- the handle suites (test_lsqr_handles_cpu.py, test_gpu_lsqr_handles.py) -------------------------------------------------
# An OPERAND is a dense operator A (m x n) with five inconsistent right-hand sides Bi (m rows) and five right-hand sides Bu (n
# rows) of the under-determined system A^H X = Bu.  A LEG of it is a system the twin and the device solve: "inconsistent" is
# (A, Bi), ended by rule 2; "adjoint" is (A^H, Bu) -- Lsqr(adjoint(H)) --, ended by rule 1.  The operands:
#   base         lsqr_problem's A, Bi, Bu (the pairs test_lsqr_cpu.py pins: its legs "inconsistent" and "under");
#   cvec         the real base operand of the complex type's precision under complex columns Bi + i Bi[:, ::-1], Bu + i Bu[:, ::-1]
#                (the columns of test_real_operator_under_complex_vectors);
#   rounded      base with A rounded to single precision and widened again: what a storage=float32 / complex64 handle holds;
#   bordered     the blocks of the blocksparse base problem at size (608, 408): rows 601 .. 608 and columns 401 .. 408 lie in no
#                block.  B (608 x 5), then Bu (408 x 5) uniform from default_rng(4700), the uncovered rows of Bu zeroed (A^H X =
#                Bu is consistent then).  The uncovered entries of X are zero in every iterate: X is a combination of the v, and
#                v = A^H u has exact zeros there;
#   symmetric    D = Q diag(+-linspace(1, 3, 400)) Q^T of order 400, signs alternating, symmetrised to the bit, and five uniform
#                columns B; rng = default_rng(4100): Q, the sets cut(rng, 400), B in this order.  Real types only.  D is regular,
#                both legs are (D, B) ended by rule 1;
#   vbcrs2       base with block 1 of the VBCRS grid (rows 1 .. 100 x columns 1 .. 100) negated, as
#                test_one_solver_across_update_blocks does;
#   blocksparse2 base with every block of the largest row set negated (block 1 of that cut is 1 x 1): ten ids, a partial update.
LEGS = ("inconsistent", "adjoint")
BORDER = 8
_operands, _handle_runs, _extra = {}, {}, {}


class Operand:
    def __init__(self, A, Bi, Bu):
        self.A, self.Bi, self.Bu = A, Bi, Bu


def single_of(dtype):
    return np.dtype(np.complex64 if is_complex(dtype) else np.float32)


def complex_columns(B, cdtype):
    return np.asfortranarray((B + 1j * B[:, ::-1]).astype(cdtype))


def largest_row_set(dtype=np.float64):
    """-> (position of the largest row set of the blocksparse cut, its 0-based rows, the 1-based ids of its blocks)"""
    p = lsqr_problem("blocksparse", dtype)[0]
    sizes = [len(r) for r in p["rowindices"]]
    big = max(sizes)
    ids = [k + 1 for k, s in enumerate(sizes) if s == big]
    rows = p["rowindices"][ids[0] - 1]
    assert all(np.array_equal(p["rowindices"][k - 1], rows) for k in ids)
    return ids[0] - 1, rows - 1, ids


def bordered_problem(dtype):
    """-> (blocksparse problem of size (608, 408), A, B, Bu) (the operand `bordered`); computed once, not to be written to"""
    key = ("bordered", np.dtype(dtype).name)
    if key not in _extra:
        p0, A0 = lsqr_problem("blocksparse", dtype)[:2]
        m, n = M600 + BORDER, N400 + BORDER
        A = np.zeros((m, n), dtype)
        A[:M600, :N400] = A0
        rng = np.random.default_rng(4700)
        B = np.asfortranarray(uniform(rng, (m, NB), dtype))
        Bu = np.asfortranarray(uniform(rng, (n, NB), dtype))
        Bu[N400:] = 0
        _extra[key] = (dict(p0, size=(m, n)), A, B, Bu)
    return _extra[key]


def symmetric_problem(dtype):
    """-> (symmetric problem of order 400: a diagonal block per set, every lower off-diagonal block; D; B) (the operand
    `symmetric`); computed once, not to be written to"""
    key = ("symmetric", np.dtype(dtype).name)
    if key not in _extra:
        assert not is_complex(dtype)
        rng = np.random.default_rng(4100)
        Q, _ = np.linalg.qr(rng.uniform(-1, 1, (N400, N400)))
        D = (Q * (np.linspace(1, 3, N400) * np.where(np.arange(N400) % 2 == 0, 1.0, -1.0))) @ Q.T
        D = ((D + D.T) / 2).astype(dtype)
        sets = cut(rng, N400)
        B = np.asfortranarray(uniform(rng, (N400, NB), dtype))
        offs, ri, ci = [], [], []
        for a in range(len(sets)):
            for b in range(a):
                offs.append(np.asfortranarray(D[np.ix_(sets[a] - 1, sets[b] - 1)]))
                ri.append(sets[a])
                ci.append(sets[b])
        p = dict(kind="symmetric", diagonals=[np.asfortranarray(D[np.ix_(s - 1, s - 1)]) for s in sets], diagonalindices=sets,
                 offdiagonals=offs, rowindices=ri, colindices=ci, size=(N400, N400))
        _extra[key] = (p, D, B)
    return _extra[key]


def operand(name, dtype):
    """-> Operand (the table above); computed once per (name, dtype) and not to be written to"""
    key = (name, np.dtype(dtype).name)
    if key in _operands:
        return _operands[key]
    if name == "cvec":
        assert is_complex(dtype)
        _, A, _, _, Bi, Bu = lsqr_problem("vbcrs", real_of(dtype))
        o = Operand(A.astype(dtype), complex_columns(Bi, dtype), complex_columns(Bu, dtype))
    elif name == "bordered":
        o = Operand(*bordered_problem(dtype)[1:])
    elif name == "symmetric":
        _, D, B = symmetric_problem(dtype)
        o = Operand(D, B, B)
    else:
        _, A, _, _, Bi, Bu = lsqr_problem("vbcrs", dtype)
        if name == "rounded":
            assert np.dtype(dtype) != single_of(dtype)
            A = A.astype(single_of(dtype)).astype(dtype)
        elif name == "vbcrs2":
            A = A.copy()
            A[:100, :100] = -A[:100, :100]
        elif name == "blocksparse2":
            A = A.copy()
            rows = largest_row_set(dtype)[1]
            A[rows] = -A[rows]
        else:
            assert name == "base", name
        o = Operand(A, Bi, Bu)
    _operands[key] = o
    return o


def leg_system(name, dtype, leg):
    """-> (dense operator of the system, B, the rule its columns end by)"""
    o = operand(name, dtype)
    assert leg in LEGS
    if name == "symmetric":
        return o.A, o.Bi, 1
    return (o.A, o.Bi, 2) if leg == "inconsistent" else (np.ascontiguousarray(o.A.conj().T), o.Bu, 1)


def leg_runs(name, dtype, leg):
    """the twin on the five columns of a leg at rtol = ntol = lsqr_rtol(dtype), maxiter 400; computed once"""
    key = (name, np.dtype(dtype).name, "adjoint" if name == "symmetric" else leg)
    if key not in _handle_runs:
        A, B, _ = leg_system(name, dtype, leg)
        r = lsqr_rtol(dtype)
        _handle_runs[key] = [lsqr_twin(A, B[:, c], r, 0.0, r, 0.0, 400, dtype) for c in range(NB)]
    return _handle_runs[key]


def new_values(kind, dtype):
    """the update legs' second set of values -> (1-based ids, the new blocks, the problem with them in place, the operand's name)"""
    p = lsqr_problem(kind, dtype)[0]
    ids = [1] if kind == "vbcrs" else largest_row_set(dtype)[2]
    blocks = list(p["blocks"])
    for k in ids:
        blocks[k - 1] = np.asfortranarray(-p["blocks"][k - 1])
    return ids, [blocks[k - 1] for k in ids], dict(p, blocks=blocks), kind + "2"


class Half:
    """an operator whose forward product uses one set of values and whose adjoint product another: what LSQR sees of a
    transpose_image handle whose refill reached one image only"""

    def __init__(self, forward, backward):
        self.forward, self.backward = _as_op(forward), _as_op(backward)
        assert self.forward.shape == self.backward.shape
        self.shape, self.dtype = self.forward.shape, self.forward.dtype

    def astype(self, dtype):
        return Half(self.forward.astype(dtype), self.backward.astype(dtype))

    def times(self, v, perm=None):
        return self.forward.times(v, perm)

    def adj(self, u, perm=None):
        return self.backward.adj(u, perm)


# ---- what the GPU suite accepts ---------------------------------------------------------------------------------------------
def true_criteria(A, x, b, tol, ntol, anorm, damp=0.0, x0=None):
    """in complex128: (||r|| / tol, ||A^H r - damp^2 (x - x0)|| / (ntol anorm ||rbar||)) with r = b - A x and rbar the residual
    of the damped system -- the two stopping rules as the true quantities state them (inf where a threshold is zero)"""
    op = _as_op(A).astype(np.complex128)
    x = np.asarray(x).astype(np.complex128)
    dx = x if x0 is None else x - np.asarray(x0).astype(np.complex128)
    r = np.asarray(b).astype(np.complex128) - op.times(x)
    rbar = float(np.sqrt(np.linalg.norm(r) ** 2 + (damp * np.linalg.norm(dx)) ** 2))
    g = float(np.linalg.norm(op.adj(r) - damp * damp * dx))
    first = rbar / tol if tol > 0 else np.inf
    second = g / (ntol * anorm * rbar) if ntol * anorm * rbar > 0 else (0.0 if g == 0 else np.inf)
    return first, second


def check_columns(info, runs, A, x, B, rtol, ntol, what, rule, damp=0.0, use_x0=False):
    """every column: status 0, the twin's count (+-1: the multi-column products round differently from one column, the twin's
    count is stable under permuted sums -- test_lsqr_cpu.py), the true criterion of stopping rule `rule` (1: the residual, 2:
    the normal-equation residual, with info.anorm[c]) <= 2 x its threshold evaluated in complex128, and the product count"""
    op = _as_op(A)
    x = np.asarray(x).reshape(op.shape[1], -1)
    for c, run in enumerate(runs):
        tol = rtol * float(np.linalg.norm(B[:, c].astype(np.complex128)))
        crit = true_criteria(op, x[:, c], B[:, c], tol, ntol, float(info.anorm[c]), damp)[rule - 1]
        print(f"LSSTAT {what} column {c}: {info.column_iterations[c]} iterations, twin {run.iterations}, rule {rule} criterion / threshold "
              f"{crit:.3f}, anorm {info.anorm[c]:.4g} (twin {run.anorm:.4g})")
        assert run.status == 0, (what, c, "the twin did not converge")
        assert info.column_status[c] == 0, (what, c, info.column_status[c])
        assert abs(int(info.column_iterations[c]) - run.iterations) <= 1, (what, c, info.column_iterations[c], run.iterations)
        assert crit <= 2, (what, c, crit)
    assert info.iterations == max(info.column_iterations) and info.status == 0 and info.columns_converged == len(runs)
    check_products(info, use_x0)


def check_products(info, use_x0=False):
    assert info.a_products == 2 * info.iterations + 1 + (1 if use_x0 else 0)
    assert info.m_products == 0


# ---- raw ctypes drivers --------------------------------------------------------------------------------------------------
def raw_lsqr_create(A, opA, code, nrhs_max):
    """bsm_lsqr_create as C sees it -> (return code, solver pointer); a created solver is destroyed by the caller"""
    from bsm_amd import _lib as L
    out = C.c_void_p(0xdead)
    rc = L.lib().bsm_lsqr_create(None if A is None else A._h.ptr, opA, code, nrhs_max, C.byref(out))
    return rc, out


def raw_lsqr_destroy(ptr):
    from bsm_amd import _lib as L
    return L.lib().bsm_lsqr_destroy(ptr)


def raw_lsqr_solve(ptr, nrhs, B, ldb, X, ldx, rtol=1e-8, atol=0.0, ntol=1e-8, damp=0.0, maxiter=100, use_x0=0, capacity=None, memspace=1,
                   stream=None, struct_size=None, want_cols=True):
    """bsm_lsqr_solve as C sees it (B, X: addresses) -> (return code, info, columns, history of `capacity` rows prefilled with
    -1, arnorm, anorm)"""
    from bsm_amd import _lib as L
    cap = maxiter if capacity is None else capacity
    p = L.BsmLsqrParams(C.sizeof(L.BsmLsqrParams) if struct_size is None else struct_size, use_x0, rtol, atol, ntol, damp, maxiter, cap)
    info = L.BsmCgInfo()
    cols = (L.BsmCgColumn * max(nrhs, 1))() if want_cols else None
    hist = np.full((max(cap, 1), max(nrhs, 1)), -1.0)
    arn, an = np.full(max(nrhs, 1), -1.0), np.full(max(nrhs, 1), -1.0)
    dp = C.POINTER(C.c_double)
    rc = L.lib().bsm_lsqr_solve(ptr, nrhs, B, ldb, X, ldx, C.byref(p), C.byref(info), cols, hist.ctypes.data_as(dp), arn.ctypes.data_as(dp),
                                an.ctypes.data_as(dp), memspace, stream)
    return rc, info, cols, hist, arn, an


def raw_lsqr_step(scalars, betan, alphan, damp, tol, ntol):
    """the unexported test hook bsm_debug_lsqr_step (csrc/bsm_lsqr.cpp) -> (the ten values after the step, status)"""
    from bsm_amd import _lib as L
    fn = L.lib().bsm_debug_lsqr_step
    dp = C.POINTER(C.c_double)
    fn.argtypes = [dp, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, dp, C.POINTER(C.c_int32)]
    fn.restype = C.c_int
    a, out, status = np.array(scalars, dtype=np.float64), np.zeros(10), C.c_int32(99)
    rc = fn(a.ctypes.data_as(dp), betan, alphan, damp, tol, ntol, out.ctypes.data_as(dp), C.byref(status))
    assert rc == 0
    return out, status.value
