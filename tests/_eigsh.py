"""What the eigsh suites (test_eigsh_cpu.py, test_gpu_eigsh.py, test_eigsh_grid_cpu.py, test_gpu_eigsh_grid.py) share: the numpy
twin of bsm_eigsh_solve, the test problems, the acceptance checks (check_pairs, and accept for a device solve) and raw ctypes
drivers of bsm_krylov_combine, bsm_eigsh_create / _solve / _destroy and the test hooks bsm_debug_eig_jacobi / _select / _keep.
Test code only.

The twin.  eigsh_twin is thick-restart Lanczos as include/bsm_rocm.h states it: the same step order (product, two classical
Gram-Schmidt passes whose coefficients add up, norm, guarded scale), the projected matrix T kept in double with the analytic
arrow entries beta_m S[m - 1, i] after a restart, the same selection and keep rules, anorm = the largest |theta| seen, the
same statuses.  Every vector, product and coefficient is rounded to `dtype`.  T is diagonalised by numpy.linalg.eigh, not by
the library's Jacobi method: it shares no code with the library.

The problem.  Order 400.  Eigenvalues lam: -3.3, -2.2, -1.5, -0.9, -0.4, then 390 values uniform in [1, 2], then 3, 3.6, 4.3, 5.1,
6.  rng = default_rng(3600): sets = _submat.cut(rng, 400), the bulk, G Gaussian 400 x 400 (complex types: real part, then
imaginary part), Q = the Q of qr(G), D = Q diag(lam) Q^H symmetrised, v0 = uniform(-1, 1) from default_rng(1).  D is cut the way
_cg.cg_problem cuts its D: a 4 x 4 grid of 100 x 100 blocks (vbcrs), one block per pair of sets (blocksparse), or D[I_s, I_s]
as diagonals and D[I_a, I_b], a > b, as off-diagonals (symmetric: real types only).

The grid problems (grid_eig_problem).  Orders that put 2 and 3 workgroups on a vector (grid_sizes).  Block diagonal, Hermitian
blocks of order 8 and one of order n mod 8, so that the twin and the acceptance need no dense array: the designed eigenvalues
-- LOW, a bulk uniform in [1, 2], and `high` -- are dealt to the rows by a random permutation, block b is Q_b diag(lam_b)
Q_b^H with Q_b the Q of qr(Gaussian), symmetrised and rounded to the type; v0 uniform(-1, 1); the reference spectrum is
eigvalsh of the blocks as stored, widened, block by block."""
import ctypes as C

import numpy as np

from _cg import BlockDiagonal
from _jacobi import CODE, set_blocks
from _krylov import ERR_DEVICE, ERR_INVALID, ERR_UNSUPPORTED, real_of, wide_of  # noqa: F401
from _submat import cut

NEIG = 400
MAX_NCV = 128  # BSM_GMRES_MAX_RESTART
LA, SA, BE, LM = 0, 1, 2, 3
WHICH = {"LA": LA, "SA": SA, "BE": BE, "LM": LM}
LOW = np.array([-3.3, -2.2, -1.5, -0.9, -0.4])
HIGH = np.array([3.0, 3.6, 4.3, 5.1, 6.0])
# for the cases with more than 5 wanted pairs: the [1, 2] bulk gives LA with nev > 5 nothing separated to converge to
HIGH40 = 3.0 + 0.4 * np.arange(40)
DTYPES = [np.float32, np.float64, np.complex64, np.complex128]
# (nev, ncv) the GPU module runs; (4, 400) is the twin's alone: the library takes ncv <= BSM_GMRES_MAX_RESTART = 128
CASES = [(4, 20), (5, 12), (1, 3), (4, 128)]


def is_complex(dtype):
    return np.dtype(dtype).kind == "c"


def eig_rtol(dtype):
    return 2e-5 if np.finfo(dtype).eps > 1e-10 else 1e-10


# ---- selection, as bsm_eig.h has it -----------------------------------------------------------------------------------------
def select(which, theta, count):
    """the `count` of the ASCENDING theta that `which` wants, in the order it reports them (0-based indices)"""
    m = len(theta)
    count = min(count, m)
    if which == LA:
        return [m - 1 - i for i in range(count)]
    if which == SA:
        return list(range(count))
    if which == BE:
        top = (count + 1) // 2
        return [m - 1 - i for i in range(top)] + list(range(count - top))
    lo, hi, out = 0, m - 1, []
    for _ in range(count):
        if abs(theta[hi]) >= abs(theta[lo]):
            out.append(hi)
            hi -= 1
        else:
            out.append(lo)
            lo += 1
    return out


def keep_of(nev, ncv):
    return min(ncv - 1, nev + (ncv - nev) // 2)


# ---- the problems -------------------------------------------------------------------------------------------------------------
_problems = {}


def spectrum(rng):
    return np.concatenate([LOW, np.sort(rng.uniform(1, 2, NEIG - 10)), HIGH])


def cut_dense(kind, D, sets):
    """the dense D as a constructor dictionary of `kind` (the cuts of _cg.cg_problem)"""
    n = len(D)
    if kind == "vbcrs":
        blocks, rs, cs = [], [], []
        for a in range(0, n, 100):
            for b in range(0, n, 100):
                blocks.append(np.asfortranarray(D[a:a + 100, b:b + 100]))
                rs.append(a + 1)
                cs.append(b + 1)
        return dict(kind="vbcrs", blocks=blocks, rowstart=np.array(rs, np.int64), colstart=np.array(cs, np.int64), size=(n, n))
    if kind == "blocksparse":
        blocks, ri, ci = [], [], []
        for a in sets:
            for b in sets:
                blocks.append(np.asfortranarray(D[np.ix_(a - 1, b - 1)]))
                ri.append(a)
                ci.append(b)
        return dict(kind="blocksparse", blocks=blocks, rowindices=ri, colindices=ci, size=(n, n))
    assert kind == "symmetric" and not is_complex(D.dtype)
    offs, ri, ci = [], [], []
    for a in range(len(sets)):
        for b in range(a):
            offs.append(np.asfortranarray(D[np.ix_(sets[a] - 1, sets[b] - 1)]))
            ri.append(sets[a])
            ci.append(sets[b])
    return dict(kind="symmetric", diagonals=set_blocks(D, sets), diagonalindices=list(sets), offdiagonals=offs, rowindices=ri,
                colindices=ci, size=(n, n))


def eig_dense(dtype):
    """-> (D of `dtype`, symmetric / Hermitian to the bit; sets; lam as designed; v0); computed once, not to be written to"""
    key = np.dtype(dtype).name
    if key not in _problems:
        rng = np.random.default_rng(3600)
        sets = cut(rng, NEIG)
        lam = spectrum(rng)
        G = rng.standard_normal((NEIG, NEIG))
        if is_complex(dtype):
            G = G + 1j * rng.standard_normal((NEIG, NEIG))
        Q, _ = np.linalg.qr(G)
        D = (Q * lam) @ Q.conj().T
        D = ((D + D.conj().T) / 2).astype(dtype)
        v0 = np.random.default_rng(1).uniform(-1, 1, NEIG).astype(dtype)
        _problems[key] = (D, sets, lam, v0)
    return _problems[key]


def eig_problem(kind, dtype):
    """-> (problem, D, v0)"""
    D, sets, _, v0 = eig_dense(dtype)
    return cut_dense(kind, D, sets), D, v0


_refs = {}


def stored_eigenvalues(D):
    """eigvalsh of the matrix AS STORED (the type's values, widened), ascending; cached by identity of D"""
    key = id(D)
    if key not in _refs:
        _refs[key] = (D, np.linalg.eigvalsh(D.astype(wide_of(D.dtype))))
    return _refs[key][1]


def tridiagonal_block(dtype):
    """-> (vbcrs problem of order 12, D, e_1): diag(T3, B) with T3 = tridiag(diag (1, -2, 3), off-diagonals (2, 1/2)) and B a
    symmetric 9 x 9 block with the spectrum 10 .. 18.  Lanczos from e_1 reproduces T3 EXACTLY in any precision and any order
    of summation -- every product is a number times 1, every sum has one nonzero term, the norms are powers of two -- and
    beta_2 is exactly zero: the invariant subspace of dimension 3."""
    T3 = np.array([[1, 2, 0], [2, -2, 0.5], [0, 0.5, 3]])
    rng = np.random.default_rng(77)
    Q, _ = np.linalg.qr(rng.standard_normal((9, 9)))
    B = (Q * np.arange(10.0, 19.0)) @ Q.T
    B = (B + B.T) / 2
    D = np.zeros((12, 12))
    D[:3, :3], D[3:, 3:] = T3, B
    D = D.astype(dtype)
    p = dict(kind="vbcrs", blocks=[np.asfortranarray(D[:3, :3]), np.asfortranarray(D[3:, 3:])], rowstart=np.array([1, 4], np.int64),
             colstart=np.array([1, 4], np.int64), size=(12, 12))
    e1 = np.zeros(12, dtype)
    e1[0] = 1
    return p, D, e1


# ---- the grid problems: several workgroups on a vector ------------------------------------------------------------------------
class HermitianBlocks(BlockDiagonal):
    """_cg.BlockDiagonal with what the twin and the acceptance ask of a dense array besides: len, dtype, products with
    matrices (column by column the product with a vector), and the spectrum block by block"""

    @property
    def dtype(self):
        return self.main.dtype

    def __len__(self):
        return self.main.shape[0] * self.main.shape[1] + self.tail.shape[0]

    def astype(self, dtype):
        return HermitianBlocks(self.main.astype(dtype), self.tail.astype(dtype))

    def times(self, v, order=None):
        if np.ndim(v) == 1:
            return BlockDiagonal.times(self, v, order)
        assert order is None
        nb, bs, _ = self.main.shape
        out = np.empty_like(v)
        out[:nb * bs] = np.einsum("bij,bjk->bik", self.main, v[:nb * bs].reshape(nb, bs, -1)).reshape(nb * bs, -1)
        out[nb * bs:] = self.tail @ v[nb * bs:]
        return out

    def shifted(self, shift):
        """diag(blocks) + shift I, rounded to the blocks' type"""
        eye, eyet = np.eye(self.main.shape[1]), np.eye(self.tail.shape[0])
        return HermitianBlocks((self.main + shift * eye).astype(self.dtype), (self.tail + shift * eyet).astype(self.dtype))

    def eigenvalues(self):
        """eigvalsh of the blocks AS STORED (widened), ascending"""
        wide = wide_of(self.dtype)
        tail = [np.linalg.eigvalsh(self.tail.astype(wide))] if self.tail.size else []
        return np.sort(np.concatenate([np.linalg.eigvalsh(self.main.astype(wide)).ravel()] + tail))


def grid_sizes(dtype):
    """(n with krylov_grid = 2, n with krylov_grid = 3): one row more than a row range of 8192 bytes, and three more than two
    of them -- odd, so that the padded leading dimension of the workspace differs from n in every type but complex128"""
    r0 = 8192 // np.dtype(dtype).itemsize
    return r0 + 1, 2 * r0 + 3


_grid_problems = {}


def grid_eig_problem(dtype, n, high, seed):
    """-> (vbcrs problem, HermitianBlocks, ref: its spectrum as stored, ascending, v0) (module docstring); computed once, not to
    be written to"""
    dtype, high = np.dtype(dtype), np.asarray(high, dtype=float)
    key = (dtype.name, n, high.tobytes(), seed)
    if key not in _grid_problems:
        rng = np.random.default_rng(seed)
        bs, nb, t = 8, n // 8, n % 8
        lam = np.concatenate([LOW, rng.uniform(1, 2, n - len(LOW) - len(high)), high])[rng.permutation(n)]

        def blocks(lams, k):
            G = rng.standard_normal((len(lams), k, k))
            if is_complex(dtype):
                G = G + 1j * rng.standard_normal((len(lams), k, k))
            out = np.empty(G.shape, dtype)
            for b in range(len(lams)):
                Q, _ = np.linalg.qr(G[b])
                B = (Q * lams[b]) @ Q.conj().T
                out[b] = ((B + B.conj().T) / 2).astype(dtype)
            return out
        main = blocks(lam[:nb * bs].reshape(nb, bs), bs)
        tail = blocks(lam[nb * bs:].reshape(1, t), t)[0] if t else np.zeros((0, 0), dtype)
        v0 = rng.uniform(-1, 1, n).astype(dtype)
        blks = [np.asfortranarray(main[b]) for b in range(nb)] + ([np.asfortranarray(tail)] if t else [])
        starts = np.arange(len(blks), dtype=np.int64) * bs + 1
        p = dict(kind="vbcrs", blocks=blks, rowstart=starts, colstart=starts.copy(), size=(n, n))
        Dop = HermitianBlocks(main, tail)
        _grid_problems[key] = (p, Dop, Dop.eigenvalues(), v0, lam)
    return _grid_problems[key][:4]


# name -> (the outliers above the bulk, the seed's base: the generator is default_rng(base + n))
SPECTRA = {"high": (HIGH, 3700), "high20": (HIGH40[:20], 3900), "high40": (HIGH40, 4100)}
# (nev, ncv, which) at both grid sizes of every type, on "high"; (1, 3) restarts 24 .. 59 times, (4, 20) would not restart
GRID_CASES = [(5, 12, "LA"), (5, 12, "BE"), (3, 8, "LM"), (1, 3, "SA")]
# (nev, ncv, which, spectrum) at the G = 2 size: true-residual batches of 16 + 1 and 16 + 16 + 1
BATCH_CASES = [(17, 24, "LA", "high20"), (33, 48, "LA", "high40"), (33, 40, "LA", "high40")]
# The single types once more at a LOOSE tolerance.  At eig_rtol = 2e-5 their residuals are of the size of the acceptance's
# |true - residual| <= 1e-5 anorm, which a residual that lost a workgroup's share therefore passes; at 1e-2 the last pair's
# residual is some 5e-3 anorm and the share of the last row range some 5e-4 anorm of it (pinned in test_eigsh_grid_cpu.py)
LOOSE_RTOL, LOOSE_CASE, LOOSE_TYPES = 1e-2, (3, 8, "LM"), [np.float32, np.complex64]
# what test_gpu_eigsh_grid.py runs besides: (dtype, n index, nev, ncv, which, spectrum)
EXTRA_CASES = [(np.float64, 1, 5, 12, "LM", "high"), (np.complex128, 1, 5, 12, "LA", "high")]


def grid_problem(dtype, n, spec="high"):
    high, base = SPECTRA[spec]
    return grid_eig_problem(dtype, n, high, base + n)


def all_grid_cases():
    """[(dtype, n, nev, ncv, which, spectrum)]: every solve of test_gpu_eigsh_grid.py on a grid problem"""
    out = []
    for dt in DTYPES:
        sizes = grid_sizes(dt)
        out += [(dt, n, nev, ncv, which, "high") for n in sizes for nev, ncv, which in GRID_CASES]
        out += [(dt, sizes[0]) + c for c in BATCH_CASES]
    out += [(dt, grid_sizes(dt)[i]) + tuple(c) for dt, i, *c in EXTRA_CASES]
    seen, uniq = set(), []
    for c in out:
        k = grid_id(c)
        if k not in seen:
            seen.add(k)
            uniq.append(c)
    return uniq


def grid_id(c):
    dt, n, nev, ncv, which, spec = c
    return f"{np.dtype(dt).name}-n{n}-{nev}of{ncv}-{which}-{spec}"


_grid_twins = {}


def grid_twin(dtype, n, nev, ncv, which, spec="high", rtol=None):
    """the twin on grid_problem(dtype, n, spec) at rtol (None: eig_rtol(dtype)) from the problem's v0; computed once"""
    key = (grid_id((dtype, n, nev, ncv, which, spec)), rtol)
    if key not in _grid_twins:
        _, Dop, _, v0 = grid_problem(dtype, n, spec)
        _grid_twins[key] = eigsh_twin(Dop, v0, nev, ncv, which, eig_rtol(dtype) if rtol is None else rtol, dtype=dtype)
    return _grid_twins[key]


# ---- the twin -----------------------------------------------------------------------------------------------------------------
class EigTwin:
    pass


def eigsh_twin(D, v0, nev, ncv, which, rtol, atol=0.0, maxcycles=300, dtype=None):
    """numpy twin of bsm_eigsh_solve (module docstring) on a dense array or a HermitianBlocks operator -> EigTwin: status, nconv, cycles, steps, anorm, value, estimate,
    residual (||D x - theta x|| in `dtype` arithmetic, norm in double), X (n x nconv), orth = max |X^H X - I|"""
    dtype = np.dtype(D.dtype if dtype is None else dtype)
    real = real_of(dtype)
    which = WHICH.get(which, which)
    D = D.astype(dtype) if isinstance(D, BlockDiagonal) else np.asarray(D).astype(dtype)
    n = len(D)
    assert 1 <= nev and nev + 2 <= ncv <= n
    V = np.zeros((n, ncv + 1), dtype)
    out = EigTwin()
    out.status, out.nconv, out.cycles, out.steps, out.anorm = None, 0, 0, 0, 0.0
    out.value = out.estimate = out.residual = np.zeros(0)
    out.X, out.orth = np.zeros((n, 0), dtype), 0.0

    def norm(v):
        return real.type(np.linalg.norm(v))

    def scaled(w, b):
        if not (b > 0 and np.isfinite(b)):
            return np.zeros_like(w)
        return (w * real.type(1 / b)).astype(dtype)

    with np.errstate(all="ignore"):
        b0 = norm(np.asarray(v0).astype(dtype))
        V[:, 0] = scaled(np.asarray(v0).astype(dtype), b0)
        start, kept, arrow = 0, np.zeros(0), np.zeros(0)
        alpha, beta = np.zeros(ncv), np.zeros(ncv)
        idx, beta_m, theta, S, d = [], 0.0, np.zeros(0), np.zeros((0, 0)), 0
        while True:
            out.cycles += 1
            for j in range(start, ncv):
                w = (D @ V[:, j]).astype(dtype)
                hsum = np.zeros(j + 1, dtype)
                for _ in range(2):
                    h = (V[:, :j + 1].conj().T @ w).astype(dtype)
                    w = (w - V[:, :j + 1] @ h).astype(dtype)
                    hsum = (hsum + h).astype(dtype)
                alpha[j] = float(hsum[j].real)
                beta[j] = float(norm(w))
                V[:, j + 1] = scaled(w, real.type(beta[j]))
                out.steps += 1
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
            T = np.zeros((d, d))
            for i in range(start):
                T[i, i] = kept[i]
                T[i, start] = T[start, i] = arrow[i]
            for j in range(start, d):
                T[j, j] = alpha[j]
                if j + 1 < d:
                    T[j, j + 1] = T[j + 1, j] = beta[j]
            theta, S = np.linalg.eigh(T)
            if not np.all(np.isfinite(theta)):
                out.status = 2
                break
            out.anorm = max(out.anorm, float(np.max(np.abs(theta))))
            beta_m = beta[d - 1]
            if d < ncv:
                out.nconv = min(nev, d)
                out.status = 0 if d >= nev else 3
                idx = select(which, theta, out.nconv)
                break
            idx = select(which, theta, nev)
            tol = max(rtol * out.anorm, atol)
            done = all(abs(beta_m * S[d - 1, i]) <= tol for i in idx)
            if done or out.cycles >= maxcycles:
                out.status, out.nconv = (0 if done else 1), nev
                break
            keep = keep_of(nev, ncv)
            idx = select(which, theta, keep)
            Sk = S[:, idx].astype(real)
            carried = V[:, ncv].copy()
            V[:, :keep] = combine_reference(V[:, :ncv], Sk, dtype)
            V[:, keep] = carried
            kept, arrow, start = theta[idx], beta_m * S[d - 1, idx], keep
        if out.nconv:
            out.value = theta[idx]
            out.estimate = np.abs(beta_m * S[d - 1, idx])
            out.X = combine_reference(V[:, :d], S[:, idx].astype(real), dtype)
            R = (D @ out.X).astype(dtype) - (out.X * out.value.astype(real)).astype(dtype)
            out.residual = np.linalg.norm(R.astype(wide_of(dtype)), axis=0)
            Xw = out.X.astype(wide_of(dtype))
            out.orth = float(np.max(np.abs(Xw.conj().T @ Xw - np.eye(out.nconv))))
    return out


def combine_reference(V, S, dtype):
    """V S with the sum over j ascending, one multiply-add per term rounded to `dtype` (numpy has no fma: the product is
    rounded too, which the error bound of the GPU test does not rely on)"""
    dtype = np.dtype(dtype)
    out = np.zeros((V.shape[0], S.shape[1]), dtype)
    for j in range(V.shape[1]):
        out = (out + V[:, j:j + 1].astype(dtype) * S[j:j + 1, :].astype(real_of(dtype))).astype(dtype)
    return out


_twins = {}


def twin_of(dtype, nev, ncv, which, maxcycles=300):
    """the twin on the order-400 problem of `dtype` at eig_rtol(dtype) from the problem's v0; computed once"""
    key = (np.dtype(dtype).name, nev, ncv, which, maxcycles)
    if key not in _twins:
        D, _, _, v0 = eig_dense(dtype)
        _twins[key] = eigsh_twin(D, v0, nev, ncv, which, eig_rtol(dtype), 0.0, maxcycles, dtype)
    return _twins[key]


# ---- what both suites accept ----------------------------------------------------------------------------------------------
def wanted_reference(ref, which, count):
    """the `count` eigenvalues of the ascending reference spectrum `which` wants, in its order"""
    return ref[select(WHICH.get(which, which), ref, count)]


def check_pairs(value, estimate, residual, anorm, ref, which, tol, dtype, what):
    """the two inequalities of the issue, per pair:  |theta_i - lam_i| <= residual_i + n eps anorm  (the Hermitian residual
    bound plus the backward error of the dense reference, n = 400) and  residual_i <= tol + |residual_i - estimate_i|.
    -> the largest gap |residual - estimate| / (eps anorm)"""
    eps = float(np.finfo(dtype).eps)
    lam = wanted_reference(ref, which, len(value))
    gap = 0.0
    for i in range(len(value)):
        err, bound = abs(value[i] - lam[i]), residual[i] + len(ref) * eps * anorm
        g = abs(residual[i] - estimate[i])
        gap = max(gap, g / (eps * anorm))
        print(f"EIGSTAT {what} pair {i}: theta {value[i]:+.12f} lam {lam[i]:+.12f} |theta - lam| {err:.3e} bound {bound:.3e} "
              f"residual {residual[i]:.3e} estimate {estimate[i]:.3e} gap / (eps anorm) {g / (eps * anorm):.2f}")
        assert err <= bound, (what, i, err, bound)
        assert residual[i] <= tol + g, (what, i, residual[i], tol, g)
    return gap


def steps_of(nev, ncv, cycles):
    return ncv + (cycles - 1) * (ncv - keep_of(nev, ncv))


def accept(torch, w, X, info, D, n, twin, nev, ncv, which, dtype, what, ref=None, rtol=None):
    """the acceptance of a converged device solve (docstring of test_gpu_eigsh.py).  D: the operator of order n, a dense array
    or HermitianBlocks (then with ref, its spectrum); X: a torch tensor"""
    from _gpu import TOL
    dtype = np.dtype(dtype)
    eps = float(np.finfo(dtype).eps)
    ref = stored_eigenvalues(D) if ref is None else ref
    assert len(D) == n == len(ref)
    assert twin.status == 0, (what, "the twin did not converge")
    assert info.status == 0 and info.nconv == nev == len(w), (what, info)
    tol = (eig_rtol(dtype) if rtol is None else rtol) * info.anorm
    assert np.all(info.estimate <= tol), (what, info.estimate, tol)
    gap = check_pairs(w, info.estimate, info.residual, info.anorm, ref, which, tol, dtype, what)
    # the derived bound of test_eigsh_cpu.py on |residual - estimate|: forming X = V S ((ncv + 1) eps |V| |S| ||A||) and the product
    # (n eps ||A||).  With estimate <= tol it is what makes the residual of the returned X small.
    gap_bound = n + ncv + 2
    assert gap <= gap_bound, (what, gap, gap_bound)
    Xh = X.cpu().numpy().astype(wide_of(dtype))
    true = np.linalg.norm(D.astype(wide_of(dtype)) @ Xh - Xh * w, axis=0)
    print(f"EIGSTAT {what}: gap / (eps anorm) {gap:.2f} of {gap_bound}, max |true - residual| / anorm {np.max(np.abs(true - info.residual)) / info.anorm:.3e} "
          f"of {TOL[dtype]:.0e}, max |true - estimate| / (eps anorm) {np.max(np.abs(true - info.estimate)) / (eps * info.anorm):.2f} of {gap_bound}, "
          f"max estimate / tol {np.max(info.estimate) / tol:.3e}")
    assert np.all(np.abs(true - info.residual) <= TOL[dtype] * info.anorm), (what, true, info.residual)
    assert np.all(np.abs(true - info.estimate) <= gap_bound * eps * info.anorm), (what, true, info.estimate)
    assert np.all(true <= tol + gap_bound * eps * info.anorm), (what, true, tol)
    orth = float(np.max(np.abs(Xh.conj().T @ Xh - np.eye(nev))))
    print(f"EIGSTAT {what}: cycles {info.cycles} (twin {twin.cycles}), orth / eps {orth / eps:.2f} (twin {twin.orth / eps:.2f}, margin used "
          f"{orth / twin.orth if twin.orth else float('inf'):.2f} of 8), anorm {info.anorm:.6f}, a_products {info.a_products}")
    assert orth <= 8 * twin.orth, (what, orth / eps, twin.orth / eps)
    assert info.cycles <= twin.cycles + 1, (what, info.cycles, twin.cycles)
    assert info.a_products == steps_of(nev, ncv, info.cycles) + nev, (what, info.a_products)
    assert info.anorm <= float(np.max(np.abs(ref))) * (1 + n * eps)  # a lower bound of ||A||_2, up to the error of both sides


# ---- raw ctypes drivers --------------------------------------------------------------------------------------------------
def raw_combine(code, n, m, k, V, ldv, S, lds, Out, ldo, carry, stream=None):
    from bsm_amd import _lib as L
    return L.lib().bsm_krylov_combine(code, n, m, k, V, ldv, S, lds, Out, ldo, carry, stream)


def raw_eigsh_create(A, opA, code, nev, ncv, null_out=False):
    """bsm_eigsh_create as C sees it -> (return code, solver pointer); a created solver is destroyed by the caller"""
    from bsm_amd import _lib as L
    out = C.c_void_p(0xdead)
    rc = L.lib().bsm_eigsh_create(None if A is None else A._h.ptr, opA, code, nev, ncv, None if null_out else C.byref(out))
    return rc, out


def raw_eigsh_destroy(ptr):
    from bsm_amd import _lib as L
    return L.lib().bsm_eigsh_destroy(ptr)


def raw_eigsh_solve(ptr, nev, v0, X, ldx, which=LA, rtol=1e-10, atol=0.0, maxcycles=300, vectors=1, memspace=1, stream=None,
                    struct_size=None, null=()):
    """bsm_eigsh_solve as C sees it (v0, X: addresses) -> (return code, info, pairs); null: names of p / info / pairs to pass as
    NULL"""
    from bsm_amd import _lib as L
    p = L.BsmEigshParams(C.sizeof(L.BsmEigshParams) if struct_size is None else struct_size, which, rtol, atol, maxcycles, vectors)
    info = L.BsmEigshInfo()
    pairs = (L.BsmEigshPair * max(nev, 1))()
    rc = L.lib().bsm_eigsh_solve(ptr, v0, X, ldx, None if "p" in null else C.byref(p), None if "info" in null else C.byref(info),
                                 None if "pairs" in null else pairs, memspace, stream)
    return rc, info, pairs


def raw_jacobi(T):
    """the unexported test hook bsm_debug_eig_jacobi (csrc/bsm_eig.cpp) -> (theta ascending, S)"""
    from bsm_amd import _lib as L
    fn = L.lib().bsm_debug_eig_jacobi
    dp = C.POINTER(C.c_double)
    fn.argtypes = [C.c_int32, dp, C.c_int64, dp, dp]
    fn.restype = C.c_int
    T = np.asfortranarray(T, dtype=np.float64)
    m = len(T)
    theta, S = np.zeros(m), np.zeros((m, m), order="F")
    rc = fn(m, T.ctypes.data_as(dp), m, theta.ctypes.data_as(dp), S.ctypes.data_as(dp))
    assert rc == 0
    return theta, S


def raw_select(which, theta, count):
    """the unexported test hook bsm_debug_eig_select -> 0-based indices"""
    from bsm_amd import _lib as L
    fn = L.lib().bsm_debug_eig_select
    fn.argtypes = [C.c_int, C.c_int32, C.POINTER(C.c_double), C.c_int32, C.POINTER(C.c_int32)]
    fn.restype = C.c_int
    th = np.ascontiguousarray(theta, dtype=np.float64)
    idx = np.full(max(count, 1), -1, dtype=np.int32)
    rc = fn(which, len(th), th.ctypes.data_as(C.POINTER(C.c_double)), count, idx.ctypes.data_as(C.POINTER(C.c_int32)))
    assert rc == 0
    return idx[:count].tolist()


def raw_keep(nev, ncv):
    from bsm_amd import _lib as L
    fn = L.lib().bsm_debug_eig_keep
    fn.argtypes = [C.c_int32, C.c_int32]
    fn.restype = C.c_int
    return fn(nev, ncv)
