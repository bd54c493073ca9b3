"""CPU suite of bsm_lobpcg (no GPU): the numpy twin of the solve (tests/_lobpcg.py) against eigvalsh of the matrix as stored on
every case test_gpu_lobpcg.py runs, with its iteration counts pinned; the multiplicity claim -- the twin returns every copy of a
triple eigenvalue, the single-vector eigsh_twin misses one in double --; the preconditioner claim on _cg.cg_problem; the host
Rayleigh-Ritz step (csrc/bsm_lobpcg.h, hook bsm_debug_lobpcg_rr) against the twin's, which uses numpy.linalg.eigh; the
Hermitian Jacobi eigensolver (hook bsm_debug_eig_jacobi_h); and the premise of the positive-data case of the GPU Gram test: a
lost share of the last row range exceeds its bound.  The hook tests fail without the feature: the entry points do not exist.

The preconditioner claim, measured on this twin: without M the (SA, 3, 5) solve on cg_problem takes 561 (float64), 517
(complex64) and 1970 (complex128) iterations and float32 does not converge in 2000; with the exact block-Jacobi inverse 32, 18,
37 and 13.  (The prototype the feature was designed on saw complex128 pass 2000 as well; on this twin it converges just below.
Every type needs more than ten times the preconditioned count, which is what is asserted, with the counts pinned.)"""
import numpy as np
import pytest

from _eigsh import eig_dense, eig_rtol, eigsh_twin, stored_eigenvalues, wanted_reference
from _lobpcg import (CASES, CG_CASE, DTYPES, MULT_CASE, MULT_LOW, NEIG, cg_dense, lobpcg_twin, mult_dense, raw_jacobi_h, raw_rr, rr_twin,  # noqa: F401
                     start_block, twin_of)

name = lambda d: np.dtype(d).name  # noqa: E731
EPS = float(np.finfo(np.float64).eps)

# iterations of the twin at eig_rtol from start_block: what test_gpu_lobpcg.py bounds the device's counts with (<= 2 x).
# Columns: float32, float64, complex64, complex128.
TWIN_ITERATIONS = {
    ("eig", "SA", 4, 6): (16, 19, 10, 19), ("eig", "LA", 4, 6): (18, 22, 20, 21), ("eig", "SA", 5, 5): (12, 21, 20, 22),
    ("eig", "LA", 1, 3): (12, 21, 10, 18), ("eig", "SA", 5, 16): (9, 20, 10, 19), ("mult", "SA", 4, 6): (16, 19, 15, 18),
    ("cg", "SA", 3, 5): (13, 32, 18, 37),
}
PLAIN_ITERATIONS = (2000, 561, 517, 1970)  # cg_problem without M, maxiter 2000; float32 ends with status 1


def dense_of(problem, dtype):
    return {"eig": lambda: eig_dense(dtype)[0], "mult": lambda: mult_dense(dtype)[0], "cg": lambda: cg_dense(dtype)[2]}[problem]()


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
def test_twin_against_eigvalsh_of_the_stored_matrix(dtype):
    eps = float(np.finfo(dtype).eps)
    for (problem, which, nev, block), counts in TWIN_ITERATIONS.items():
        D = dense_of(problem, dtype)
        ref = stored_eigenvalues(D)
        r = twin_of(problem, dtype, which, nev, block)
        what = f"twin {problem} {name(dtype)} {which, nev, block}"
        assert r.status == 0 and r.nconv == nev and r.X.shape == (NEIG, nev), what
        tol = eig_rtol(dtype) * r.anorm
        assert np.all(r.carried <= tol) and r.history.shape == (r.iterations + 1, nev) and np.array_equal(r.history[-1], r.carried)
        assert r.a_products == r.iterations + 2 and r.m_products == (r.iterations if problem == "cg" else 0)
        assert r.anorm <= np.max(np.abs(ref)) * (1 + NEIG * eps)
        lam = wanted_reference(ref, which, nev)
        bound = np.sqrt(nev) * float(np.max(r.true)) + NEIG * eps * r.anorm
        print(f"LOBSTAT {what}: iterations {r.iterations} drops {r.drops} max |theta - lam| {np.max(np.abs(r.value - lam)):.3e} of {bound:.3e} "
              f"drift / (eps anorm) {np.max(np.abs(r.true - r.carried)) / (eps * r.anorm):.2f} orth / eps {r.orth / eps:.2f}")
        assert np.all(np.abs(r.value - lam) <= bound), what
        assert r.iterations == counts[DTYPES.index(dtype)], (what, r.iterations)


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
def test_the_block_method_sees_every_copy_of_a_triple_eigenvalue(dtype):
    which, nev, block = MULT_CASE
    D, _, lam = mult_dense(dtype)
    assert np.array_equal(lam[:5], MULT_LOW) and np.array_equal(D, D.conj().T)
    r = twin_of("mult", dtype, which, nev, block)
    tol = np.sqrt(nev) * float(np.max(r.true)) + NEIG * float(np.finfo(dtype).eps) * r.anorm
    assert r.status == 0 and np.all(np.abs(r.value[:3] + 2) <= tol) and abs(r.value[3] + 1) <= tol, r.value
    if np.finfo(dtype).eps < 1e-10:
        # a single-vector Krylov space sees one vector of an eigenspace (rounding brings a second copy in, not the third)
        v0 = np.random.default_rng(1).uniform(-1, 1, NEIG).astype(dtype)
        e = eigsh_twin(D, v0, 4, 20, "SA", eig_rtol(dtype), dtype=dtype)
        assert e.status == 0 and e.value[2] > -1.5, e.value


def test_the_preconditioner_cuts_the_iterations_tenfold():
    which, nev, block = CG_CASE
    for dtype, pinned in zip(DTYPES, PLAIN_ITERATIONS):
        with_m = twin_of("cg", dtype, which, nev, block)
        plain = twin_of("cg-plain", dtype, which, nev, block, maxiter=2000)
        print(f"LOBSTAT preconditioner {name(dtype)}: {plain.iterations} iterations (status {plain.status}) without M, {with_m.iterations} with")
        assert with_m.status == 0 and plain.iterations == pinned, (name(dtype), plain.iterations)
        assert 10 * with_m.iterations <= plain.iterations
        assert plain.status == (1 if dtype is np.float32 else 0)


# ---- the host step against the twin's -----------------------------------------------------------------------------------------
def gram_pair(rng, p, cplx, n=300):
    """G_B = S^H S, G_A = S^H A S for a random S (n x p) whose last column nearly repeats the first, A = diag(uniform)"""
    S = rng.standard_normal((n, p)) + (1j * rng.standard_normal((n, p)) if cplx else 0)
    if p > 3:
        S[:, -1] = S[:, 0] + 1e-4 * S[:, -1]  # (lambda_min of G_B about 1e-8 / 2: far above tau lambda_max, nothing is dropped)
    S /= np.linalg.norm(S, axis=0)
    d = rng.uniform(-2, 3, n)
    return S.conj().T @ S, S.conj().T @ (d[:, None] * S)


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("p", [3, 9, 18, 48])
def test_rayleigh_ritz_hook_against_the_twin(bsm, p, cplx):
    rng = np.random.default_rng(700 + p + cplx)
    k = p // 3
    GB, GA = gram_pair(rng, p, cplx)
    use = np.ones(p, bool)
    if p > 3:
        use[k + 1] = use[2 * k] = False  # a P column and a W column out of use
    at = np.flatnonzero(use)
    cond = np.linalg.cond(GB[np.ix_(at, at)])
    bound = p * EPS * np.linalg.norm(GA[np.ix_(at, at)], 2) * cond  # the pencil's eigenvalues move by the backward error times cond(G_B)
    tau = 64 * p * EPS
    for which in ("SA", "LA"):
        st, theta, Cm, drops = raw_rr(GB, GA, use, k, which, tau)
        st2, theta2, C2, drops2, _ = rr_twin(GB, GA, use, k, which, tau)
        print(f"LOBSTAT rr p {p} {'complex' if cplx else 'real'} {which}: cond {cond:.3e} max |theta - twin| / bound {np.max(np.abs(theta - theta2)) / bound:.3e}")
        assert st == st2 == 0 and drops == drops2 == 0
        assert np.all(Cm[~use] == 0) and np.all(np.abs(theta - theta2) <= bound)
        assert np.max(np.abs(Cm.conj().T @ GB @ Cm - np.eye(k))) <= p * EPS * cond
        assert np.max(np.abs(Cm.conj().T @ GA @ Cm - np.diag(theta))) <= bound
        again = raw_rr(GB, GA, use, k, which, tau)
        assert again[1].tobytes() == theta.tobytes() and again[2].tobytes() == Cm.tobytes()


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_rayleigh_ritz_drops_the_same_directions_and_reports_the_statuses(bsm, cplx):
    rng = np.random.default_rng(810 + cplx)
    p, k, tau = 18, 6, 1e-8
    # a scaled Gram matrix with a prescribed spectrum: a gap of 1e4 on both sides of tau lambda_max
    G = rng.standard_normal((p, p)) + (1j * rng.standard_normal((p, p)) if cplx else 0)
    Q, _ = np.linalg.qr(G)
    for ndrop in (0, 1, 5):
        lam = np.concatenate([np.full(ndrop, 1e-12), rng.uniform(1e-4, 1, p - ndrop)])
        GB = (Q * lam) @ Q.conj().T
        GB = (GB + GB.conj().T) / 2
        H = rng.standard_normal((p, p)) + (1j * rng.standard_normal((p, p)) if cplx else 0)
        GA = GB @ (H + H.conj().T) @ GB
        st, theta, Cm, drops = raw_rr(GB, GA, np.ones(p, bool), k, "SA", tau)
        st2, theta2, _, drops2, _ = rr_twin(GB, GA, np.ones(p, bool), k, "SA", tau)
        assert st == st2 == 0 and drops == drops2 == ndrop, (ndrop, drops, drops2)
    # fewer than k directions kept: status 3; a diagonal entry that is not positive: 3; a NaN: 2
    lam = np.concatenate([np.full(p - k + 1, 1e-12), np.ones(k - 1)])
    GB = (Q * lam) @ Q.conj().T
    assert raw_rr(GB, GB, np.ones(p, bool), k, "SA", tau)[0] == 3 == rr_twin(GB, GB, np.ones(p, bool), k, "SA", tau)[0]
    few = np.zeros(p, bool)
    few[:k - 1] = True
    assert raw_rr(np.eye(p), np.eye(p), few, k, "LA", tau)[0] == 3
    Z = np.eye(p) + 0
    Z[2, 2] = 0
    assert raw_rr(Z, np.eye(p), np.ones(p, bool), k, "SA", tau)[0] == 3
    Z[2, 2] = np.nan
    assert raw_rr(Z, np.eye(p), np.ones(p, bool), k, "SA", tau)[0] == 2 and raw_rr(np.eye(p), Z, np.ones(p, bool), k, "SA", tau)[0] == 2


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("m", [1, 2, 3, 20, 48])
def test_hermitian_jacobi_hook(bsm, m, cplx):
    rng = np.random.default_rng(600 + m + cplx)
    G = rng.standard_normal((m, m)) + (1j * rng.standard_normal((m, m)) if cplx else 0)
    A = (G + G.conj().T) / 2
    theta, Q, sweeps = raw_jacobi_h(A)
    scale = m * EPS * np.linalg.norm(A, 2)
    print(f"LOBSTAT jacobi_h m {m} {'complex' if cplx else 'real'}: sweeps {sweeps} max |theta - ref| / scale "
          f"{np.max(np.abs(theta - np.linalg.eigvalsh(A))) / scale:.3f} ||A Q - Q diag|| / scale {np.linalg.norm(A @ Q - Q * theta, 2) / scale:.3f}")
    assert 0 <= sweeps < 60 and np.all(np.diff(theta) >= 0)
    assert np.max(np.abs(theta - np.linalg.eigvalsh(A))) <= scale
    assert np.linalg.norm(A @ Q - Q * theta, 2) <= scale
    assert np.linalg.norm(Q.conj().T @ Q - np.eye(m), 2) <= m * EPS * max(1.0, np.linalg.norm(A, 2))
    theta2, Q2, _ = raw_jacobi_h(A)
    assert theta.tobytes() == theta2.tobytes() and Q.tobytes() == Q2.tobytes()


# ---- the premise of the positive-data Gram case -------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=name)
def test_a_lost_share_exceeds_the_bound_of_the_gram_test(bsm, dtype):
    dtype = np.dtype(dtype)
    eps = float(np.finfo(dtype).eps)
    nprime = 2 if dtype.kind == "c" else 1
    r0 = 8192 // dtype.itemsize
    rng = np.random.default_rng(9400)
    for n, grid in ((r0 + 1, 2), (2 * r0 + 1, 3)):
        assert bsm.block_gram_grid(dtype, n) == grid
        per = -(-n // grid)
        U, W = rng.uniform(0, 1, (n, 5)), rng.uniform(0, 1, (n, 7))
        if dtype.kind == "c":
            U, W = U + 1j * rng.uniform(0, 1, (n, 5)), W + 1j * rng.uniform(0, 1, (n, 7))
        mod = lambda M: np.abs(M.real) + np.abs(M.imag)  # noqa: E731
        bound = (nprime * n + 2) * eps * (mod(U).T @ mod(W))
        lost = U[(grid - 1) * per:].conj().T @ W[(grid - 1) * per:]  # the share of the last row range, however short
        assert len(U[(grid - 1) * per:]) >= 1 and np.all(mod(lost) > bound), (name(dtype), n, float(np.min(mod(lost) / bound)))
