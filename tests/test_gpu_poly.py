"""GPU suite of the polynomial preconditioners (bsm_poly_create / PolynomialPreconditioner): the product of a composed handle
against the numpy twin of tests/_poly.py (same recurrence, none of the code) over the layout table of the lockstep suites,
the guarded access to the caller's matrices, alpha / beta, op T / C, the (handle, vector) pairings, one pass over A and D per
step, bit-identity, live values, every solver with the composed handle as M, lanczos_bounds, and the refusals that need a
device.  The twin itself, the counts of the solver twins and the refusals that need no device are in test_poly_cpu.py.

Acceptance of a product (_poly.accept): max|M @ R - ref| in eps(dtype) max|ref|, ref the twin in _lockstep.reference_of(dtype),
bounded by _lockstep.MARGIN x the same-precision twin's spread over 8 permuted product orders.  Printed in POLYSTAT lines.

The twin's D.  The handle under test is given D = block_jacobi(A, sets), whose values are the device's own block inverses
(Gauss-Jordan in the element type: test_gpu_invert_blocks.py); the exact inverse rounded to the type differs from them by a
few eps, which one step of the recurrence hands through undamped (measured: 1.8 .. 3.9 eps max|ref| at s = 1 against a
spread of 0.9).  What is under test here is the recurrence, so the twin takes the values the handle D HOLDS, read through
D's own product with unit vectors (held_blocks / held_dense: every entry is one product with 1, exact).  The solver tests
hand their twins the exact inverse, as the solvers' own suites do: they compare counts and true residuals."""
import ctypes as C

import numpy as np
import pytest

from _bicgstab import bicgstab_twin
from _bicgstab import check_columns as bicgstab_check
from _bicgstab import check_products as bicgstab_products
from _cg import BlockDiagonal, cg_problem, column_tol, is_complex
from _common import Cc, T, wrap
from _gmres_multi import check_columns as gmres_check
from _gmres_multi import gmres_multi_twin, products as gmres_products
from _gpu import dev_copy, dev_mat, outside_bytes, torch_cuda  # noqa: F401
from _jacobi import CODE, uniform
from _krylov import ERR_UNSUPPORTED, exact_minv, rtol_of, wide_of
from _lockstep import COLUMNS, MARGIN, TABLE, TABLE_IDS, grid_case, half_sets, nonsym_problem, path_rtol, reference_of, solvers
from _poly import accept, dense_poly, deviation, half_inverse, neumann_coefficients, poly_twin, raw_destroy, raw_poly_create, twin_spread
from _values import copied, diagonal_shift

pytestmark = pytest.mark.gpu

STEPS = [1, 2, 5]
# (family, problem of _lockstep.grid_case, with D = block_jacobi over half_sets(n))
CONFIGS = [(f, m, d) for f, m in (("chebyshev", "cg"), ("neumann", "cg"), ("neumann", "bicgstab")) for d in (False, True)]
CONFIG_IDS = [f"{f}-{m}-{'D' if d else 'noD'}" for f, m, d in CONFIGS]


def name(dtype):
    return np.dtype(dtype).name


def coefficients(bsm, family, steps, with_d):
    """Nominal coefficients for the grid problems (blocks T^H T + I of order 8: spectrum in [1, 24]; with the block-Jacobi D
    over the half blocks the spectrum of D A lies in (0, 2)).  The product is checked, not the quality of the polynomial."""
    if family == "chebyshev":
        return bsm.chebyshev_coefficients(*((0.25, 2.0) if with_d else (1.0, 24.0)), steps)
    return neumann_coefficients(0.8 if with_d else 0.05, steps)


_handles = {}


def grid_handles(bsm, method, n, dtype):
    """(A, block_jacobi(A, half_sets(n))) of _lockstep.grid_case, built once per problem"""
    key = (method, n, name(dtype))
    if key not in _handles:
        A = bsm.synthetic.build(grid_case(method, n, dtype)[0])
        _handles[key] = (A, bsm.block_jacobi(A, half_sets(n)))
    return _handles[key]


def held_dense(torch, H, n, dtype):
    """the dense values a handle holds, by its product with the identity"""
    return apply(torch, H, np.asfortranarray(np.eye(n, dtype=dtype)))


def held_blocks(torch, Dj, n, dtype):
    """the values of block_jacobi(A, half_sets(n)) as the handle holds them -> BlockDiagonal of blocks of order 4 (the tail
    block whole).  Eight probe columns, X[i, i mod 8] = 1: the blocks start at multiples of 4, the tail at a multiple of 8"""
    X = np.zeros((n, 8), dtype=dtype, order="F")
    X[np.arange(n), np.arange(n) % 8] = 1
    Y = apply(torch, Dj, X)
    nb, t = n // 8, n % 8
    Yb = Y[:8 * nb].reshape(nb, 8, 8)
    main = np.stack([Yb[:, :4, :4], Yb[:, 4:, 4:]], axis=1).reshape(2 * nb, 4, 4)
    return BlockDiagonal(np.ascontiguousarray(main), np.ascontiguousarray(Y[8 * nb:, :t]))


def apply(torch, M, R, K=None):
    """M @ (the first K columns of R) on the device -> numpy"""
    Rk = R if K is None else np.asfortranarray(R[:, :K])
    Y = M @ dev_copy(torch, Rk)
    torch.cuda.synchronize()
    return Y.cpu().numpy()


# ---- 1. the product against the twin over the layout table ----------------------------------------------------------------
@pytest.mark.parametrize("config", CONFIGS, ids=CONFIG_IDS)
@pytest.mark.parametrize("dtype, n, G", TABLE, ids=TABLE_IDS)
def test_apply_against_the_twin(torch_cuda, bsm, dtype, n, G, config):
    torch, (family, method, with_d) = torch_cuda, config
    p, Dop, B = grid_case(method, n, dtype)
    A, Dj = grid_handles(bsm, method, n, dtype)
    Dinv = held_blocks(torch, Dj, n, dtype) if with_d else None
    if with_d:  # a sanity check of the read-out, not of the inversion: what D holds IS the block inverse
        exact = half_inverse(Dop)
        assert np.max(np.abs(Dinv.main - exact.main)) <= 1024 * np.finfo(dtype).eps * np.max(np.abs(exact.main))
        assert Dinv.tail.shape == exact.tail.shape and np.allclose(Dinv.tail, exact.tail, rtol=0, atol=1024 * np.finfo(dtype).eps * np.max(np.abs(exact.main)))
    for steps in STEPS:
        a, b = coefficients(bsm, family, steps, with_d)
        M = bsm.polynomial(A, a, b, D=Dj if with_d else None)
        assert M.steps == steps and M.size == (n, n) and M.dtype == np.dtype(dtype)
        got = {K: apply(torch, M, B, K) for K in COLUMNS}
        what = f"{CONFIG_IDS[CONFIGS.index(config)]} {name(dtype)} n={n} G={G} s={steps}"
        # one reference on all 16 columns; the spread from column 0
        dev, s, ref = accept(got[16], Dop, Dinv, a, b, B, dtype, what + " K=16")
        for K in COLUMNS[:-1]:  # the same columns in narrower products: the same reference, the same bound
            d = deviation(got[K], ref[:, :K], dtype)
            print(f"POLYSTAT {what} K={K}: deviation {d:.3f}, bound {MARGIN * s:.3f}")
            assert d <= MARGIN * s, (what, K, d, s)


@pytest.mark.parametrize("dtype", [np.float64, np.complex64], ids=name)
@pytest.mark.parametrize("K", [17, 35])
def test_more_columns_than_the_workspace_run_in_batches(torch_cuda, bsm, dtype, K):
    torch, n = torch_cuda, 203
    p, Dop, _ = grid_case("cg", n, dtype)
    A, Dj = grid_handles(bsm, "cg", n, dtype)
    R = np.asfortranarray(uniform(np.random.default_rng(9300 + K), (n, K), dtype))
    a, b = coefficients(bsm, "chebyshev", 5, True)
    for nrhs in (16, 4):
        M = bsm.polynomial(A, a, b, D=Dj, nrhs=nrhs)
        accept(apply(torch, M, R), Dop, held_blocks(torch, Dj, n, dtype), a, b, R, dtype, f"batches {name(dtype)} K={K} nrhs_max={nrhs}")


# ---- 2. guarded buffers, alpha / beta -----------------------------------------------------------------------------------------
ALPHA_BETA = [(1, False), (1, 0.0), (-0.5, 2.0), (0.5 - 1.5j, 2.0 + 1.0j)]


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.complex64, np.complex128], ids=name)
@pytest.mark.parametrize("with_d", [False, True], ids=["noD", "D"])
def test_guarded_buffers_and_scalars(torch_cuda, bsm, dtype, with_d):
    """X at ldx = n + 3, Y one element past a 16-byte boundary with ldy = n + 1, both inside NaN-filled buffers: every byte
    outside the n x nrhs window of Y keeps its bits and X is unchanged.  y = alpha p(A) x + beta y against alpha twin + beta y0:
    the scaling adds one rounding per product and sum (two products and a sum more for complex scalars) to the twin's, so the
    bound is the acceptance's plus 4 units of eps max|result| (8 for complex scalars)."""
    torch, n, K = torch_cuda, 203, 3
    p, Dop, B = grid_case("cg", n, dtype)
    A, Dj = grid_handles(bsm, "cg", n, dtype)
    Dinv = held_blocks(torch, Dj, n, dtype) if with_d else None
    R = np.asfortranarray(B[:, :K])
    Y0 = np.asfortranarray(B[:, K:2 * K])
    a, b = coefficients(bsm, "chebyshev", 5, with_d)
    M = bsm.polynomial(A, a, b, D=Dj if with_d else None)
    for alpha, beta in ALPHA_BETA:
        if np.iscomplexobj(alpha) and not is_complex(dtype):
            continue
        strong = beta is False
        xbuf, xview = dev_mat(torch, R, pad=3, guard=5)
        ybuf, yview = dev_mat(torch, np.full((n, K), np.nan, dtype=dtype) if strong else Y0, pad=1, off=1, guard=5)
        before = (outside_bytes(ybuf, n, n + 1, K, off=1), xbuf.cpu().numpy().tobytes())
        bsm.mul(yview, M, xview, alpha, beta)
        torch.cuda.synchronize()
        assert outside_bytes(ybuf, n, n + 1, K, off=1) == before[0], "Y was written outside its n x nrhs window"
        assert xbuf.cpu().numpy().tobytes() == before[1], "X was written"
        got = yview.cpu().numpy()
        assert np.all(np.isfinite(got)), (alpha, beta)
        what = f"guarded {name(dtype)} {'D' if with_d else 'noD'} alpha={alpha} beta={beta}"
        if alpha == 1 and strong:
            accept(got, Dop, Dinv, a, b, R, dtype, what)
            continue
        wide, rt = wide_of(dtype), reference_of(dtype)
        z = poly_twin(Dop.astype(rt), None if Dinv is None else Dinv.astype(rt), a, b, R.astype(rt), rt).astype(wide)
        want = wide(alpha) * z + (0 if strong else wide(beta) * Y0.astype(wide))
        unit = np.finfo(dtype).eps * np.max(np.abs(want))
        s = twin_spread(Dop, Dinv, a, b, R[:, 0], dtype, z[:, 0]) * np.max(np.abs(z[:, 0])) * abs(alpha) / np.max(np.abs(want))
        extra = 8 if np.iscomplexobj(alpha) else 4
        dev = float(np.max(np.abs(got - want)) / unit)
        print(f"POLYSTAT {what}: deviation {dev:.3f}, bound {MARGIN * s + extra:.3f} (eps max|result|)")
        assert dev <= MARGIN * s + extra, (what, dev, s)


# ---- 3. op T / C on the composed handle ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.complex128, np.complex64], ids=name)
@pytest.mark.parametrize("op", [T, Cc], ids=["T", "C"])
def test_transpose_and_adjoint_of_the_composed_handle(torch_cuda, bsm, dtype, op):
    """the same recurrence on the transposed / adjoint dense operators (the coefficients are real)"""
    torch, n, K = torch_cuda, 203, 3
    p, Dop, B = grid_case("bicgstab", n, dtype)
    A, Dj = grid_handles(bsm, "bicgstab", n, dtype)
    Dd = Dop.dense()
    Di = held_dense(torch, Dj, n, dtype)
    flip = (lambda X: np.ascontiguousarray(X.T)) if op == T else (lambda X: np.ascontiguousarray(X.conj().T))
    R = np.asfortranarray(B[:, :K])
    for family, with_d in (("neumann", True), ("chebyshev", False)):
        a, b = coefficients(bsm, family, 5, with_d)
        M = bsm.polynomial(A, a, b, D=Dj if with_d else None)
        Y = wrap(bsm, M, op) @ dev_copy(torch, R)
        torch.cuda.synchronize()
        accept(Y.cpu().numpy(), flip(Dd), flip(Di) if with_d else None, a, b, R, dtype, f"op {'T' if op == T else 'C'} {name(dtype)} {family}")
    # ops compose: the polynomial of transpose(A) applied transposed is the polynomial of A
    a, b = coefficients(bsm, "neumann", 3, True)
    Mt = bsm.polynomial(wrap(bsm, A, op), a, b, D=wrap(bsm, Dj, op))
    Y = wrap(bsm, Mt, op) @ dev_copy(torch, R)
    torch.cuda.synchronize()
    accept(Y.cpu().numpy(), Dd, Di, a, b, R, dtype, f"op on op {name(dtype)}")
    if is_complex(dtype):  # T on C would need conj(A)
        with pytest.raises(bsm._lib.BsmError, match="conj"):
            wrap(bsm, Mt, T if op == Cc else Cc) @ dev_copy(torch, R)


# ---- 4. pairings ------------------------------------------------------------------------------------------------------------------
def test_real_handles_under_complex_vectors(torch_cuda, bsm):
    torch, n, K, dtype = torch_cuda, 203, 3, np.complex128
    p, Dop, _ = grid_case("cg", n, np.float64)
    A, Dj = grid_handles(bsm, "cg", n, np.float64)
    R = np.asfortranarray(uniform(np.random.default_rng(9310), (n, K), dtype))
    a, b = coefficients(bsm, "chebyshev", 5, True)
    M = bsm.polynomial(A, a, b, D=Dj, dtype=dtype)
    got = apply(torch, M, R)
    Dinv = held_blocks(torch, Dj, n, np.float64)
    for part, x in (("real", np.asfortranarray(R.real)), ("imaginary", np.asfortranarray(R.imag))):
        accept(got.real if part == "real" else got.imag, Dop, Dinv, a, b, x, np.float64, f"real A, D under complex128, {part} part")
    # a composed handle of real vectors takes no complex ones
    Mr = bsm.polynomial(A, a, b, D=Dj)
    with pytest.raises(bsm._lib.BsmError, match="complex vdtype"):
        Mr @ dev_copy(torch, R)


def test_mixed_storage_transposed_image_and_coloured_operators(torch_cuda, bsm):
    torch, n, K, dtype = torch_cuda, 203, 3, np.float64
    p, Dop, B = grid_case("bicgstab", n, dtype)
    R = np.asfortranarray(B[:, :K])
    a, b = neumann_coefficients(0.05, 5)
    # values stored in float32 under float64 vectors: the twin on the rounded operator
    M = bsm.polynomial(bsm.synthetic.build(p, storage=np.float32), a, b)
    rounded = BlockDiagonal(Dop.main.astype(np.float32).astype(dtype), Dop.tail.astype(np.float32).astype(dtype))
    accept(apply(torch, M, R), rounded, None, a, b, R, dtype, "storage=float32 A under float64")
    # a second ordering: transpose(A) runs forward on it
    At = bsm.synthetic.build(p, transpose_image=True)
    Dd = Dop.dense()
    M = bsm.polynomial(bsm.transpose(At), a, b)
    accept(apply(torch, M, R), np.ascontiguousarray(Dd.T), None, a, b, R, dtype, "transpose_image A, op T")
    # a coloured blocksparse operator (order 400) with its coloured block-Jacobi
    pc, sets, D, Bc = cg_problem("blocksparse", dtype)
    Ac = bsm.synthetic.build(pc, accumulate="colored")
    Dc = bsm.block_jacobi(Ac, sets, accumulate="colored")
    Mc = bsm.chebyshev(Ac, 0.3, 1.8, 4, D=Dc)
    Rc = np.asfortranarray(Bc[:, :K])
    accept(apply(torch, Mc, Rc), D, held_dense(torch, Dc, 400, dtype), Mc.a, Mc.b, Rc, dtype, "coloured A and D")


# ---- 5. one pass per step, bit-identity, live values ----------------------------------------------------------------------------
@pytest.mark.parametrize("steps", [1, 2, 5])
def test_one_pass_over_a_and_d_per_step(torch_cuda, bsm, steps):
    torch, n, dtype = torch_cuda, 203, np.float64
    p, Dop, B = grid_case("cg", n, dtype)
    A = bsm.synthetic.build(p)
    Dj = bsm.block_jacobi(A, half_sets(n))
    M = bsm.chebyshev(A, 0.25, 2.0, steps, D=Dj)
    Rd = dev_copy(torch, B)
    Y = torch.empty((16, n), dtype=Rd.dtype, device="cuda").t()
    before = A.value_passes(), Dj.value_passes()
    bsm.mul(Y, A, Rd)
    bsm.mul(Y, Dj, Rd)
    assert (A.value_passes(), Dj.value_passes()) == (before[0] + 1, before[1] + 1), "a plain 16-column product is not one pass"
    before = A.value_passes(), Dj.value_passes()
    bsm.mul(Y, M, Rd)
    torch.cuda.synchronize()
    assert A.value_passes() - before[0] == steps - 1 and Dj.value_passes() - before[1] == steps


def test_two_applies_agree_to_the_bit(torch_cuda, bsm):
    torch, dtype = torch_cuda, np.float64
    p, sets, D, B = cg_problem("vbcrs", dtype)
    A = bsm.synthetic.build(p)
    assert isinstance(A, bsm.VariableBlockCompressedRowStorage)
    M = bsm.chebyshev(A, 0.3, 1.8, 5, D=bsm.block_jacobi(A, sets))
    Rd = dev_copy(torch, B)
    one, two = M @ Rd, M @ Rd
    torch.cuda.synchronize()
    assert one.cpu().numpy().tobytes() == two.cpu().numpy().tobytes()


def test_values_are_live(torch_cuda, bsm):
    """update_blocks(A, ...) and D.refresh() are seen by the SAME composed handle; its workspace stays"""
    torch, dtype, K = torch_cuda, np.float64, 3
    p, sets, D, B = cg_problem("vbcrs", dtype)
    q = copied(p)
    A = bsm.synthetic.build(q)
    Dj = bsm.block_jacobi(A, sets)
    a, b = bsm.chebyshev_coefficients(0.3, 1.8, 4)
    M = bsm.polynomial(A, a, b, D=Dj)
    R = np.asfortranarray(B[:, :K])
    Dold = held_dense(torch, Dj, 400, dtype)
    accept(apply(torch, M, R), D, Dold, a, b, R, dtype, "before the update")
    info, stats = M.info(), M.stats()
    assert stats["nnz"] == 0 and stats["device_bytes"] == info[3] >= 5 * 16 * 400 * 8
    assert info[0] == 4 and np.array_equal(info[1], M.a) and np.array_equal(info[2], M.b)
    shift = 0.5 * np.diag(D)  # half of every diagonal entry more: the problem's rows are scaled by powers of two
    ids, new = diagonal_shift(p, shift)
    bsm.update_blocks(A, new, ids=ids)
    D2 = D + np.diag(shift)
    accept(apply(torch, M, R), D2, Dold, a, b, R, dtype, "new A, old D")
    assert deviation(apply(torch, M, R), poly_twin(D, Dold, a, b, R, dtype), dtype) > 1e6, "the update of A is not seen"
    Dj.refresh()
    Dnew = held_dense(torch, Dj, 400, dtype)
    assert np.max(np.abs(Dnew - exact_minv(D2, sets))) <= 1e-8 * np.max(np.abs(Dnew)) < np.max(np.abs(Dnew - Dold)), "D was not refreshed"
    accept(apply(torch, M, R), D2, Dnew, a, b, R, dtype, "new A, refreshed D")
    assert M.info()[3] == info[3] and M.stats() == stats


# ---- 6. every solver takes it as M ------------------------------------------------------------------------------------------------
def spectrum(D, Minv):
    ev = np.linalg.eigvals(Minv.astype(np.complex128) @ D.astype(np.complex128)).real
    return float(ev.min()), float(ev.max())


@pytest.mark.parametrize("sname", ["cg", "minres"])
@pytest.mark.parametrize("dtype", [np.float64, np.complex128], ids=name)
def test_cg_and_minres_with_the_chebyshev_polynomial(torch_cuda, bsm, sname, dtype):
    """Chebyshev, 4 steps, over the exact [0.95 lmin, 1.05 lmax] of D P (P: the operator itself; MINRES: its definite sibling,
    which the polynomial is built over -- M must be positive definite)"""
    torch, K = torch_cuda, 3
    R = solvers()[sname]
    c = R.case("vbcrs", dtype)
    A = bsm.synthetic.build(c.p)
    Ap = A if c.pm is c.p else bsm.synthetic.build(c.pm)
    Dj = bsm.block_jacobi(Ap, c.sets)
    Minv = exact_minv(c.P, c.sets)
    lmin, lmax = spectrum(c.P, Minv)
    a, b = bsm.chebyshev_coefficients(0.95 * lmin, 1.05 * lmax, 4)
    M = bsm.polynomial(Ap, a, b, D=Dj, nrhs=K)
    B = np.asfortranarray(c.B[:, :K])
    P = dense_poly(c.P, Minv, a, b, dtype)
    runs = R.runs(c.D, B, P, dtype)
    X, info = R.solve(R.make(bsm, A, M, nrhs=K), dev_copy(torch, B))
    R.accept(info, runs, c.D, X.cpu().numpy(), B, f"{sname} chebyshev s=4 {name(dtype)}")
    assert info.a_products == info.iterations and info.m_products == info.iterations + 1
    if sname == "cg":  # at most half the iterations of D alone (test_poly_cpu.py: 20 against 6 for the twin in float64)
        Xd, plain = R.solve(R.make(bsm, A, Dj, nrhs=K), dev_copy(torch, B))
        print(f"POLYSTAT cg {name(dtype)}: {int(info.iterations)} iterations with the polynomial, {int(plain.iterations)} with D alone")
        assert plain.status == 0 and 2 * int(info.iterations) <= int(plain.iterations)


@pytest.mark.parametrize("sname", ["bicgstab", "gmres_multi"])
@pytest.mark.parametrize("dtype", [np.float64, np.complex128], ids=name)
def test_bicgstab_and_gmres_with_the_neumann_polynomial(torch_cuda, bsm, sname, dtype):
    """Neumann, 3 steps, omega = 0.8, over the block-Jacobi D of half_sets on the nonsymmetric order-400 problem"""
    torch, K, n, restart = torch_cuda, 3, 400, 30
    rng = np.random.default_rng(9200)
    p, Dop = nonsym_problem(rng, n, dtype)
    B = np.asfortranarray(uniform(rng, (n, K), dtype))
    Dd = Dop.dense()
    Di = exact_minv(Dd, half_sets(n))
    a, b = neumann_coefficients(0.8, 3)
    A = bsm.synthetic.build(p)
    M = bsm.neumann(A, 0.8, 3, D=bsm.block_jacobi(A, half_sets(n)), nrhs=K)
    P = dense_poly(Dd, Di, a, b, dtype)
    rtol = rtol_of(dtype)
    Bd = dev_copy(torch, B)
    what = f"{sname} neumann s=3 {name(dtype)}"
    if sname == "bicgstab":
        runs = [bicgstab_twin(Dd, B[:, c], P, rtol, 0.0, 100, dtype) for c in range(K)]
        X, info = bsm.BiCgStab(A, M, nrhs=K).solve(Bd, rtol=rtol, maxiter=100)
        bicgstab_check(info, runs, Dd, X.cpu().numpy(), B, [column_tol(B[:, c], rtol) for c in range(K)], what)
        bicgstab_products(info, True)
    else:
        runs = [gmres_multi_twin(Dd, B[:, c], P, restart, rtol, 100, dtype) for c in range(K)]
        X, info = bsm.GmresMulti(A, M, nrhs=K, restart=restart).solve(Bd, rtol=rtol, maxiter=100)
        print(f"POLYSTAT {what}: iterations {[int(v) for v in info.column_iterations]}, twin {[r.iterations for r in runs]}")
        gmres_check(info, runs, Dd, X.cpu().numpy(), B, rtol, what)
        assert abs(int(info.iterations) - max(r.iterations for r in runs)) <= 1
        assert (info.a_products, info.m_products) == gmres_products(info, restart, False, True)


# ---- 7. lanczos_bounds -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype, herm", [(np.float64, False), (np.float32, False), (np.complex128, True)], ids=["float64", "float32", "complex128-herm"])
def test_lanczos_bounds_on_the_device_agree_with_the_numpy_core(torch_cuda, bsm, dtype, herm):
    from bsm_amd.solvers import _lanczos_ritz
    steps = 20
    p, sets, D, B = cg_problem("vbcrs", dtype, herm)
    A = bsm.synthetic.build(p)
    Dj = bsm.block_jacobi(A, sets)
    Minv = exact_minv(D, sets)
    v0 = np.random.default_rng(0).uniform(-1, 1, len(D)).astype(dtype)
    want = _lanczos_ritz(lambda v: (D @ v).astype(dtype), lambda v: (Minv @ v).astype(dtype), v0, steps, np)
    got = bsm.lanczos_bounds(A, Dj, steps=steps, v0=v0)
    assert got == bsm.lanczos_bounds(A, Dj, steps=steps)  # the default v0 is this one
    tol = path_rtol(dtype) * steps
    print(f"POLYSTAT lanczos {name(dtype)}: device {got}, numpy {want}, relative {abs(got[0] / want[0] - 1):.3e} {abs(got[1] / want[1] - 1):.3e}, bound {tol:.1e}")
    assert abs(got[0] / want[0] - 1) <= tol and abs(got[1] / want[1] - 1) <= tol
    lmin, lmax = spectrum(D, Minv)
    assert 0.95 * got[0] <= lmin and 1.05 * got[1] >= lmax


# ---- 8. refusals that need a device ---------------------------------------------------------------------------------------------
def test_refusals_on_the_device(torch_cuda, bsm):
    torch, dtype, n = torch_cuda, np.float64, 203
    Err = bsm._lib.BsmError
    p, Dop, B = grid_case("cg", n, dtype)
    A, Dj = grid_handles(bsm, "cg", n, dtype)
    a, b = neumann_coefficients(0.05, 2)
    M = bsm.polynomial(A, a, b)
    code = CODE[np.dtype(dtype)]
    # a composed handle as A or D
    for args in ((M, 0, None, 0), (A, 0, M, 0)):
        rc, out = raw_poly_create(*args, code, 1, a, b)
        assert rc == ERR_UNSUPPORTED and not out.value and "composed" in bsm._lib.lib().bsm_last_error().decode()
    with pytest.raises(Err, match="composed"):
        bsm.polynomial(M, a, b)
    # an analysis-only D under a device A
    rc, out = raw_poly_create(A, 0, bsm.block_jacobi(bsm.synthetic.build(p, device=-2), half_sets(n)), 0, code, 1, a, b)
    assert rc == -3 and not out.value
    # handles on two devices
    if torch.cuda.device_count() >= 2:
        A1 = bsm.synthetic.build(p, device=1)
        rc, out = raw_poly_create(A, 0, A1, 0, code, 1, a, b)
        assert rc == -1 and "different devices" in bsm._lib.lib().bsm_last_error().decode()
    # a handle that owns a row range only
    rc, out = raw_poly_create(bsm.synthetic.build(p, own=(1, 96)), 0, None, 0, code, 1, a, b)
    assert rc == ERR_UNSUPPORTED and not out.value
    # products: host vectors at the C level, the _cvec entries, a capturing stream
    L = bsm._lib.lib()
    x, y = np.zeros(n), np.zeros(n)
    one, zero = np.ones(1), np.zeros(1)
    assert L.bsm_mul(M._h.ptr, 0, x.ctypes.data, y.ctypes.data, one.ctypes.data, zero.ctypes.data, 1, 0, None) == ERR_UNSUPPORTED
    xd, yd = torch.zeros(n, dtype=torch.complex128, device="cuda"), torch.zeros(n, dtype=torch.complex128, device="cuda")
    assert L.bsm_mul_cvec(M._h.ptr, 0, xd.data_ptr(), yd.data_ptr(), None, None, 1, 1, None) == ERR_UNSUPPORTED
    with pytest.raises(Err, match="complex vdtype"):
        bsm.mul(yd, M, xd)
    xr, yr = torch.ones(n, dtype=torch.float64, device="cuda"), torch.zeros(n, dtype=torch.float64, device="cuda")
    # (refused before anything is enqueued, the capture stays valid: as test_gpu_cg.py does it)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        yr.zero_()
        rc = L.bsm_mul(M._h.ptr, 0, xr.data_ptr(), yr.data_ptr(), one.ctypes.data, zero.ctypes.data, 1, 1,
                       C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == ERR_UNSUPPORTED and "captured" in L.bsm_last_error().decode()
    torch.cuda.synchronize()
    bsm.mul(yr, M, xr)  # and it still works afterwards
    torch.cuda.synchronize()
    assert np.all(np.isfinite(yr.cpu().numpy()))
    # the entry accessors raise what the C refusal maps to
    for call in (lambda: M[0, 0], lambda: M[[0, 1], [0, 1]], lambda: bsm.diag(M), lambda: bsm.rowcolvals_device(M), lambda: M.value_passes(),
                 lambda: bsm.update_blocks(M, []), lambda: bsm.refresh(M)):
        with pytest.raises(Err, match="composed handle"):
            call()
    # numpy operands of M @ X are staged through torch
    Xh = np.asfortranarray(B[:, :2])
    x0 = np.ascontiguousarray(Xh[:, 0])
    assert np.array_equal(M @ Xh, apply(torch, M, Xh)) and np.array_equal(M @ x0, (M @ torch.from_numpy(x0).cuda()).cpu().numpy())
    # a solver over complex vectors takes a composed handle of real vectors as M at create and is refused at the product
    S = bsm.Cg(A, M, nrhs=1, dtype=np.complex128)
    with pytest.raises(Err, match="complex vdtype"):
        S.solve(torch.ones(n, dtype=torch.complex128, device="cuda"))
    assert raw_destroy(None) == 0
