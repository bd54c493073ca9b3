"""GPU suite of bsm_block_gram, bsm_block_combine and bsm_lobpcg (-m gpu).  The Gram matrix on exact integer data (it must EQUAL
the integer product: a wrong lane map or the f64 / f32 accumulator map shows as wrong entries) and at its edges -- n = 0 and the
sizes that put 1, 2 and 3 workgroups on a column, +-1 row, odd offsets in NaN-guarded buffers -- under the bound of ANY
summation order, (n' + 2) eps |U|^T |W| with n' = n (real) / 2 n (complex) and moduli |Re| + |Im|; the combination with a complex
C at the edges of its tile under (2 p + 1) eps |V| |C|, in place with the same bits; the solves of tests/_lobpcg.py against the
numpy twin and eigvalsh of the stored matrix (accept); the multiplicity problem; block-Jacobi and Chebyshev handles as M; the
grid problems in guarded buffers; one case per kind of handle; one solver across update_blocks; the statuses; run-to-run
bytes; every refusal at the C level.  The whole module fails without the feature: the entry points do not exist there."""
import ctypes

import numpy as np
import pytest

from _eigsh import HermitianBlocks, eig_dense, eig_problem, eig_rtol, grid_problem, grid_sizes  # noqa: F401
from _gpu import dev_copy, dev_mat, outside_bytes, torch_cuda, torch_dtype  # noqa: F401
from _jacobi import CODE
from _krylov import real_of, wide_of
from _lobpcg import (CASES, CG_CASE, DTYPES, ERR_DEVICE, ERR_INVALID, ERR_UNSUPPORTED, GRID_CASES, LA, MULT_CASE, NEIG, SA, WHICH, accept,
                     cg_dense, cut_dense, lobpcg_twin, mult_dense, raw_block_combine, raw_gram, raw_lobpcg_create, raw_lobpcg_destroy,
                     raw_lobpcg_solve, start_block, twin_of)
from _values import copied, diagonal_shift, on_device

pytestmark = pytest.mark.gpu
name = lambda d: np.dtype(d).name  # noqa: E731


def mod1(M):
    """|Re| + |Im|, wide"""
    return np.abs(M.real).astype(np.float64) + np.abs(M.imag).astype(np.float64)


def integers(rng, shape, dtype):
    M = rng.integers(-3, 4, shape).astype(np.float64)
    if np.dtype(dtype).kind == "c":
        M = M + 1j * rng.integers(-3, 4, shape)
    return np.asfortranarray(M.astype(dtype))


def uniform(rng, shape, dtype, lo=-1.0):
    M = rng.uniform(lo, 1, shape)
    if np.dtype(dtype).kind == "c":
        M = M + 1j * rng.uniform(lo, 1, shape)
    return np.asfortranarray(M.astype(dtype))


def gram_sizes(bsm, dtype):
    """the row counts that put 1, 2 and 3 workgroups on a column, each +-1 row, and the grid they give"""
    r0 = 8192 // np.dtype(dtype).itemsize
    out = []
    for g in (1, 2, 3):
        for n in (g * r0 - 1, g * r0, g * r0 + 1):
            out.append((n, bsm.block_gram_grid(dtype, n)))
    assert [g for n, g in out] == [1, 1, 2, 2, 2, 3, 3, 3, 4]
    return [n for n, _ in out]


# ---- block_gram ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=name)
def test_gram_of_integer_data_is_exact(torch_cuda, bsm, dtype):
    torch = torch_cuda
    rng = np.random.default_rng(9100 + CODE[np.dtype(dtype)])
    for n in (1, 3, 4, 5, 8, 64):
        for p, q in [(1, 1), (15, 17), (16, 16), (17, 33), (48, 96)]:
            U, W = integers(rng, (n, p), dtype), integers(rng, (n, q), dtype)
            G = bsm.block_gram(dev_copy(torch, U), dev_copy(torch, W))
            torch.cuda.synchronize()
            want = U.astype(wide_of(dtype)).conj().T @ W.astype(wide_of(dtype))
            got = G.cpu().numpy()
            assert got.dtype == np.dtype(wide_of(dtype)) and got.shape == (p, q)
            assert np.array_equal(got, want), (name(dtype), n, p, q, np.argwhere(got != want)[:4])


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
def test_gram_at_its_edges(torch_cuda, bsm, dtype):
    torch = torch_cuda
    dtype = np.dtype(dtype)
    wide, eps = wide_of(dtype), float(np.finfo(dtype).eps)
    nprime = 2 if dtype.kind == "c" else 1
    rng = np.random.default_rng(9200 + CODE[dtype])
    worst = 0.0
    for n in [0] + gram_sizes(bsm, dtype):
        for (p, q), lo in [((5, 7), -1.0), ((17, 33), 0.0)]:  # lo = 0: positive data, a lost share cannot hide
            U, W = uniform(rng, (n, p), dtype, lo), uniform(rng, (n, q), dtype, lo)
            gbuf, Gd = dev_mat(torch, np.full((p, q), np.nan, wide), pad=2, off=1, guard=5)
            before = outside_bytes(gbuf, p, p + 2, q, 1)
            work = torch.empty(bsm.block_gram_work(dtype, n, p, q) + 16, dtype=torch.uint8, device="cuda")
            if n == 0:
                assert raw_gram(CODE[dtype], 0, p, None, 1, q, None, 1, Gd.data_ptr(), p + 2, work.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
                torch.cuda.synchronize()
                assert bool((Gd == 0).all()) and outside_bytes(gbuf, p, p + 2, q, 1) == before
                continue
            ubuf, Ud = dev_mat(torch, U, pad=3, off=1, guard=5)
            wbuf, Wd = dev_mat(torch, W, pad=1, off=3, guard=7)
            got = bsm.block_gram(Ud, Wd, out=Gd, work=work).cpu().numpy()
            torch.cuda.synchronize()
            want = U.astype(wide).conj().T @ W.astype(wide)
            bound = (nprime * n + 2) * eps * (mod1(U).T @ mod1(W))
            err = mod1(got - want)
            assert np.all(err <= bound), (name(dtype), n, p, q, float(np.max(err / bound)))
            worst = max(worst, float(np.max(err / bound)))
            assert outside_bytes(gbuf, p, p + 2, q, 1) == before, "written outside G"
            assert np.array_equal(ubuf.cpu().numpy()[1:1 + p * (n + 3)].reshape(p, n + 3)[:, :n].T, U), "U was written"
            again = bsm.block_gram(Ud, Wd, work=work).cpu().numpy()
            assert again.tobytes() == got.tobytes(), "run to run"
            # W aliasing U, and W containing U's columns
            self_g = bsm.block_gram(Ud, Ud).cpu().numpy()
            want_s = U.astype(wide).conj().T @ U.astype(wide)
            assert np.all(mod1(self_g - want_s) <= (nprime * n + 2) * eps * (mod1(U).T @ mod1(U))), (name(dtype), n, "alias")
            assert np.array_equal(self_g[:, :3], bsm.block_gram(Ud, Ud[:, :3]).cpu().numpy())
    print(f"LOBSTAT gram {name(dtype)}: largest error / bound {worst:.4f}")


def test_refusals_and_capture_of_gram(torch_cuda, bsm):
    torch = torch_cuda
    U = torch.ones((8, 40), dtype=torch.float64, device="cuda").t()
    W = torch.full((12, 40), 0.5, dtype=torch.float64, device="cuda").t()
    G = torch.zeros((12, 8), dtype=torch.float64, device="cuda").t()
    work = torch.zeros(bsm.block_gram_work(np.float64, 40, 8, 12), dtype=torch.uint8, device="cuda")
    u, w, g, k, st = U.data_ptr(), W.data_ptr(), G.data_ptr(), work.data_ptr(), torch.cuda.current_stream().cuda_stream
    good = dict(code=1, n=40, p=8, U=u, ldu=40, q=12, W=w, ldw=40, G=g, ldg=8, work=k)

    def rc(**kw):
        a = dict(good, **kw)
        return raw_gram(a["code"], a["n"], a["p"], a["U"], a["ldu"], a["q"], a["W"], a["ldw"], a["G"], a["ldg"], a["work"], st)
    assert rc() == 0 and rc(W=u, q=8) == 0 and rc(n=0, U=None, W=None) == 0
    for what, kw in [("dtype", dict(code=9)), ("mixed code", dict(code=4)), ("n", dict(n=-1)), ("p low", dict(p=0)), ("p high", dict(p=49)),
                     ("q low", dict(q=0)), ("q high", dict(q=97)), ("ldu", dict(ldu=39)), ("ldw", dict(ldw=39)), ("ldg", dict(ldg=7)),
                     ("null U", dict(U=None)), ("null W", dict(W=None)), ("null G", dict(G=None)), ("null work", dict(work=None)),
                     ("G is U", dict(G=u)), ("G inside W", dict(G=w + 64)), ("work is W", dict(work=w)), ("work is G", dict(work=g)),
                     ("work inside U", dict(work=u + 16))]:
        assert rc(**kw) == ERR_INVALID, what
    assert rc() == 0
    torch.cuda.synchronize()
    assert bool((G == 20.0).all())  # 40 x 1 x 0.5
    G.zero_()
    gr = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(gr):
        assert raw_gram(1, 40, 8, u, 40, 12, w, 40, g, 8, k, torch.cuda.current_stream().cuda_stream) == 0
    gr.replay()
    torch.cuda.synchronize()
    assert bool((G == 20.0).all())


# ---- block_combine ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [1, 2, 3, 20, 48])
@pytest.mark.parametrize("dtype", DTYPES, ids=name)
def test_block_combine_at_the_edges_of_its_tile(torch_cuda, bsm, dtype, p):
    torch = torch_cuda
    dtype = np.dtype(dtype)
    wide, eps = wide_of(dtype), float(np.finfo(dtype).eps)
    tile = bsm.block_combine_tile(dtype, p)
    assert tile >= 64 and tile % 64 == 0
    rng = np.random.default_rng(9300 + 10 * p + CODE[dtype])
    worst = 0.0
    for n in sorted({0, tile - 1, tile, tile + 1, 2 * tile + 3}):
        Vh = uniform(rng, (n, p), dtype)
        for q in sorted({0, 1, p - 1, p}):
            Ch = uniform(rng, (p, q), dtype)
            _, Cd = dev_mat(torch, Ch, pad=1, off=1) if q else (None, torch.empty((0, p), dtype=torch_dtype(torch, dtype), device="cuda").t())
            st = torch.cuda.current_stream().cuda_stream
            if n == 0 or q == 0:  # (torch gives an empty view no address worth passing: straight through the C ABI)
                Vp = None if n == 0 else dev_copy(torch, Vh)
                assert raw_block_combine(CODE[dtype], n, p, q, None if n == 0 else Vp.data_ptr(), max(n, 1), Cd.data_ptr() if q else None, p + 1,
                                         None if n == 0 else Vp.data_ptr(), max(n, 1), st) == 0
                continue
            vbuf, Vd = dev_mat(torch, Vh, pad=3, off=1, guard=5)
            obuf, Od = dev_mat(torch, np.full((n, q), np.nan, dtype), pad=2, off=3, guard=7)
            before = outside_bytes(obuf, n, n + 2, q, 3)
            got = bsm.block_combine(Vd, Cd, out=Od).cpu().numpy()
            torch.cuda.synchronize()
            assert outside_bytes(obuf, n, n + 2, q, 3) == before, ("written outside the target", n, p, q)
            assert np.array_equal(vbuf.cpu().numpy()[1:1 + p * (n + 3)].reshape(p, n + 3)[:, :n].T, Vh), "V was written"
            exact = Vh.astype(wide) @ Ch.astype(wide)
            bound = (2 * p + 1) * eps * (mod1(Vh) @ mod1(Ch))
            err = mod1(got - exact)
            assert np.all(err <= bound), (name(dtype), n, p, q, float(np.max(err / bound)))
            worst = max(worst, float(np.max(err / bound)))
            vin = outside_bytes(vbuf, n, n + 3, q, 1)
            res = bsm.block_combine(Vd, Cd)
            torch.cuda.synchronize()
            assert res.cpu().numpy().tobytes() == got.tobytes(), ("in place differs from out of place", n, p, q)
            assert outside_bytes(vbuf, n, n + 3, q, 1) == vin, ("in place wrote outside the target", n, p, q)
    print(f"LOBSTAT combine {name(dtype)} p {p} tile {tile}: largest error / bound {worst:.3f}")


def test_refusals_of_block_combine(torch_cuda, bsm):
    torch = torch_cuda
    V = torch.zeros((9, 40), dtype=torch.complex128, device="cuda").t()
    Cm = torch.zeros((8, 8), dtype=torch.complex128, device="cuda").t()
    O = torch.zeros((9, 40), dtype=torch.complex128, device="cuda").t()
    v, c, o, st = V.data_ptr(), Cm.data_ptr(), O.data_ptr(), torch.cuda.current_stream().cuda_stream
    good = dict(code=3, n=40, p=8, q=4, V=v, ldv=40, C=c, ldc=8, Out=o, ldo=40)

    def rc(**kw):
        a = dict(good, **kw)
        return raw_block_combine(a["code"], a["n"], a["p"], a["q"], a["V"], a["ldv"], a["C"], a["ldc"], a["Out"], a["ldo"], st)
    assert rc() == 0 and rc(Out=v) == 0 and rc(q=0) == 0 and rc(n=0, V=None, Out=None) == 0 and rc(q=8) == 0
    for what, kw in [("dtype", dict(code=9)), ("mixed code", dict(code=5)), ("n", dict(n=-1)), ("p low", dict(p=0)), ("p high", dict(p=49)),
                     ("q low", dict(q=-1)), ("q high", dict(q=9)), ("ldv", dict(ldv=39)), ("ldo", dict(ldo=39)), ("ldc", dict(ldc=7)),
                     ("null V", dict(V=None)), ("null Out", dict(Out=None)), ("null C", dict(C=None)), ("shifted overlap", dict(Out=v + 16)),
                     ("same start, other ld", dict(Out=v, ldo=41)), ("C is Out", dict(C=o, ldc=40)), ("C inside V, in place", dict(Out=v, C=v + 32, ldc=40))]:
        assert rc(**kw) == ERR_INVALID, what
    torch.cuda.synchronize()
    assert bool((V == 0).all()) and bool((O == 0).all())
    g = torch.cuda.CUDAGraph()
    V.fill_(1.0), Cm.fill_(0.5j)
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        assert raw_block_combine(3, 40, 8, 4, v, 40, c, 8, o, 40, torch.cuda.current_stream().cuda_stream) == 0
    g.replay()
    torch.cuda.synchronize()
    assert bool((O[:, :4] == 4.0j).all()) and bool((O[:, 4:] == 0).all())


# ---- the solves ---------------------------------------------------------------------------------------------------------------
_handles = {}


def handle(bsm, problem, kind, dtype, **kw):
    key = (problem, kind, name(dtype), tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _handles:
        if problem == "eig":
            p = eig_problem(kind, dtype)[0]
        elif problem == "mult":
            D, sets, _ = mult_dense(dtype)
            p = cut_dense(kind, D, sets)
        else:
            p = cg_dense(dtype)[0]
        _handles[key] = bsm.synthetic.build(p, **kw)
    return _handles[key]


def x0_dev(torch, n, block, dtype):
    return dev_copy(torch, start_block(n, block, dtype))


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-{c[1]}of{c[2]}")
@pytest.mark.parametrize("dtype", DTYPES, ids=name)
def test_solve_against_twin_and_dense_reference(torch_cuda, bsm, dtype, case):
    which, nev, block = case
    twin = twin_of("eig", dtype, which, nev, block)
    A = handle(bsm, "eig", "vbcrs", dtype)
    w, X, info = bsm.Lobpcg(A, nev=nev, block=block, which=which).solve(x0_dev(torch_cuda, NEIG, block, dtype), rtol=eig_rtol(dtype),
                                                                       maxiter=2 * twin.iterations)
    accept(torch_cuda, w, X, info, eig_dense(dtype)[0], twin, nev, block, which, dtype, f"vbcrs {name(dtype)} {case}")


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
def test_every_copy_of_a_triple_eigenvalue(torch_cuda, bsm, dtype):
    which, nev, block = MULT_CASE
    twin = twin_of("mult", dtype, which, nev, block)
    D = mult_dense(dtype)[0]
    A = handle(bsm, "mult", "vbcrs", dtype)
    w, X, info = bsm.lobpcg(A, nev, block=block, which=which, X0=x0_dev(torch_cuda, NEIG, block, dtype), rtol=eig_rtol(dtype),
                            maxiter=2 * twin.iterations)
    accept(torch_cuda, w, X, info, D, twin, nev, block, which, dtype, f"multiplicity {name(dtype)}")
    bound = np.sqrt(nev) * float(np.max(info.residual)) + NEIG * float(np.finfo(dtype).eps) * info.anorm
    assert np.all(np.abs(w[:3] + 2) <= bound + 4 * float(np.finfo(dtype).eps)) and abs(w[3] + 1) <= bound + 4 * float(np.finfo(dtype).eps), w


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
def test_block_jacobi_as_preconditioner(torch_cuda, bsm, dtype):
    which, nev, block = CG_CASE
    twin = twin_of("cg", dtype, which, nev, block)
    _, sets, D, _ = cg_dense(dtype)
    A = handle(bsm, "cg", "blocksparse", dtype)
    M = bsm.block_jacobi(A, sets)
    w, X, info = bsm.Lobpcg(A, nev=nev, block=block, M=M, which=which).solve(x0_dev(torch_cuda, NEIG, block, dtype), rtol=eig_rtol(dtype),
                                                                           maxiter=2 * twin.iterations)
    accept(torch_cuda, w, X, info, D, twin, nev, block, which, dtype, f"block-Jacobi {name(dtype)}", has_m=True)


def test_a_chebyshev_handle_as_preconditioner(torch_cuda, bsm):
    torch = torch_cuda
    dtype = np.float64
    which, nev, block = CG_CASE
    _, sets, D, Minv = cg_dense(dtype)
    A = handle(bsm, "cg", "blocksparse", dtype)
    ev = np.linalg.eigvals(Minv @ D).real
    M = bsm.chebyshev(A, 0.9 * ev.min(), 1.1 * ev.max(), 3, D=bsm.block_jacobi(A, sets))
    # the twin takes the handle's own action: M applied to the identity, 16 columns at a time
    Mh = np.zeros((NEIG, NEIG))
    for c0 in range(0, NEIG, 16):
        E = np.zeros((NEIG, 16), order="F")
        E[c0:c0 + 16] = np.eye(16)
        Y = torch.empty((16, NEIG), dtype=torch.float64, device="cuda").t()
        bsm.mul(Y, M, dev_copy(torch, E))
        Mh[:, c0:c0 + 16] = Y.cpu().numpy()
    twin = lobpcg_twin(D, start_block(NEIG, block, dtype), nev, block, which, eig_rtol(dtype), Minv=(Mh + Mh.T) / 2, dtype=dtype)
    assert twin.status == 0 and twin.iterations < twin_of("cg", dtype, which, nev, block).iterations
    w, X, info = bsm.Lobpcg(A, nev=nev, block=block, M=M, which=which).solve(x0_dev(torch, NEIG, block, dtype), rtol=eig_rtol(dtype),
                                                                           maxiter=2 * twin.iterations)
    accept(torch, w, X, info, D, twin, nev, block, which, dtype, "Chebyshev over block-Jacobi", has_m=True)


@pytest.mark.parametrize("case", GRID_CASES, ids=lambda c: f"{c[0]}-{c[1]}of{c[2]}")
@pytest.mark.parametrize("dtype", DTYPES, ids=name)
def test_grid_problems_in_guarded_buffers(torch_cuda, bsm, dtype, case):
    torch = torch_cuda
    which, nev, block = case
    dtype = np.dtype(dtype)
    for n in grid_sizes(dtype):
        p, Dop, ref, _ = grid_problem(dtype, n)
        X0 = start_block(n, block, dtype)
        twin = lobpcg_twin(Dop, X0, nev, block, which, eig_rtol(dtype), dtype=dtype)
        A = bsm.synthetic.build(p)
        S = bsm.Lobpcg(A, nev=nev, block=block, which=which)
        x0buf, X0d = dev_mat(torch, X0, pad=3, off=1, guard=5)
        xbuf, Xd = dev_mat(torch, np.full((n, nev), np.nan, dtype), pad=1, off=3, guard=7)
        before = outside_bytes(xbuf, n, n + 1, nev, 3)
        w, X, info = S.solve(X0d, rtol=eig_rtol(dtype), maxiter=2 * twin.iterations, X=Xd)
        accept(torch, w, X, info, Dop, twin, nev, block, which, dtype, f"grid {name(dtype)} n {n} {case}", ref=ref)
        assert outside_bytes(xbuf, n, n + 1, nev, 3) == before, "written outside X"
        assert np.array_equal(x0buf.cpu().numpy()[1:1 + block * (n + 3)].reshape(block, n + 3)[:, :n].T, X0), "X0 was written"
        if case == GRID_CASES[0] and n == grid_sizes(dtype)[0]:
            # host operands, X at its own leading dimension: the same solve as on device operands
            rc, ptr = raw_lobpcg_create(A, 0, None, 0, CODE[dtype], nev, block)
            assert rc == 0
            try:
                Xh = np.full((n + 3, nev), np.nan, dtype, order="F")
                rc, hinfo, pairs = raw_lobpcg_solve(ptr, nev, X0.ctypes.data, n, Xh.ctypes.data, n + 3, which=WHICH[which], rtol=eig_rtol(dtype),
                                                    maxiter=2 * twin.iterations, memspace=0)
                assert rc == 0 and hinfo.status == 0 and hinfo.iterations == info.iterations
                # (the same iteration; the norm a column is scaled by is summed by 16-byte groups whose fast path depends on the
                # column's alignment, which differs between the staged X and the guarded one: the last bit may differ)
                Xg = X.cpu().numpy()
                assert np.all(np.isnan(Xh[n:])) and np.all(np.abs(Xh[:n] - Xg) <= 2 * np.finfo(dtype).eps * np.abs(Xg))
                assert [pairs[i].value for i in range(nev)] == list(w)
            finally:
                assert raw_lobpcg_destroy(ptr) == 0


HANDLES = [("blocksparse", "blocksparse", np.float32, {}, None),
           ("symmetric", "symmetric", np.float64, {}, None),
           ("colored", "blocksparse", np.complex128, dict(accumulate="colored"), None),
           ("transpose_image", "vbcrs", np.complex64, dict(transpose_image=True), "adjoint"),
           ("device blocks", "vbcrs", np.float32, {}, "device"),
           ("mixed storage", "blocksparse", np.float64, dict(storage=np.float32), "rounded")]


@pytest.mark.parametrize("what,kind,dtype,kw,mode", HANDLES, ids=[h[0] for h in HANDLES])
def test_one_case_per_kind_of_handle(torch_cuda, bsm, what, kind, dtype, kw, mode):
    torch = torch_cuda
    which, nev, block = CASES[0]
    p, D, _ = eig_problem(kind, dtype)
    rtol = eig_rtol(dtype)
    A = bsm.synthetic.build(on_device(torch, p), **kw) if mode == "device" else handle(bsm, "eig", kind, dtype, **kw)
    op = bsm.adjoint(A) if mode == "adjoint" else A  # (D is Hermitian: the adjoint is the same operator)
    twin, ref = twin_of("eig", dtype, which, nev, block), None
    if mode == "rounded":  # the handle holds the values rounded to single and widened: so do the twin and the reference
        D = D.astype(np.float32).astype(np.float64)
        twin, ref = lobpcg_twin(D, start_block(NEIG, block, dtype), nev, block, which, rtol), np.linalg.eigvalsh(D)
    S = bsm.Lobpcg(op, nev=nev, block=block, which=which)
    assert S.dtype == np.dtype(dtype)
    w, X, info = S.solve(x0_dev(torch, NEIG, block, dtype), rtol=rtol, maxiter=2 * twin.iterations)
    accept(torch, w, X, info, D, twin, nev, block, which, dtype, what, ref=ref)


def test_one_solver_across_update_blocks(torch_cuda, bsm):
    torch = torch_cuda
    dtype, (which, nev, block) = np.float64, CASES[0]
    p, D, _ = eig_problem("vbcrs", dtype)
    A = bsm.synthetic.build(copied(p))
    S = bsm.Lobpcg(A, nev=nev, block=block, which=which)
    X0 = x0_dev(torch, NEIG, block, dtype)
    twin = twin_of("eig", dtype, which, nev, block)
    w, X, info = S.solve(X0, maxiter=2 * twin.iterations)
    accept(torch, w, X, info, D, twin, nev, block, which, dtype, "before the update")
    shift = 2.5
    ids, new = diagonal_shift(p, np.full(NEIG, shift))
    bsm.update_blocks(A, new, ids=ids)
    D2 = (D + shift * np.eye(NEIG)).astype(dtype)
    twin2 = lobpcg_twin(D2, start_block(NEIG, block, dtype), nev, block, which, eig_rtol(dtype))
    w2, X2, info2 = S.solve(X0, maxiter=2 * twin2.iterations)
    accept(torch, w2, X2, info2, D2, twin2, nev, block, which, dtype, "after the update", ref=np.linalg.eigvalsh(D2))
    assert np.max(np.abs(w2 - w - shift)) <= 2 * (info.residual.max() + info2.residual.max()) + 2 * NEIG * np.finfo(dtype).eps * info2.anorm


def test_statuses(torch_cuda, bsm):
    torch = torch_cuda
    for dtype in DTYPES:
        p, D, _ = eig_problem("vbcrs", dtype)
        A = handle(bsm, "eig", "vbcrs", dtype)
        S = bsm.Lobpcg(A, nev=4, block=6, which="SA")
        X0 = start_block(NEIG, 6, dtype)
        # status 1: one iteration where the twin needs many; the pairs stand as they are
        w, X, info = S.solve(dev_copy(torch, X0), rtol=eig_rtol(dtype), maxiter=1)
        assert info.status == 1 and info.iterations == 1 and info.a_products == 3 and info.m_products == 0 and info.nconv < 4
        assert info.history.shape == (2, 4) and np.all(np.isfinite(w)) and np.all(info.estimate > eig_rtol(dtype) * info.anorm)
        Xh = X.cpu().numpy().astype(wide_of(dtype))
        assert np.max(np.abs(np.linalg.norm(Xh, axis=0) - 1)) <= 8 * np.finfo(dtype).eps
        # status 3: two equal columns in X0, and a zero X0; X is not written
        for bad in (np.asfortranarray(np.concatenate([X0[:, :5], X0[:, :1]], axis=1)), np.zeros_like(X0)):
            Xn = torch.full((4, NEIG), 7.0, dtype=torch_dtype(torch, dtype), device="cuda").t()
            w, X, info = S.solve(dev_copy(torch, bad), X=Xn)
            assert info.status == 3 and info.nconv == 0 and info.iterations == 0 and np.all(np.isnan(w)) and bool((Xn == 7.0).all())
        # status 2: a NaN in one block; X is not written
        q = copied(p)
        q["blocks"][5][2, 2] = np.nan
        An = bsm.synthetic.build(q)
        Xn = torch.full((4, NEIG), 7.0, dtype=torch_dtype(torch, dtype), device="cuda").t()
        w, X, info = bsm.Lobpcg(An, nev=4, block=6).solve(dev_copy(torch, X0), X=Xn)
        assert info.status == 2 and info.nconv == 0 and np.all(np.isnan(w)) and bool((Xn == 7.0).all())
        # the solver object recovers: the next solve on the good handle converges
        w, X, info = S.solve(dev_copy(torch, X0), rtol=eig_rtol(dtype))
        assert info.status == 0


def test_two_solves_give_the_same_bytes(torch_cuda, bsm):
    torch = torch_cuda
    A = handle(bsm, "eig", "blocksparse", np.float64, accumulate="colored")  # (reproducible products)
    X0 = x0_dev(torch, NEIG, 6, np.float64)
    ys = []
    for _ in range(2):
        y = torch.empty((6, NEIG), dtype=torch.float64, device="cuda").t()
        bsm.mul(y, A, X0)
        torch.cuda.synchronize()
        ys.append(y.cpu().numpy().tobytes())
    assert ys[0] == ys[1], "the products of this handle are not reproducible"
    S = bsm.Lobpcg(A, nev=4, block=6, which="LA")
    runs = [S.solve(X0) for _ in range(2)] + [bsm.Lobpcg(A, nev=4, block=6, which="LA").solve(X0)]
    for w, X, info in runs[1:]:
        assert w.tobytes() == runs[0][0].tobytes() and X.cpu().numpy().tobytes() == runs[0][1].cpu().numpy().tobytes()
        for f in ("status", "nconv", "iterations", "drops", "a_products", "m_products", "anorm"):
            assert getattr(info, f) == getattr(runs[0][2], f), f
        assert info.residual.tobytes() == runs[0][2].residual.tobytes() and info.history.tobytes() == runs[0][2].history.tobytes()
    assert runs[0][2].status == 0 and runs[0][2].iterations > 5
    w, X, info = S.solve(seed=3)  # the default start block, on the device
    assert info.status == 0 and X.is_cuda and np.max(np.abs(w - runs[0][0])) <= 2 * (info.residual.max() + runs[0][2].residual.max()) + NEIG * 2.3e-16 * info.anorm


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_of_create(torch_cuda, bsm):
    from bsm_amd import _lib as L
    from _ctors import ctor_build
    f32, f64, c64, c128 = 0, 1, 2, 3
    p = eig_problem("blocksparse", np.float64)[0]
    H = handle(bsm, "eig", "blocksparse", np.float64)

    def refused(code, A, op, M, opM, vt, nev, block, null_out=False):
        rc, out = raw_lobpcg_create(A, op, M, opM, vt, nev, block, null_out)
        assert rc == code and (null_out or not out.value), (rc, L.lib().bsm_last_error().decode())
    refused(ERR_INVALID, None, 0, None, 0, f64, 4, 6)
    refused(ERR_INVALID, H, 0, None, 0, f64, 4, 6, null_out=True)
    refused(ERR_INVALID, H, 3, None, 0, f64, 4, 6)
    refused(ERR_INVALID, H, 0, H, 3, f64, 4, 6)
    for vt in (4, 5, -1, 6):
        refused(ERR_INVALID, H, 0, None, 0, vt, 4, 6)
    refused(ERR_INVALID, H, 0, None, 0, f32, 4, 6)   # a vector type other than the handle's own
    refused(ERR_INVALID, H, 0, None, 0, c128, 4, 6)  # a real handle under a complex vdtype has no use as A
    refused(ERR_INVALID, handle(bsm, "eig", "blocksparse", np.float64, storage=np.float32), 0, None, 0, f32, 4, 6)
    for nev, block in [(0, 6), (-1, 6), (4, 3), (4, 17), (17, 17), (4, 0)]:
        refused(ERR_INVALID, H, 0, None, 0, f64, nev, block)
    small = dict(kind="vbcrs", blocks=[np.asfortranarray(np.eye(11))], rowstart=np.array([1], np.int64), colstart=np.array([1], np.int64), size=(11, 11))
    refused(ERR_INVALID, bsm.synthetic.build(small), 0, None, 0, f64, 2, 4)  # 3 block > n
    wide = dict(kind="vbcrs", blocks=[np.asfortranarray(np.ones((30, 40)))], rowstart=np.array([1], np.int64), colstart=np.array([1], np.int64),
                size=(30, 40))
    refused(ERR_INVALID, bsm.synthetic.build(wide), 0, None, 0, f64, 1, 3)  # not square
    refused(ERR_UNSUPPORTED, bsm.neumann(H, 0.1, 2), 0, None, 0, f64, 4, 6)  # a composed handle as A
    assert "composed" in L.lib().bsm_last_error().decode()
    refused(ERR_UNSUPPORTED, ctor_build(bsm, "blocksparse", p, devices=[0, 0]), 0, None, 0, f64, 4, 6)
    refused(ERR_DEVICE, bsm.synthetic.build(p, device=-2), 0, None, 0, f64, 4, 6)
    # the pairing of M: another order, a type that does not pair, multi-device, analysis-only
    refused(ERR_INVALID, H, 0, bsm.synthetic.build(small), 0, f64, 4, 6)
    refused(ERR_INVALID, H, 0, handle(bsm, "eig", "blocksparse", np.float32), 0, f64, 4, 6)
    refused(ERR_INVALID, H, 0, handle(bsm, "eig", "blocksparse", np.complex128), 0, f64, 4, 6)
    refused(ERR_UNSUPPORTED, H, 0, ctor_build(bsm, "blocksparse", p, devices=[0, 0]), 0, f64, 4, 6)
    refused(ERR_DEVICE, H, 0, bsm.synthetic.build(p, device=-2), 0, f64, 4, 6)
    with pytest.raises(bsm._lib.BsmError, match="block"):
        bsm.Lobpcg(H, nev=4, block=17)
    with pytest.raises(ValueError, match="which"):
        bsm.Lobpcg(H, which="LM")
    # what passes: a composed handle and a real handle under a complex A as M, the widest and the narrowest block
    Hc = handle(bsm, "eig", "blocksparse", np.complex128)
    for A, M, vt, nev, block in [(H, bsm.neumann(H, 0.1, 2), f64, 4, 6), (Hc, H, c128, 4, 6), (H, None, f64, 16, 16), (H, None, f64, 1, 1)]:
        rc, ptr = raw_lobpcg_create(A, 0, M, 0, vt, nev, block)
        assert rc == 0 and ptr.value and raw_lobpcg_destroy(ptr) == 0
    assert bsm.Lobpcg(H, nev=4).block == 6 and bsm.Lobpcg(H, nev=15).block == 16


def test_refusals_of_solve(torch_cuda, bsm):
    from bsm_amd import _lib as L
    torch = torch_cuda
    H = handle(bsm, "eig", "blocksparse", np.float64)
    rc, ptr = raw_lobpcg_create(H, 0, None, 0, 1, 4, 6)
    assert rc == 0
    try:
        X0 = x0_dev(torch, NEIG, 6, np.float64)
        buf = torch.full((5 * NEIG,), 7.0, dtype=torch.float64, device="cuda")
        hist = (ctypes.c_double * (8 * 4))()  # (history_capacity counts ROWS of nev entries)
        v, x, st = X0.data_ptr(), buf.data_ptr(), torch.cuda.current_stream().cuda_stream
        good = (ptr, 4, v, NEIG, x, NEIG)
        for what, args, kw in [("null X0", (ptr, 4, None, NEIG, x, NEIG), {}), ("null X", (ptr, 4, v, NEIG, None, NEIG), {}),
                               ("ldx", (ptr, 4, v, NEIG, x, NEIG - 1), {}), ("ldx0", (ptr, 4, v, NEIG - 1, x, NEIG), {}),
                               ("null p", good, dict(null=("p",))), ("null info", good, dict(null=("info",))), ("null pairs", good, dict(null=("pairs",))),
                               ("struct size", good, dict(struct_size=24)), ("memspace", good, dict(memspace=2)), ("which BE", good, dict(which=2)),
                               ("which LM", good, dict(which=3)), ("which negative", good, dict(which=-1)), ("negative rtol", good, dict(rtol=-1e-3)),
                               ("NaN rtol", good, dict(rtol=float("nan"))), ("negative atol", good, dict(atol=-1.0)),
                               ("NaN atol", good, dict(atol=float("nan"))), ("maxiter", good, dict(maxiter=0)),
                               ("capacity without an array", good, dict(capacity=4)), ("negative capacity", good, dict(capacity=-1, history=hist))]:
            assert raw_lobpcg_solve(*args, stream=st, **kw)[0] == ERR_INVALID, what
        assert raw_lobpcg_solve(None, 4, v, NEIG, x, NEIG, stream=st)[0] == ERR_INVALID  # null S
        # X overlapping X0's last column, and just behind it (no overlap)
        big = torch.zeros(11 * NEIG, dtype=torch.float64, device="cuda")
        big[:6 * NEIG] = X0.t().reshape(-1)
        assert raw_lobpcg_solve(ptr, 4, big.data_ptr(), NEIG, big.data_ptr() + (6 * NEIG - 1) * 8, NEIG, stream=st)[0] == ERR_INVALID
        rc, info, _ = raw_lobpcg_solve(ptr, 4, big.data_ptr(), NEIG, big.data_ptr() + 6 * NEIG * 8, NEIG, stream=st, capacity=8, history=hist)
        assert rc == 0 and info.status == 0 and all(np.isfinite(hist[i]) and hist[i] > 0 for i in range(8 * 4))
        # a capturing stream
        torch.cuda.synchronize()
        scratch = torch.zeros(4, device="cuda")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            scratch.zero_()
            rc = raw_lobpcg_solve(*good, stream=torch.cuda.current_stream().cuda_stream)[0]
            why = L.lib().bsm_last_error().decode()
        assert rc == ERR_INVALID and "graph-captured" in why
        torch.cuda.synchronize()
        assert bool((buf == 7.0).all()), "a refused solve wrote X"
    finally:
        assert raw_lobpcg_destroy(ptr) == 0
    S = bsm.Lobpcg(H, nev=4, block=6)
    with pytest.raises(ValueError, match="nev"):
        S.solve(X0, X=torch.empty((3, NEIG), dtype=torch.float64, device="cuda").t())
    with pytest.raises(ValueError, match="block"):
        S.solve(X0[:, :5])
    with pytest.raises((TypeError, ValueError)):
        S.solve(X0.to(torch.float32))
