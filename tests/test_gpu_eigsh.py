"""GPU suite of bsm_krylov_combine and bsm_eigsh (-m gpu): the basis compression at the edges of its tile, in place and into
NaN-padded caller matrices, against the float64 / complex128 product under the DERIVED bound of sequential fma summation; the
solve on the order-400 problems of tests/_eigsh.py against the numpy twin and eigvalsh of the stored matrix -- every `which`
on every type, the (nev, ncv) cases of _eigsh.CASES --; the statuses on operators of order 12; one case per kind of handle and
one solver across update_blocks; run-to-run bytes; every refusal at the C level.  The whole module fails without the
feature: the entry points do not exist there.

(nev, ncv) = (4, 400) is the twin's alone (test_eigsh_cpu.py): the library bounds ncv by BSM_GMRES_MAX_RESTART = 128 -- the
Gram-Schmidt kernels and the LDS tile are sized by it -- so the device runs (4, 128) as its widest case and REFUSES (4, 400),
which test_refusals_of_create asserts.

Acceptance of a converged solve (accept, tests/_eigsh.py): the two inequalities of the issue; the gap |residual - estimate| under the derived
bound (n + ncv + 2) eps anorm that test_eigsh_cpu.py pins -- with estimate <= tol this is what bounds the residual of the
returned X --, for the reported residual and for the one recomputed in numpy from X and w; max |X^H X - I| <= 8 x the twin's
value on the same case; the twin's cycle count (+ 1); the product count."""
import ctypes as C

import numpy as np
import pytest

from _eigsh import (CASES, DTYPES, ERR_DEVICE, ERR_INVALID, ERR_UNSUPPORTED, NEIG, WHICH, accept, eig_dense, eig_problem, eig_rtol, eigsh_twin,
                    raw_combine, raw_eigsh_create, raw_eigsh_destroy, raw_eigsh_solve, steps_of, tridiagonal_block, twin_of)
from _gpu import dev_mat, outside_bytes, torch_cuda, torch_dtype  # noqa: F401
from _jacobi import CODE
from _krylov import real_of, wide_of
from _values import copied, diagonal_shift, on_device

pytestmark = pytest.mark.gpu
name = lambda d: np.dtype(d).name  # noqa: E731


def dev(torch, v):
    return torch.from_numpy(np.ascontiguousarray(v)).cuda()


# ---- krylov_combine at its edges ----------------------------------------------------------------------------------------------
def as_reals(M):
    """a (complex) matrix as the kernel walks it: its columns as 2 n reals"""
    if M.dtype.kind != "c":
        return np.asarray(M)
    return np.ascontiguousarray(M.T).view(real_of(M.dtype)).T


@pytest.mark.parametrize("m", [1, 2, 3, 20, 128])
@pytest.mark.parametrize("dtype", DTYPES, ids=name)
def test_combine_at_the_edges_of_its_tile(torch_cuda, bsm, dtype, m):
    torch = torch_cuda
    dtype = np.dtype(dtype)
    real = real_of(dtype)
    eps = float(np.finfo(dtype).eps)
    tile = bsm.krylov_combine_tile(dtype, m)
    assert tile >= 32
    rng = np.random.default_rng(8000 + 10 * m + CODE[dtype])
    worst = 0.0
    for n in sorted({0, 1, tile - 1, tile, tile + 1, 2 * tile + 3, 400}):
        Vh = rng.uniform(-1, 1, (n, m + 1)).astype(real).astype(dtype)
        if dtype.kind == "c":
            Vh = (Vh + 1j * rng.uniform(-1, 1, (n, m + 1)).astype(real)).astype(dtype)
        Vh = np.asfortranarray(Vh)
        for k in sorted({0, 1, m - 1, m}):
            Sh = np.asfortranarray(rng.uniform(-1, 1, (m, k)).astype(real))
            wide = np.float64
            exact = as_reals(Vh[:, :m]).astype(wide) @ Sh.astype(wide)
            bound = (m + 1) * eps * (np.abs(as_reals(Vh[:, :m])).astype(wide) @ np.abs(Sh).astype(wide))
            for carry in (None, m, 0):
                cols = k + (carry is not None)
                if cols == 0:
                    continue
                want_carry = None if carry is None else Vh[:, carry]
                # S at an odd element offset with a padded leading dimension; V padded, at an odd offset too
                _, Sd = dev_mat(torch, Sh, pad=1, off=1) if k else (None, torch.empty((0, m), dtype=torch_dtype(torch, real), device="cuda").t())
                vbuf, Vd = dev_mat(torch, Vh, pad=3, off=1, guard=5)
                obuf, Od = dev_mat(torch, np.full((n, cols), np.nan, dtype), pad=2, off=3, guard=7)
                before = outside_bytes(obuf, n, n + 2, cols, 3)
                if n == 0:  # (torch gives an empty view no address worth passing: straight through the C ABI)
                    assert raw_combine(CODE[dtype], 0, m, k, None, 1, Sd.data_ptr() if k else None, m + 1, None, 1,
                                       -1 if carry is None else carry, torch.cuda.current_stream().cuda_stream) == 0
                    continue
                out = bsm.krylov_combine(Vd, Sd, out=Od, carry=carry)
                torch.cuda.synchronize()
                got = out.cpu().numpy()
                assert outside_bytes(obuf, n, n + 2, cols, 3) == before, ("written outside the target", n, m, k, carry)
                assert np.array_equal(vbuf.cpu().numpy()[1:1 + (m + 1) * (n + 3)].reshape(m + 1, n + 3)[:, :n].T, Vh), "V was written"
                err = np.abs(as_reals(got[:, :k]).astype(wide) - exact)
                assert np.all(err <= bound), (name(dtype), n, m, k, carry, float(np.max(err - bound)))
                worst = max(worst, float(np.max(err / np.maximum(bound, 1e-300))) if k and n else 0.0)
                if carry is not None:
                    assert np.array_equal(got[:, k], want_carry), (n, m, k, carry)
                # in place: the same bits, and nothing of V outside the target written
                vin = outside_bytes(vbuf, n, n + 3, cols, 1)
                res = bsm.krylov_combine(Vd, Sd, carry=carry)
                torch.cuda.synchronize()
                assert res.cpu().numpy().tobytes() == got.tobytes(), ("in place differs from out of place", n, m, k, carry)
                assert outside_bytes(vbuf, n, n + 3, cols, 1) == vin, ("in place wrote outside the target", n, m, k, carry)
    print(f"EIGSTAT combine {name(dtype)} m {m} tile {tile}: largest error / bound {worst:.3f}")


def test_refusals_of_combine(torch_cuda, bsm):
    torch = torch_cuda
    V = torch.zeros((9, 40), dtype=torch.float64, device="cuda").t()  # 40 x 9, ld 40
    S = torch.zeros((8, 8), dtype=torch.float64, device="cuda").t()
    O = torch.zeros((9, 40), dtype=torch.float64, device="cuda").t()
    v, s, o, st = V.data_ptr(), S.data_ptr(), O.data_ptr(), torch.cuda.current_stream().cuda_stream
    good = dict(code=1, n=40, m=8, k=4, V=v, ldv=40, S=s, lds=8, Out=o, ldo=40, carry=8)

    def rc(**kw):
        a = dict(good, **kw)
        return raw_combine(a["code"], a["n"], a["m"], a["k"], a["V"], a["ldv"], a["S"], a["lds"], a["Out"], a["ldo"], a["carry"], st)
    assert rc() == 0 and rc(Out=v) == 0 and rc(k=0) == 0 and rc(n=0, V=None, Out=None) == 0 and rc(carry=-1, k=8) == 0
    for what, kw in [("dtype", dict(code=9)), ("mixed code", dict(code=4)), ("n", dict(n=-1)), ("m low", dict(m=0)), ("m high", dict(m=129)),
                     ("k low", dict(k=-1)), ("k high", dict(k=9)), ("carry low", dict(carry=-2)), ("carry high", dict(carry=9)),
                     ("ldv", dict(ldv=39)), ("ldo", dict(ldo=39)), ("lds", dict(lds=7)), ("null V", dict(V=None)), ("null Out", dict(Out=None)),
                     ("null S", dict(S=None)), ("shifted overlap", dict(Out=v + 8)), ("same start, other ld", dict(Out=v, ldo=41)),
                     ("overlap from behind", dict(Out=v + 8 * 40 * 8)), ("S is Out", dict(S=o, lds=40)), ("S inside V, in place", dict(Out=v, S=v + 16, lds=40)),
                     ("S behind the first column of Out", dict(S=o + 39 * 8, lds=40))]:
        assert rc(**kw) == ERR_INVALID, what
    torch.cuda.synchronize()
    assert bool((V == 0).all()) and bool((O == 0).all())
    # capturable: the call only enqueues
    g = torch.cuda.CUDAGraph()
    V.fill_(1.0), S.fill_(0.5)
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        assert raw_combine(1, 40, 8, 4, v, 40, s, 8, o, 40, -1, torch.cuda.current_stream().cuda_stream) == 0
    g.replay()
    torch.cuda.synchronize()
    assert bool((O[:, :4] == 4.0).all()) and bool((O[:, 4:] == 0).all())


# ---- the solve against twin and dense reference -------------------------------------------------------------------------------
_handles = {}


def handle(bsm, kind, dtype, **kw):
    key = (kind, name(dtype), tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _handles:
        _handles[key] = bsm.synthetic.build(eig_problem(kind, dtype)[0], **kw)
    return _handles[key]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}of{c[1]}")
@pytest.mark.parametrize("which", list(WHICH))
@pytest.mark.parametrize("dtype", DTYPES, ids=name)
def test_solve_against_twin_and_dense_reference(torch_cuda, bsm, dtype, which, case):
    nev, ncv = case
    D, _, _, v0 = eig_dense(dtype)
    A = handle(bsm, "vbcrs", dtype)
    w, X, info = bsm.Eigsh(A, nev=nev, ncv=ncv, which=which).solve(dev(torch_cuda, v0), rtol=eig_rtol(dtype))
    accept(torch_cuda, w, X, info, D, NEIG, twin_of(dtype, nev, ncv, which), nev, ncv, which, dtype, f"vbcrs {name(dtype)} {which} {case}")


@pytest.mark.parametrize("which", list(WHICH))
@pytest.mark.parametrize("kind,dtype", [("symmetric", np.float32), ("symmetric", np.float64)] + [("blocksparse", d) for d in DTYPES],
                         ids=lambda v: v if isinstance(v, str) else name(v))
def test_solve_on_the_other_kinds(torch_cuda, bsm, kind, dtype, which):
    D, _, _, v0 = eig_dense(dtype)
    A = handle(bsm, kind, dtype)
    w, X, info = bsm.eigsh(A, 4, ncv=20, which=which, v0=dev(torch_cuda, v0), rtol=eig_rtol(dtype))
    accept(torch_cuda, w, X, info, D, NEIG, twin_of(dtype, 4, 20, which), 4, 20, which, dtype, f"{kind} {name(dtype)} {which}")


def test_host_operands_and_default_start_vector(torch_cuda, bsm):
    D, _, _, v0 = eig_dense(np.float64)
    A = handle(bsm, "blocksparse", np.float64, accumulate="colored")  # (reproducible products: the bytes below can be compared)
    S = bsm.Eigsh(A, nev=4, ncv=20, which="SA")
    w, X, info = S.solve(v0)  # numpy in, numpy out: staged
    assert isinstance(X, np.ndarray) and X.flags.f_contiguous
    accept(torch_cuda, w, torch_cuda.from_numpy(X), info, D, NEIG, twin_of(np.float64, 4, 20, "SA"), 4, 20, "SA", np.float64, "host operands")
    wd, Xd, infod = S.solve(dev(torch_cuda, v0))
    assert wd.tobytes() == w.tobytes() and Xd.cpu().numpy().tobytes() == X.tobytes()
    w2, X2, info2 = S.solve(seed=3)  # the default start vector, on the device
    assert info2.status == 0 and X2.is_cuda and np.max(np.abs(w2 - w)) <= info2.residual.max() + info.residual.max() + NEIG * 2.3e-16 * info.anorm
    w3, X3, info3 = S.solve(dev(torch_cuda, v0), vectors=False)
    assert X3 is None and w3.tobytes() == w.tobytes() and np.array_equal(info3.residual, info3.estimate) and info3.a_products == info.a_products - 4


# ---- decisions and statuses, on operators of order 12 -------------------------------------------------------------------------
def test_statuses(torch_cuda, bsm):
    torch = torch_cuda
    for dtype in DTYPES:
        p, D, e1 = tridiagonal_block(dtype)
        A = bsm.synthetic.build(p)
        # status 3: e_1 lies in the invariant subspace of dimension 3, four pairs are wanted
        w, X, info = bsm.Eigsh(A, nev=4, ncv=8, which="LA").solve(dev(torch, e1))
        want = np.linalg.eigvalsh(D[:3, :3].astype(np.float64))[::-1]
        assert info.status == 3 and info.nconv == 3 and info.cycles == 1 and len(w) == 3
        assert np.max(np.abs(w - want)) <= 12 * np.finfo(np.float64).eps * 4 and np.all(info.estimate == 0)
        Xh = X.cpu().numpy()
        assert np.all(Xh[3:, :3] == 0) and np.all(info.residual <= 12 * np.finfo(dtype).eps * 4)
        assert np.max(np.abs(Xh[:, :3].conj().T @ Xh[:, :3] - np.eye(3))) <= 8 * np.finfo(dtype).eps
        # the space ends with as many pairs as are wanted: convergence
        w, X, info = bsm.Eigsh(A, nev=3, ncv=8, which="SA").solve(dev(torch, e1))
        assert info.status == 0 and info.nconv == 3 and np.max(np.abs(w - want[::-1])) <= 12 * np.finfo(np.float64).eps * 4
        # status 3 with nothing: a zero start vector; X is not written
        Xn = torch.full((4, 12), float("nan"), dtype=torch_dtype(torch, dtype), device="cuda").t()
        w, X, info = bsm.Eigsh(A, nev=4, ncv=8).solve(dev(torch, np.zeros(12, dtype)), X=Xn)
        assert info.status == 3 and info.nconv == 0 and len(w) == 0 and bool(torch.isnan(Xn).all())
        # status 1: one cycle where the twin needs more
        v0 = np.random.default_rng(5).uniform(-1, 1, 12).astype(dtype)
        twin = eigsh_twin(D, v0, 1, 3, "LA", eig_rtol(dtype))
        assert twin.status == 0 and twin.cycles > 2
        w, X, info = bsm.Eigsh(A, nev=1, ncv=3).solve(dev(torch, v0), rtol=eig_rtol(dtype), maxcycles=1)
        assert info.status == 1 and info.nconv == 1 and info.cycles == 1 and info.a_products == 3 + 1
        assert info.estimate[0] > eig_rtol(dtype) * info.anorm and abs(info.residual[0] - info.estimate[0]) <= (12 + 3 + 2) * np.finfo(dtype).eps * info.anorm
        w, X, info = bsm.Eigsh(A, nev=1, ncv=3).solve(dev(torch, v0), rtol=eig_rtol(dtype))
        assert info.status == 0 and info.cycles <= twin.cycles + 1 and abs(w[0] - 18) <= info.residual[0] + 12 * np.finfo(dtype).eps * 18
        # status 2: a NaN in one block; nothing is written to X
        q = copied(p)
        q["blocks"][1][2, 2] = np.nan
        An = bsm.synthetic.build(q)
        Xn = torch.full((4, 12), 7.0, dtype=torch_dtype(torch, dtype), device="cuda").t()
        w, X, info = bsm.Eigsh(An, nev=4, ncv=8).solve(dev(torch, v0), X=Xn)
        assert info.status == 2 and info.nconv == 0 and len(w) == 0 and bool((Xn == 7.0).all())


def test_vectors_off_leaves_x_untouched(torch_cuda, bsm):
    torch = torch_cuda
    D, _, _, v0 = eig_dense(np.float64)
    A = handle(bsm, "vbcrs", np.float64)
    rc, ptr = raw_eigsh_create(A, 0, 1, 4, 20)
    assert rc == 0
    try:
        vd = dev(torch, v0)
        Xd = torch.full((4, NEIG), 7.0, dtype=torch.float64, device="cuda")
        st = torch.cuda.current_stream().cuda_stream
        rc, info, pairs = raw_eigsh_solve(ptr, 4, vd.data_ptr(), Xd.data_ptr(), NEIG, vectors=0, stream=st)
        assert rc == 0 and info.status == 0 and info.nconv == 4 and bool((Xd == 7.0).all())
        assert all(pairs[i].residual == pairs[i].estimate for i in range(4)) and info.workspace_bytes > 21 * NEIG * 8
        rc, info2, _ = raw_eigsh_solve(ptr, 4, vd.data_ptr(), None, 0, vectors=0, stream=st)  # X may be NULL then
        assert rc == 0 and info2.a_products == info.a_products == steps_of(4, 20, info.cycles)
    finally:
        assert raw_eigsh_destroy(ptr) == 0


# ---- handles ------------------------------------------------------------------------------------------------------------------
HANDLES = [("gather", "blocksparse", np.float64, dict(accumulate="gather"), None),
           ("colored", "blocksparse", np.complex128, dict(accumulate="colored"), None),
           ("transpose_image", "vbcrs", np.complex128, dict(transpose_image=True), "adjoint"),
           ("device blocks", "vbcrs", np.float32, {}, "device"),
           ("mixed storage", "blocksparse", np.float64, dict(storage=np.float32), "rounded"),
           ("adjoint", "blocksparse", np.complex64, {}, "adjoint")]


@pytest.mark.parametrize("what,kind,dtype,kw,mode", HANDLES, ids=[h[0] for h in HANDLES])
def test_one_case_per_kind_of_handle(torch_cuda, bsm, what, kind, dtype, kw, mode):
    torch = torch_cuda
    p, D, v0 = eig_problem(kind, dtype)
    rtol = eig_rtol(dtype)
    if mode == "device":
        A = bsm.synthetic.build(on_device(torch, p), **kw)
    else:
        A = handle(bsm, kind, dtype, **kw)
    op = bsm.adjoint(A) if mode == "adjoint" else A  # (D is Hermitian: the adjoint is the same operator)
    twin, ref = twin_of(dtype, 4, 20, "BE"), None
    if mode == "rounded":  # the handle holds the values rounded to single and widened: so do the twin and the reference
        D = D.astype(np.float32).astype(np.float64)
        twin, ref = eigsh_twin(D, v0, 4, 20, "BE", rtol), np.linalg.eigvalsh(D)
    S = bsm.Eigsh(op, nev=4, ncv=20, which="BE")
    assert S.dtype == np.dtype(dtype)
    w, X, info = S.solve(dev(torch, v0), rtol=rtol)
    accept(torch, w, X, info, D, NEIG, twin, 4, 20, "BE", dtype, what, ref=ref)


@pytest.mark.parametrize("kind,dtype", [("symmetric", np.float64), ("vbcrs", np.complex128)], ids=lambda v: v if isinstance(v, str) else name(v))
def test_one_solver_across_update_blocks(torch_cuda, bsm, kind, dtype):
    torch = torch_cuda
    p, D, v0 = eig_problem(kind, dtype)
    A = bsm.synthetic.build(copied(p))
    S = bsm.Eigsh(A, nev=4, ncv=20, which="SA")
    vd = dev(torch, v0)
    w, X, info = S.solve(vd)
    accept(torch, w, X, info, D, NEIG, twin_of(dtype, 4, 20, "SA"), 4, 20, "SA", dtype, f"before the update {kind}")
    shift = 2.5
    ids, new = diagonal_shift(p, np.full(NEIG, shift))
    bsm.update_blocks(A, new, ids=ids)
    D2 = (D + shift * np.eye(NEIG)).astype(dtype)
    w2, X2, info2 = S.solve(vd)
    accept(torch, w2, X2, info2, D2, NEIG, eigsh_twin(D2, v0, 4, 20, "SA", eig_rtol(dtype)), 4, 20, "SA", dtype, f"after the update {kind}",
           ref=np.linalg.eigvalsh(D2.astype(wide_of(dtype))))
    assert np.max(np.abs(w2 - w - shift)) <= info.residual.max() + info2.residual.max() + 2 * NEIG * np.finfo(dtype).eps * info2.anorm


# ---- determinism --------------------------------------------------------------------------------------------------------------
def test_two_solves_give_the_same_bytes(torch_cuda, bsm):
    torch = torch_cuda
    D, _, _, v0 = eig_dense(np.float64)
    A = handle(bsm, "blocksparse", np.float64, accumulate="colored")
    vd = dev(torch, v0)
    # the premise: the products of this handle are reproducible, one column and four
    for cols in (1, 4):
        x = vd if cols == 1 else torch.stack([vd] * 4).contiguous().t()
        ys = []
        for _ in range(2):
            y = torch.empty_like(x) if cols == 1 else torch.empty((4, NEIG), dtype=x.dtype, device="cuda").t()
            bsm.mul(y, A, x)
            torch.cuda.synchronize()
            ys.append(y.cpu().numpy().tobytes())
        assert ys[0] == ys[1], "the products of this handle are not reproducible"
    S = bsm.Eigsh(A, nev=5, ncv=12, which="LM")
    runs = [S.solve(vd) for _ in range(2)] + [bsm.Eigsh(A, nev=5, ncv=12, which="LM").solve(vd)]
    for w, X, info in runs[1:]:
        assert w.tobytes() == runs[0][0].tobytes() and X.cpu().numpy().tobytes() == runs[0][1].cpu().numpy().tobytes()
        for f in ("status", "nconv", "cycles", "a_products", "anorm"):
            assert getattr(info, f) == getattr(runs[0][2], f), f
        assert info.residual.tobytes() == runs[0][2].residual.tobytes() and info.estimate.tobytes() == runs[0][2].estimate.tobytes()
    assert runs[0][2].cycles > 2  # restarts are part of what is compared


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_of_create(torch_cuda, bsm):
    from bsm_amd import _lib as L
    from _ctors import ctor_build
    f32, f64, c64, c128 = 0, 1, 2, 3
    p = eig_problem("blocksparse", np.float64)[0]
    H = handle(bsm, "blocksparse", np.float64)

    def refused(code, A, op, vt, nev, ncv, null_out=False):
        rc, out = raw_eigsh_create(A, op, vt, nev, ncv, null_out)
        assert rc == code and (null_out or not out.value), (rc, L.lib().bsm_last_error().decode())
    refused(ERR_INVALID, None, 0, f64, 4, 20)
    refused(ERR_INVALID, H, 0, f64, 4, 20, null_out=True)
    refused(ERR_INVALID, H, 3, f64, 4, 20)
    refused(ERR_INVALID, H, -1, f64, 4, 20)
    for vt in (4, 5, -1, 6):  # the mixed storage codes are no vector types
        refused(ERR_INVALID, H, 0, vt, 4, 20)
    refused(ERR_INVALID, H, 0, f32, 4, 20)   # a vector type other than the handle's own
    refused(ERR_INVALID, H, 0, c128, 4, 20)  # a real handle under a complex vdtype has no use here
    refused(ERR_INVALID, handle(bsm, "vbcrs", np.complex128), 0, f64, 4, 20)
    refused(ERR_INVALID, handle(bsm, "blocksparse", np.float64, storage=np.float32), 0, f32, 4, 20)  # mixed storage solves in double
    for nev, ncv in [(0, 20), (-1, 20), (4, 5), (4, 4), (4, 0), (4, 129), (4, 400), (4, 401), (126, 127), (127, 128)]:
        refused(ERR_INVALID, H, 0, f64, nev, ncv)
    p12, _, _ = tridiagonal_block(np.float64)
    refused(ERR_INVALID, bsm.synthetic.build(p12), 0, f64, 4, 13)  # ncv > n
    wide = dict(kind="vbcrs", blocks=[np.asfortranarray(np.ones((6, 9)))], rowstart=np.array([1], np.int64), colstart=np.array([1], np.int64),
                size=(6, 9))
    refused(ERR_INVALID, bsm.synthetic.build(wide), 0, f64, 1, 3)  # not square
    refused(ERR_UNSUPPORTED, bsm.neumann(H, 0.1, 2), 0, f64, 4, 20)  # a composed handle
    assert "composed" in L.lib().bsm_last_error().decode()
    refused(ERR_UNSUPPORTED, ctor_build(bsm, "blocksparse", p, devices=[0, 0]), 0, f64, 4, 20)
    refused(ERR_DEVICE, bsm.synthetic.build(p, device=-2), 0, f64, 4, 20)
    pv = eig_problem("vbcrs", np.float64)[0]
    keep = [i for i, r0 in enumerate(pv["rowstart"]) if 101 <= r0 <= 201]
    sub = dict(kind="vbcrs", blocks=[pv["blocks"][i] for i in keep], rowstart=pv["rowstart"][keep], colstart=pv["colstart"][keep], size=pv["size"])
    refused(ERR_UNSUPPORTED, bsm.synthetic.build(sub, own=(101, 300)), 0, f64, 4, 20)
    assert "own a row range" in L.lib().bsm_last_error().decode()
    with pytest.raises(bsm._lib.BsmError, match="ncv"):
        bsm.Eigsh(H, nev=4, ncv=400)
    with pytest.raises(ValueError, match="which"):
        bsm.Eigsh(H, which="SM")
    # the widest and the narrowest that pass
    for nev, ncv in [(126, 128), (1, 3)]:
        rc, ptr = raw_eigsh_create(H, 0, f64, nev, ncv)
        assert rc == 0 and ptr.value and raw_eigsh_destroy(ptr) == 0


def test_refusals_of_solve(torch_cuda, bsm):
    from bsm_amd import _lib as L
    torch = torch_cuda
    H = handle(bsm, "blocksparse", np.float64)
    v0 = eig_dense(np.float64)[3]
    rc, ptr = raw_eigsh_create(H, 0, 1, 4, 20)
    assert rc == 0
    try:
        vd = dev(torch, v0)
        buf = torch.full((5 * NEIG,), 7.0, dtype=torch.float64, device="cuda")
        v, x, st = vd.data_ptr(), buf.data_ptr(), torch.cuda.current_stream().cuda_stream
        good = (ptr, 4, v, x, NEIG)
        for what, args, kw in [("null v0", (ptr, 4, None, x, NEIG), {}), ("null X", (ptr, 4, v, None, NEIG), {}), ("ldx", (ptr, 4, v, x, NEIG - 1), {}),
                               ("null p", good, dict(null=("p",))), ("null info", good, dict(null=("info",))), ("null pairs", good, dict(null=("pairs",))),
                               ("struct size", good, dict(struct_size=24)), ("memspace", good, dict(memspace=2)), ("which", good, dict(which=4)),
                               ("which negative", good, dict(which=-1)), ("negative rtol", good, dict(rtol=-1e-3)),
                               ("NaN rtol", good, dict(rtol=float("nan"))), ("negative atol", good, dict(atol=-1.0)),
                               ("NaN atol", good, dict(atol=float("nan"))), ("maxcycles", good, dict(maxcycles=0))]:
            assert raw_eigsh_solve(*args, stream=st, **kw)[0] == ERR_INVALID, what
        assert raw_eigsh_solve(None, 4, v, x, NEIG, stream=st)[0] == ERR_INVALID  # null S
        # X overlapping v0: v0 inside the matrix, and just behind its last column (no overlap)
        big = torch.zeros(5 * NEIG, dtype=torch.float64, device="cuda")
        big[3 * NEIG + 5:4 * NEIG + 5] = vd
        assert raw_eigsh_solve(ptr, 4, big.data_ptr() + (3 * NEIG + 5) * 8, big.data_ptr(), NEIG, stream=st)[0] == ERR_INVALID
        big[4 * NEIG:] = vd
        rc, info, _ = raw_eigsh_solve(ptr, 4, big.data_ptr() + 4 * NEIG * 8, big.data_ptr(), NEIG, stream=st)
        assert rc == 0 and info.status == 0
        # a capturing stream
        torch.cuda.synchronize()
        scratch = torch.zeros(4, device="cuda")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            scratch.zero_()
            rc = raw_eigsh_solve(*good, stream=torch.cuda.current_stream().cuda_stream)[0]
            why = L.lib().bsm_last_error().decode()
        assert rc == ERR_INVALID and "graph-captured" in why
        torch.cuda.synchronize()
        assert bool((buf == 7.0).all()), "a refused solve wrote X"
    finally:
        assert raw_eigsh_destroy(ptr) == 0
    # the Python layer's own checks
    S = bsm.Eigsh(H, nev=4, ncv=20)
    with pytest.raises(ValueError, match="nev"):
        S.solve(vd, X=torch.empty((3, NEIG), dtype=torch.float64, device="cuda").t())
    with pytest.raises((TypeError, ValueError)):
        S.solve(vd.to(torch.float32))
