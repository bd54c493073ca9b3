"""GPU suite of bsm_eigsh on vectors of several workgroups (-m gpu).  test_gpu_eigsh.py runs every solve on operators of order
400 and 12 -- one workgroup per vector, at most 5 wanted pairs, one batch of the true-residual pass, freshly allocated X.
Here the orders of _eigsh.grid_sizes put G = 2 and G = 3 workgroups on a vector (test_eigsh_grid_cpu.py pins that, and the
twin's status and cycle count of every case below), so that inside the solver

  * the partials part[c * G + g] of the residual pass, the norm shares nrmpart[0 .. G) and the ncv * G partials of the two
    Gram-Schmidt passes are more than one per column, and the guarded scale and the in-place restart walk more than one row
    range at a padded leading dimension (test_two_and_three_workgroups; test_a_lost_share_shows_in_single_precision runs the
    single types at a loose tolerance besides, where a residual that lost a workgroup's share leaves the acceptance's 1e-5 anorm);
  * nev = 17 and 33 walk the true-residual pass in batches of 16 + 1 and 16 + 16 + 1, X + c0 * ldx, theta + c0, res + c0 with
    c0 > 0, and reuse beta's slots past index 4 as norm slots (test_more_than_one_residual_batch);
  * the caller's X is a window of a NaN-filled buffer at ldx = n + 1, one element past a 16-byte boundary, v0 a view one
    element into a buffer, and a host X at ldx = n + 3 (test_the_callers_buffers, test_host_x_at_its_own_leading_dimension);
  * ncv == n, the largest subspace bsm_eigsh_create accepts, on the order-12 operator (test_basis_of_the_whole_space);
  * run to run at G = 3, and update_blocks + solve on one side stream at G = 3.

Acceptance is _eigsh.accept, the one of test_gpu_eigsh.py, against the numpy twin on the same operator and the spectrum of the
blocks as stored; it recomputes every pair's residual in numpy from X and w."""
import numpy as np
import pytest

from _eigsh import (BATCH_CASES, DTYPES, GRID_CASES, LOOSE_CASE, LOOSE_RTOL, LOOSE_TYPES, accept, eig_rtol, eigsh_twin, grid_problem, grid_sizes,
                    grid_twin, raw_eigsh_create, raw_eigsh_destroy, raw_eigsh_solve, tridiagonal_block, wanted_reference)
from _gpu import dev_copy, dev_mat, dev_vec, outside_bytes, torch_cuda  # noqa: F401
from _jacobi import CODE
from _krylov import wide_of
from _lockstep import krylov_grid
from _values import diagonal_shift, on_device

pytestmark = pytest.mark.gpu
name = lambda d: np.dtype(d).name  # noqa: E731
TABLE = [(dt, n, G) for dt in DTYPES for n, G in zip(grid_sizes(dt), (2, 3))]
TABLE_IDS = [f"{name(dt)}-n{n}-G{G}" for dt, n, G in TABLE]


def dev(torch, v):
    return torch.from_numpy(np.ascontiguousarray(v)).cuda()


_handles = {}


def handle(bsm, dtype, n, spec="high"):
    """the vbcrs handle of grid_problem(dtype, n, spec), built once"""
    key = (name(dtype), n, spec)
    if key not in _handles:
        _handles[key] = bsm.synthetic.build(grid_problem(dtype, n, spec)[0])
    return _handles[key]


def reproducible_products(torch, bsm, A, vd, widths=(1, 16)):
    """the premise of every comparison of bytes: two products of this handle give the same bytes, one column and several"""
    n = vd.shape[0]
    for cols in widths:
        x = vd if cols == 1 else torch.stack([vd] * cols).contiguous().t()
        ys = []
        for _ in range(2):
            y = torch.empty_like(vd) if cols == 1 else torch.empty((cols, n), dtype=vd.dtype, device="cuda").t()
            bsm.mul(y, A, x)
            torch.cuda.synchronize()
            ys.append(y.cpu().numpy().tobytes())
        assert ys[0] == ys[1], "the products of this handle are not reproducible"


# ---- 1. G = 2 and 3 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", GRID_CASES, ids=lambda c: f"{c[0]}of{c[1]}-{c[2]}")
@pytest.mark.parametrize("dtype,n,G", TABLE, ids=TABLE_IDS)
def test_two_and_three_workgroups(torch_cuda, bsm, dtype, n, G, case):
    nev, ncv, which = case
    assert krylov_grid(n, np.dtype(dtype).itemsize) == G
    _, Dop, ref, v0 = grid_problem(dtype, n)
    S = bsm.Eigsh(handle(bsm, dtype, n), nev=nev, ncv=ncv, which=which)
    w, X, info = S.solve(dev(torch_cuda, v0), rtol=eig_rtol(dtype))
    accept(torch_cuda, w, X, info, Dop, n, grid_twin(dtype, n, nev, ncv, which), nev, ncv, which, dtype, f"G {G} {name(dtype)} n {n} {which} {nev, ncv}",
           ref=ref)


@pytest.mark.parametrize("dtype,n,G", [t for t in TABLE if t[0] in LOOSE_TYPES], ids=[i for t, i in zip(TABLE, TABLE_IDS) if t[0] in LOOSE_TYPES])
def test_a_lost_share_shows_in_single_precision(torch_cuda, bsm, dtype, n, G):
    """the single types at LOOSE_RTOL.  At eig_rtol their residuals are of the size of the acceptance's |true - residual| <= 1e-5
    anorm, so that a residual pass that lost a workgroup's share passes it; here the last range's share is more than ten times
    that (test_eigsh_grid_cpu.py: test_twin_at_the_loose_tolerance)"""
    nev, ncv, which = LOOSE_CASE
    _, Dop, ref, v0 = grid_problem(dtype, n)
    w, X, info = bsm.Eigsh(handle(bsm, dtype, n), nev=nev, ncv=ncv, which=which).solve(dev(torch_cuda, v0), rtol=LOOSE_RTOL)
    accept(torch_cuda, w, X, info, Dop, n, grid_twin(dtype, n, nev, ncv, which, rtol=LOOSE_RTOL), nev, ncv, which, dtype,
           f"loose G {G} {name(dtype)} n {n} {which} {nev, ncv}", ref=ref, rtol=LOOSE_RTOL)


# ---- 2. more than one batch of the true-residual pass -----------------------------------------------------------------------
@pytest.mark.parametrize("case", BATCH_CASES, ids=lambda c: f"{c[0]}of{c[1]}-{c[2]}-{c[3]}")
@pytest.mark.parametrize("dtype", DTYPES, ids=name)
def test_more_than_one_residual_batch(torch_cuda, bsm, dtype, case):
    torch = torch_cuda
    nev, ncv, which, spec = case
    n = grid_sizes(dtype)[0]
    _, Dop, ref, v0 = grid_problem(dtype, n, spec)
    A, vd = handle(bsm, dtype, n, spec), dev(torch, v0)
    S = bsm.Eigsh(A, nev=nev, ncv=ncv, which=which)
    w, X, info = S.solve(vd, rtol=eig_rtol(dtype))
    accept(torch, w, X, info, Dop, n, grid_twin(dtype, n, nev, ncv, which, spec), nev, ncv, which, dtype, f"batches {name(dtype)} n {n} {which} {nev, ncv}",
           ref=ref)
    if nev == 17:  # without the vectors: the same values, the estimates in place of the residuals, no product of the residual pass
        reproducible_products(torch, bsm, A, vd)
        w0, X0, info0 = S.solve(vd, rtol=eig_rtol(dtype), vectors=False)
        assert X0 is None and info0.status == 0 and info0.nconv == 17 and info0.cycles == info.cycles
        assert w0.tobytes() == w.tobytes() and info0.estimate.tobytes() == info.estimate.tobytes()
        assert np.array_equal(info0.residual, info0.estimate) and info0.a_products == info.a_products - 17


# ---- 3. the caller's buffers ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.complex64], ids=name)
def test_the_callers_buffers(torch_cuda, bsm, dtype):
    """X: an n x nev window at ldx = n + 1 of a NaN-filled buffer, one element past a 16-byte boundary (one guard element in
    front, five behind); v0: a view one element into a larger buffer.  The combine writes the window, the normalisation runs
    on the caller's columns through the head / 16-byte-group route of bsm_krylov.hip (ldx * es is a multiple of 16, the first
    element is not at a boundary).  The bytes of the aligned solve are NOT demanded: that route sums the norm in another
    order."""
    torch = torch_cuda
    nev, ncv, which = 5, 12, "LA"
    n = grid_sizes(dtype)[0]
    es = np.dtype(dtype).itemsize
    _, Dop, ref, v0 = grid_problem(dtype, n)
    xbuf, xview = dev_mat(torch, np.full((n, nev), np.nan, dtype), pad=1, off=1, guard=5)
    vbuf, vview = dev_vec(torch, v0, off=1, guard=3)
    assert xview.data_ptr() % 16 == es % 16 != 0 and vview.data_ptr() % 16 == es % 16 and (n + 1) * es % 16 == 0 and xview.stride(1) == n + 1
    before = (outside_bytes(xbuf, n, n + 1, nev, off=1), vbuf.cpu().numpy().tobytes())
    S = bsm.Eigsh(handle(bsm, dtype, n), nev=nev, ncv=ncv, which=which)
    w, X, info = S.solve(vview, rtol=eig_rtol(dtype), X=xview)
    torch.cuda.synchronize()
    assert X.data_ptr() == xview.data_ptr()
    assert outside_bytes(xbuf, n, n + 1, nev, off=1) == before[0], "X was written outside its n x nev window"
    assert vbuf.cpu().numpy().tobytes() == before[1], "v0 or its surroundings were written"
    assert not bool(torch.isnan(torch.view_as_real(xview) if xview.is_complex() else xview).any())
    accept(torch, w, xview, info, Dop, n, grid_twin(dtype, n, nev, ncv, which), nev, ncv, which, dtype, f"caller's buffers {name(dtype)} n {n}", ref=ref)


@pytest.mark.parametrize("dtype", [np.float64, np.complex64], ids=name)
def test_host_x_at_its_own_leading_dimension(torch_cuda, bsm, dtype):
    """bsm_eigsh_solve with BSM_MEM_HOST at ldx = n + 3: column c lands at c * ldx, the rows behind n stay as they were, the
    values are the device solve's to the bit (the staged X has the layout of a fresh device X: ldx = n from an aligned base)"""
    torch = torch_cuda
    nev, ncv = 5, 12
    n = grid_sizes(dtype)[0]
    _, Dop, ref, v0 = grid_problem(dtype, n)
    A, vd = handle(bsm, dtype, n), dev(torch, v0)
    reproducible_products(torch, bsm, A, vd, widths=(1, nev))
    w, X, info = bsm.Eigsh(A, nev=nev, ncv=ncv, which="LA").solve(vd, rtol=eig_rtol(dtype))
    accept(torch, w, X, info, Dop, n, grid_twin(dtype, n, nev, ncv, "LA"), nev, ncv, "LA", dtype, f"device solve for the host one {name(dtype)}", ref=ref)
    rc, ptr = raw_eigsh_create(A, 0, CODE[np.dtype(dtype)], nev, ncv)
    assert rc == 0
    try:
        ldx = n + 3
        Xh = np.full((ldx, nev), np.nan, dtype, order="F")
        vh = np.ascontiguousarray(v0)
        rc, hinfo, pairs = raw_eigsh_solve(ptr, nev, vh.ctypes.data, Xh.ctypes.data, ldx, rtol=eig_rtol(dtype), memspace=0)
        assert rc == 0 and hinfo.status == 0 and hinfo.nconv == nev and hinfo.cycles == info.cycles and hinfo.a_products == info.a_products
        assert np.all(np.isnan(Xh[n:])), "the rows behind n were written"
        assert Xh[:n].tobytes() == np.asfortranarray(X.cpu().numpy()).tobytes(), "the host X differs from the device X"
        assert np.array([pairs[i].value for i in range(nev)]).tobytes() == w.tobytes()
        assert np.array([pairs[i].residual for i in range(nev)]).tobytes() == info.residual.tobytes()
        assert np.array_equal(vh, v0)
    finally:
        assert raw_eigsh_destroy(ptr) == 0


# ---- 4. ncv == n ----------------------------------------------------------------------------------------------------------------
FULL_CASES = [(10, 12, "LA"), (10, 12, "BE"), (1, 12, "SA")]  # (test_eigsh_grid_cpu.py: the twin's side)


@pytest.mark.parametrize("case", FULL_CASES, ids=lambda c: f"{c[0]}of{c[1]}-{c[2]}")
@pytest.mark.parametrize("dtype", DTYPES, ids=name)
def test_basis_of_the_whole_space(torch_cuda, bsm, dtype, case):
    """step n - 1 leaves a w that is rounding alone; the guarded scale and the decision see its norm"""
    torch = torch_cuda
    nev, ncv, which = case
    eps = float(np.finfo(dtype).eps)
    p, D, _ = tridiagonal_block(dtype)
    v0 = np.random.default_rng(5).uniform(-1, 1, 12).astype(dtype)
    twin = eigsh_twin(D, v0, nev, ncv, which, eig_rtol(dtype))
    assert twin.status == 0 and twin.cycles == 1
    w, X, info = bsm.Eigsh(bsm.synthetic.build(p), nev=nev, ncv=ncv, which=which).solve(dev(torch, v0), rtol=eig_rtol(dtype))
    lam = wanted_reference(np.linalg.eigvalsh(D.astype(wide_of(dtype))), which, nev)
    Xh = X.cpu().numpy().astype(wide_of(dtype))
    orth = float(np.max(np.abs(Xh.conj().T @ Xh - np.eye(nev))))
    print(f"EIGSTAT ncv == n {name(dtype)} {case}: status {info.status} cycles {info.cycles} a_products {info.a_products}, orth / eps {orth / eps:.2f} "
          f"(twin {twin.orth / eps:.2f}, margin used {orth / twin.orth if twin.orth else float('inf'):.2f} of 8), max (|theta - lam| - residual) / (eps anorm) "
          f"{np.max(np.abs(w - lam) - info.residual) / (eps * info.anorm):.2f} of 12, max estimate / (eps anorm) {np.max(info.estimate) / (eps * info.anorm):.2f}")
    assert info.status == 0 and info.nconv == nev == len(w) and info.cycles == 1 and info.a_products == 12 + nev
    assert np.all(np.isfinite(Xh))
    assert orth <= 8 * twin.orth, (orth / eps, twin.orth / eps)
    assert np.all(np.abs(w - lam) <= info.residual + 12 * eps * info.anorm), (w, lam, info.residual)


# ---- 5. run to run at G = 3 -----------------------------------------------------------------------------------------------------
def test_two_solves_give_the_same_bytes_on_three_workgroups(torch_cuda, bsm):
    torch = torch_cuda
    dtype, n = np.float64, grid_sizes(np.float64)[1]
    assert krylov_grid(n, 8) == 3
    _, Dop, ref, v0 = grid_problem(dtype, n)
    A, vd = handle(bsm, dtype, n), dev(torch, v0)
    reproducible_products(torch, bsm, A, vd)
    S = bsm.Eigsh(A, nev=5, ncv=12, which="LM")
    runs = [S.solve(vd) for _ in range(2)] + [bsm.Eigsh(A, nev=5, ncv=12, which="LM").solve(vd)]
    for w, X, info in runs[1:]:
        assert w.tobytes() == runs[0][0].tobytes() and X.cpu().numpy().tobytes() == runs[0][1].cpu().numpy().tobytes()
        for f in ("status", "nconv", "cycles", "a_products", "anorm"):
            assert getattr(info, f) == getattr(runs[0][2], f), f
        assert info.residual.tobytes() == runs[0][2].residual.tobytes() and info.estimate.tobytes() == runs[0][2].estimate.tobytes()
    assert runs[0][2].status == 0 and runs[0][2].cycles > 2  # restarts are part of what is compared
    w, X, info = runs[0]
    accept(torch, w, X, info, Dop, n, grid_twin(dtype, n, 5, 12, "LM"), 5, 12, "LM", dtype, "run to run, G 3", ref=ref, rtol=1e-10)


# ---- 6. update_blocks and the solve on one side stream --------------------------------------------------------------------------
def test_update_and_solve_on_a_side_stream(torch_cuda, bsm):
    """device-resident blocks; update_blocks(..., stream=side) and S.solve(..., stream=side) on the same solver object: nothing
    orders them but the stream"""
    torch = torch_cuda
    dtype, n, nev, ncv, which = np.complex128, grid_sizes(np.complex128)[1], 5, 12, "LA"
    assert krylov_grid(n, 16) == 3
    p, Dop, ref, v0 = grid_problem(dtype, n)
    A = bsm.synthetic.build(on_device(torch, p))
    S = bsm.Eigsh(A, nev=nev, ncv=ncv, which=which)
    vd = dev(torch, v0)
    shift = 2.5
    ids, new = diagonal_shift(p, np.full(n, shift))
    new = [dev_copy(torch, b) for b in new]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    w, X, info = S.solve(vd, rtol=eig_rtol(dtype), stream=side)
    accept(torch, w, X, info, Dop, n, grid_twin(dtype, n, nev, ncv, which), nev, ncv, which, dtype, "side stream, before the update", ref=ref)
    bsm.update_blocks(A, new, ids=ids, stream=side)
    w2, X2, info2 = S.solve(vd, rtol=eig_rtol(dtype), stream=side)
    D2 = Dop.shifted(shift)
    accept(torch, w2, X2, info2, D2, n, eigsh_twin(D2, v0, nev, ncv, which, eig_rtol(dtype)), nev, ncv, which, dtype, "side stream, after the update",
           ref=D2.eigenvalues())
    assert np.max(np.abs(w2 - w - shift)) <= info.residual.max() + info2.residual.max() + 2 * n * np.finfo(dtype).eps * info2.anorm
