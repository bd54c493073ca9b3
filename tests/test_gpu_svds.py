"""GPU suite of bsm_svds (-m gpu): the solve on the 600 x 400 problems of tests/_svds.py against the numpy twin and svd of the
stored matrix -- both `which`, every type, A, adjoint(A) and transpose(A) of the real types, the (nsv, ncv) cases of
_svds.CASES --; one case per kind of handle test_gpu_lsqr_handles.py runs; a block-diagonal rectangular operator that puts 3
workgroups on the m-row grid and 2 on the n-row grid, with U, V, v0 off a 16-byte boundary in NaN-guarded buffers, 17 triplets
(two batches of the residual pass), a host U at its own leading dimension, and its adjoint (the recurrence on op(A)^H);
ncv = min(m, n); the statuses on operators of order 12; run-to-run bytes on a transpose_image handle; one solver across
update_blocks; vectors=False; every refusal at the C level.  The whole module fails without the feature: the entry points do
not exist there.

Acceptance of a converged solve (accept, tests/_svds.py), every bound derived:
  1. status 0, nconv = nsv, estimates <= rtol anorm;
  2. |sigma_i - s_i| <= sqrt((r_av^2 + r_ahu^2) / 2) + max(m, n) eps anorm: the Hermitian residual bound on [[0, A], [A^H, 0]] with
     the vector [u; v] / sqrt(2), plus the backward error of the dense reference;
  3. the reported residuals against the ones recomputed in numpy from U, V and s: within TOL[dtype] anorm;
  4. |hypot(r_av, r_ahu) - estimate| <= 2 (max(m, n) + ncv + 2) eps anorm: the argument of _eigsh.accept's gap bound on both sides;
  5. max |U^H U - I|, max |V^H V - I| <= 8 x the twin's value on the same case (the margin of _eigsh.accept);
  6. cycles <= twin + 1, a_products = 2 steps + 2 nsv, anorm <= s_max (1 + max(m, n) eps)."""
import numpy as np
import pytest

from _gpu import dev_mat, dev_vec, outside_bytes, torch_cuda, torch_dtype  # noqa: F401
from _jacobi import CODE
from _lsqr import Dense
from _svds import (CASES, DTYPES, ERR_DEVICE, ERR_INVALID, ERR_UNSUPPORTED, LM, M600, N400, SIDES, SM, accept, bordered_problem,
                   diagonal_problem, grid_svd_problem, raw_svds_create, raw_svds_destroy, raw_svds_solve, side_of, steps_of,
                   stored_singular_values, svd_dense, svd_problem, svd_rtol, svds_twin, twin_of)
from _values import copied, on_device

pytestmark = pytest.mark.gpu
name = lambda d: np.dtype(d).name  # noqa: E731
ALL_CASES = [(w, c) for w in ("LM", "SM") for c in CASES[w]]


def dev(torch, v):
    return torch.from_numpy(np.ascontiguousarray(v)).cuda()


_handles = {}


def handle(bsm, kind, dtype, **kw):
    key = (kind, name(dtype), tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _handles:
        _handles[key] = bsm.synthetic.build(svd_problem(kind, dtype)[0], **kw)
    return _handles[key]


def wrapped(bsm, H, side):
    return {"A": lambda a: a, "adjoint": bsm.adjoint, "transpose": bsm.transpose}[side](H)


# ---- the solve against twin and dense reference -------------------------------------------------------------------------------
@pytest.mark.parametrize("which,case", ALL_CASES, ids=lambda v: v if isinstance(v, str) else f"{v[0]}of{v[1]}")
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("dtype", DTYPES, ids=name)
def test_solve_against_twin_and_dense_reference(torch_cuda, bsm, dtype, side, which, case):
    nsv, ncv = case
    A, _, _, _, v0 = svd_dense(dtype)
    S = bsm.Svds(wrapped(bsm, handle(bsm, "vbcrs", dtype), side), nsv=nsv, ncv=ncv, which=which)
    s, U, V, info = S.solve(dev(torch_cuda, v0), rtol=svd_rtol(dtype))
    accept(s, U, V, info, side_of(A, side), twin_of(dtype, side, nsv, ncv, which), nsv, ncv, which, dtype,
           f"vbcrs {name(dtype)} {side} {which} {case}", ref=stored_singular_values(Dense(A)))


@pytest.mark.parametrize("which", ["LM", "SM"])
@pytest.mark.parametrize("kind,dtype", [("vbcrs", np.float32), ("blocksparse", np.float64)], ids=lambda v: v if isinstance(v, str) else name(v))
def test_transpose_of_the_real_types(torch_cuda, bsm, kind, dtype, which):
    """transpose(A) of a real A is adjoint(A): the same twin"""
    A, _, _, _, v0 = svd_dense(dtype)
    s, U, V, info = bsm.svds(bsm.transpose(handle(bsm, kind, dtype)), 4, ncv=20, which=which, v0=dev(torch_cuda, v0), rtol=svd_rtol(dtype))
    accept(s, U, V, info, side_of(A, "adjoint"), twin_of(dtype, "adjoint", 4, 20, which), 4, 20, which, dtype,
           f"{kind} {name(dtype)} transpose {which}", ref=stored_singular_values(Dense(A)))


@pytest.mark.parametrize("which", ["LM", "SM"])
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("dtype", DTYPES, ids=name)
def test_solve_on_the_blocksparse_kind(torch_cuda, bsm, dtype, side, which):
    A, _, _, _, v0 = svd_dense(dtype)
    s, U, V, info = bsm.svds(wrapped(bsm, handle(bsm, "blocksparse", dtype), side), 4, ncv=20, which=which, v0=dev(torch_cuda, v0),
                             rtol=svd_rtol(dtype))
    accept(s, U, V, info, side_of(A, side), twin_of(dtype, side, 4, 20, which), 4, 20, which, dtype, f"blocksparse {name(dtype)} {side} {which}",
           ref=stored_singular_values(Dense(A)))


def test_host_operands_and_default_start_vector(torch_cuda, bsm):
    A, _, _, _, v0 = svd_dense(np.float64)
    H = handle(bsm, "blocksparse", np.float64, accumulate="colored")  # (reproducible products: the bytes below can be compared)
    S = bsm.Svds(H, nsv=4, ncv=20, which="SM")
    s, U, V, info = S.solve(v0)  # numpy in, numpy out: staged
    assert isinstance(U, np.ndarray) and U.flags.f_contiguous and U.shape == (M600, 4) and V.shape == (N400, 4)
    accept(s, U, V, info, A, twin_of(np.float64, "A", 4, 20, "SM"), 4, 20, "SM", np.float64, "host operands")
    sd, Ud, Vd, infod = S.solve(dev(torch_cuda, v0))
    assert sd.tobytes() == s.tobytes() and Ud.cpu().numpy().tobytes() == U.tobytes() and Vd.cpu().numpy().tobytes() == V.tobytes()
    s2, U2, V2, info2 = S.solve(seed=3)  # the default start vector, on the device
    assert info2.status == 0 and U2.is_cuda and S.ncv == 20
    assert np.max(np.abs(s2 - s)) <= np.hypot(info2.residual_av, info2.residual_ahu).max() + np.hypot(info.residual_av, info.residual_ahu).max() \
        + M600 * 2.3e-16 * info.anorm
    s3, U3, V3, info3 = S.solve(dev(torch_cuda, v0), vectors=False)
    assert U3 is None and V3 is None and s3.tobytes() == s.tobytes() and info3.a_products == info.a_products - 8
    assert np.array_equal(info3.residual_ahu, info3.estimate) and not info3.residual_av.any()  # (600 x 400: B = A)


# ---- handles ------------------------------------------------------------------------------------------------------------------
HANDLES = [("gather", "blocksparse", np.float64, dict(accumulate="gather"), "A", "LM"),
           ("colored", "blocksparse", np.complex128, dict(accumulate="colored"), "adjoint", "SM"),
           ("transpose_image", "vbcrs", np.complex128, dict(transpose_image=True), "A", "SM"),
           ("transpose_image adjoint", "blocksparse", np.float32, dict(transpose_image=True), "adjoint", "LM"),
           ("device blocks", "vbcrs", np.float32, {}, "device", "SM"),
           ("mixed storage", "blocksparse", np.float64, dict(storage=np.float32), "rounded", "LM"),
           ("mixed storage adjoint", "vbcrs", np.complex128, dict(storage=np.complex64), "rounded adjoint", "SM")]


@pytest.mark.parametrize("what,kind,dtype,kw,mode,which", HANDLES, ids=[h[0] for h in HANDLES])
def test_one_case_per_kind_of_handle(torch_cuda, bsm, what, kind, dtype, kw, mode, which):
    torch = torch_cuda
    p, A, v0 = svd_problem(kind, dtype)
    rtol = svd_rtol(dtype)
    H = bsm.synthetic.build(on_device(torch, p), **kw) if mode == "device" else handle(bsm, kind, dtype, **kw)
    side = "adjoint" if mode.endswith("adjoint") else "A"
    twin, ref = twin_of(dtype, side, 4, 20, which), stored_singular_values(Dense(A))
    if mode.startswith("rounded"):  # the handle holds the values rounded to single and widened: so do the twin and the reference
        A = A.astype(np.complex64 if np.dtype(dtype).kind == "c" else np.float32).astype(dtype)
        twin, ref = svds_twin(side_of(A, side), v0, 4, 20, which, rtol), np.linalg.svd(A, compute_uv=False)
    S = bsm.Svds(wrapped(bsm, H, side), nsv=4, ncv=20, which=which)
    assert S.dtype == np.dtype(dtype)
    s, U, V, info = S.solve(dev(torch, v0), rtol=rtol)
    accept(s, U, V, info, side_of(A, side), twin, 4, 20, which, dtype, what, ref=ref)


def test_one_solver_across_update_blocks(torch_cuda, bsm):
    """every block doubled: the operator is 2 A to the bit, and so is every number of the recurrence"""
    torch, dtype = torch_cuda, np.float64
    p, A, v0 = svd_problem("vbcrs", dtype)
    H = bsm.synthetic.build(copied(p))
    S = bsm.Svds(H, nsv=4, ncv=20, which="SM")
    vd = dev(torch, v0)
    s, U, V, info = S.solve(vd)
    twin = twin_of(dtype, "A", 4, 20, "SM")
    accept(s, U, V, info, A, twin, 4, 20, "SM", dtype, "before the update")
    bsm.update_blocks(H, [np.asfortranarray(2 * b) for b in p["blocks"]], ids=list(range(1, len(p["blocks"]) + 1)))
    A2 = 2 * A
    s2, U2, V2, info2 = S.solve(vd)
    accept(s2, U2, V2, info2, A2, svds_twin(A2, v0, 4, 20, "SM", svd_rtol(dtype)), 4, 20, "SM", dtype, "after the update",
           ref=2 * stored_singular_values(Dense(A)))
    assert np.max(np.abs(s2 - 2 * s)) <= 2 * M600 * np.finfo(dtype).eps * info2.anorm


# ---- several workgroups per vector, caller buffers ----------------------------------------------------------------------------
def grid_run(torch, bsm, dtype, side, nsv, ncv, which, host_u=False):
    dtype = np.dtype(dtype)
    p, op, v0 = grid_svd_problem(dtype)
    key = ("grid", dtype.name)
    if key not in _handles:
        _handles[key] = bsm.synthetic.build(p)
    H = _handles[key]
    opx = op if side == "A" else op.H
    m, n = opx.shape
    # the premise: 3 workgroups on the long grid, 2 on the short one (bsm_krylov_orth_work is k G elements + G reals, each part
    # rounded up to 16 bytes; 16 G elements are whole 16-byte groups, so the difference of two calls gives G)
    grids = [(bsm.krylov_orth_work(dtype, rows, 16) - bsm.krylov_orth_work(dtype, rows, 0)) // (16 * dtype.itemsize) for rows in (max(m, n), min(m, n))]
    assert grids == [3, 2], grids
    rtol = svd_rtol(dtype)
    twin = svds_twin(opx, v0, nsv, ncv, which, rtol)
    what = f"grid {dtype.name} {m} x {n} {side} {which} {nsv}of{ncv}"
    if host_u:  # host operands, U at its own leading dimension, through the C interface
        rc, ptr = raw_svds_create(H, 0 if side == "A" else 2, CODE[dtype], nsv, ncv)
        assert rc == 0
        try:
            ldu, ldv = m + 5, n + 2
            Uh, Vh = np.full((nsv, ldu), np.nan, dtype), np.full((nsv, ldv), np.nan, dtype)
            rc, info, trip = raw_svds_solve(ptr, nsv, v0.ctypes.data, Uh.ctypes.data, ldu, Vh.ctypes.data, ldv, which=LM if which == "LM" else SM,
                                            rtol=rtol, memspace=0)
            assert rc == 0 and info.status == 0 and info.nconv == nsv
            assert np.isnan(Uh[:, m:]).all() and np.isnan(Vh[:, n:]).all() and not np.isnan(Uh[:, :m]).any() and not np.isnan(Vh[:, :n]).any()
            out = bsm.SvdsInfo(info, trip)
            accept(out.value.copy(), np.ascontiguousarray(Uh[:, :m].T), np.ascontiguousarray(Vh[:, :n].T), out, opx, twin, nsv, ncv, which, dtype,
                   what + " host U")
        finally:
            assert raw_svds_destroy(ptr) == 0
        return
    ubuf, Ud = dev_mat(torch, np.full((m, nsv), np.nan, dtype), pad=3, off=1, guard=5)
    vbuf, Vd = dev_mat(torch, np.full((n, nsv), np.nan, dtype), pad=1, off=3, guard=7)
    wbuf, wd = dev_vec(torch, v0, off=1, guard=3)
    ub, vb, wb = outside_bytes(ubuf, m, m + 3, nsv, 1), outside_bytes(vbuf, n, n + 1, nsv, 3), wbuf.cpu().numpy().tobytes()
    S = bsm.Svds(wrapped(bsm, H, side), nsv=nsv, ncv=ncv, which=which)
    s, U, V, info = S.solve(wd, rtol=rtol, U=Ud, V=Vd)
    assert U is Ud and V is Vd
    assert outside_bytes(ubuf, m, m + 3, nsv, 1) == ub and outside_bytes(vbuf, n, n + 1, nsv, 3) == vb, "written outside U or V"
    assert wbuf.cpu().numpy().tobytes() == wb, "v0 was written"
    accept(s, U, V, info, opx, twin, nsv, ncv, which, dtype, what)


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
def test_two_and_three_workgroups_seventeen_triplets_in_caller_buffers(torch_cuda, bsm, dtype):
    grid_run(torch_cuda, bsm, dtype, "A", 17, 24, "LM")


@pytest.mark.parametrize("side,which", [("A", "SM"), ("adjoint", "LM"), ("adjoint", "SM")])
@pytest.mark.parametrize("dtype", DTYPES, ids=name)
def test_two_and_three_workgroups_restarts_and_the_adjoint(torch_cuda, bsm, dtype, side, which):
    grid_run(torch_cuda, bsm, dtype, side, 3, 8, which)


@pytest.mark.parametrize("dtype,side", [(np.float64, "A"), (np.complex64, "adjoint")], ids=lambda v: v if isinstance(v, str) else name(v))
def test_host_u_at_its_own_leading_dimension(torch_cuda, bsm, dtype, side):
    grid_run(torch_cuda, bsm, dtype, side, 3, 8, "LM", host_u=True)


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
def test_ncv_equal_to_the_short_side(torch_cuda, bsm, dtype):
    p, D = diagonal_problem(dtype, np.linspace(1, 3, 12))
    v0 = np.random.default_rng(5).uniform(-1, 1, 12).astype(dtype)
    s, U, V, info = bsm.Svds(bsm.synthetic.build(p), nsv=2, ncv=12, which="LM").solve(dev(torch_cuda, v0), rtol=svd_rtol(dtype))
    accept(s, U, V, info, D, svds_twin(D, v0, 2, 12, "LM", svd_rtol(dtype)), 2, 12, "LM", dtype, f"ncv = n = 12 {name(dtype)}")


# ---- decisions and statuses, on operators of order 12 -------------------------------------------------------------------------
def test_statuses(torch_cuda, bsm):
    torch = torch_cuda
    for dtype in DTYPES:
        eps = float(np.finfo(dtype).eps)
        p, D = diagonal_problem(dtype, np.arange(12.0, 0.0, -1.0))
        A = bsm.synthetic.build(p)
        e1 = np.zeros(12, dtype)
        e1[0] = 1
        # e_1 spans an invariant pair of subspaces of dimension 1: one triplet wanted is convergence, two are status 3
        s, U, V, info = bsm.Svds(A, nsv=1, ncv=3).solve(dev(torch, e1))
        assert info.status == 0 and info.nconv == 1 and info.cycles == 1 and s.tolist() == [12.0] and np.all(info.estimate == 0)
        assert np.array_equal(np.abs(U.cpu().numpy()[:, 0]), np.abs(e1)) and np.array_equal(np.abs(V.cpu().numpy()[:, 0]), np.abs(e1))
        assert info.residual_av[0] == 0 and info.residual_ahu[0] == 0
        Un = torch.full((2, 12), 7.0, dtype=torch_dtype(torch, dtype), device="cuda").t()
        Vn = torch.full((2, 12), 7.0, dtype=torch_dtype(torch, dtype), device="cuda").t()
        s, U, V, info = bsm.Svds(A, nsv=2, ncv=4).solve(dev(torch, e1), U=Un, V=Vn)
        assert info.status == 3 and info.nconv == 1 and len(s) == 1 and s[0] == 12.0
        assert bool((Un[:, 1] == 7.0).all()) and bool((Vn[:, 1] == 7.0).all()) and abs(abs(complex(Un[0, 0])) - 1) == 0
        # status 3 with nothing: a zero start vector; U, V are not written
        s, U, V, info = bsm.Svds(A, nsv=2, ncv=4).solve(dev(torch, np.zeros(12, dtype)), U=Un, V=Vn)
        assert info.status == 3 and info.nconv == 0 and len(s) == 0 and bool((Un[:, 1] == 7.0).all()) and bool((Vn[:, 1] == 7.0).all())
        # status 1: one cycle of a three-dimensional space
        v0 = np.random.default_rng(5).uniform(-1, 1, 12).astype(dtype)
        s, U, V, info = bsm.Svds(A, nsv=1, ncv=3).solve(dev(torch, v0), rtol=svd_rtol(dtype), maxcycles=1)
        assert info.status == 1 and info.nconv == 1 and info.cycles == 1 and info.a_products == 2 * 3 + 2
        assert info.estimate[0] > svd_rtol(dtype) * info.anorm
        assert abs(np.hypot(info.residual_av[0], info.residual_ahu[0]) - info.estimate[0]) <= 2 * (12 + 3 + 2) * eps * info.anorm
        s, U, V, info = bsm.Svds(A, nsv=1, ncv=3).solve(dev(torch, v0), rtol=svd_rtol(dtype))
        assert info.status == 0 and abs(s[0] - 12) <= np.hypot(info.residual_av[0], info.residual_ahu[0]) + 12 * eps * 12
        # status 2: a NaN entry; nothing is written to U, V
        q = copied(p)
        q["blocks"][0][2, 2] = np.nan
        Un.fill_(7.0), Vn.fill_(7.0)
        s, U, V, info = bsm.Svds(bsm.synthetic.build(q), nsv=2, ncv=4).solve(dev(torch, v0), U=Un, V=Vn)
        assert info.status == 2 and info.nconv == 0 and len(s) == 0 and bool((Un == 7.0).all()) and bool((Vn == 7.0).all())
        # a row and a column no block covers, the start vector in that null space: alpha_0 = 0 exactly -- sigma = 0, v = e_12, the
        # recurrence offers no left vector (u = 0), both residuals are zero
        pb, Db = bordered_problem(dtype)
        e12 = np.zeros(12, dtype)
        e12[11] = 1
        s, U, V, info = bsm.Svds(bsm.synthetic.build(pb), nsv=1, ncv=3, which="SM").solve(dev(torch, e12))
        assert info.status == 0 and info.nconv == 1 and s[0] == 0.0 and info.residual_av[0] <= 12 * eps and info.residual_ahu[0] <= 12 * eps
        assert np.array_equal(np.abs(V.cpu().numpy()[:, 0]), np.abs(e12)) and not U.cpu().numpy().any()
        # and from a general start vector at ncv = n: the smallest value of the whole space is zero to the accuracy of the method
        s, U, V, info = bsm.Svds(bsm.synthetic.build(pb), nsv=1, ncv=12, which="SM").solve(dev(torch, v0), rtol=svd_rtol(dtype))
        assert info.status == 0 and s[0] <= 12 * eps * info.anorm and info.residual_av[0] <= 2 * (12 + 12 + 2) * eps * info.anorm
        assert abs(abs(V.cpu().numpy()[11, 0]) - 1) <= 64 * eps


def test_vectors_off_leaves_u_and_v_untouched(torch_cuda, bsm):
    torch = torch_cuda
    A, _, _, _, v0 = svd_dense(np.float64)
    H = handle(bsm, "vbcrs", np.float64)
    rc, ptr = raw_svds_create(H, 0, 1, 4, 20)
    assert rc == 0
    try:
        vd = dev(torch, v0)
        Ud = torch.full((4, M600), 7.0, dtype=torch.float64, device="cuda")
        Vd = torch.full((4, N400), 7.0, dtype=torch.float64, device="cuda")
        st = torch.cuda.current_stream().cuda_stream
        rc, info, trip = raw_svds_solve(ptr, 4, vd.data_ptr(), Ud.data_ptr(), M600, Vd.data_ptr(), N400, vectors=0, stream=st)
        assert rc == 0 and info.status == 0 and info.nconv == 4 and bool((Ud == 7.0).all()) and bool((Vd == 7.0).all())
        assert all(trip[i].residual_ahu == trip[i].estimate and trip[i].residual_av == 0 for i in range(4))
        assert info.workspace_bytes > (21 * N400 + 20 * M600) * 8
        rc, info2, _ = raw_svds_solve(ptr, 4, vd.data_ptr(), None, 0, None, 0, vectors=0, stream=st)  # U, V may be NULL then
        assert rc == 0 and info2.a_products == info.a_products == 2 * steps_of(4, 20, info.cycles)
    finally:
        assert raw_svds_destroy(ptr) == 0


# ---- determinism --------------------------------------------------------------------------------------------------------------
def test_two_solves_give_the_same_bytes_on_a_transpose_image_handle(torch_cuda, bsm):
    """one product per step is a transposed one: on a transpose_image handle of the conflict-free VBCRS kind both are forward
    passes with exclusive stores"""
    torch = torch_cuda
    A, _, _, _, v0 = svd_dense(np.float64)
    H = handle(bsm, "vbcrs", np.float64, transpose_image=True)
    vd = dev(torch, v0)
    for op, x in ((H, vd), (bsm.adjoint(H), dev(torch, np.random.default_rng(2).uniform(-1, 1, M600)))):
        ys = []
        for _ in range(2):
            y = torch.empty(bsm.size(op)[0], dtype=torch.float64, device="cuda")
            bsm.mul(y, op, x)
            torch.cuda.synchronize()
            ys.append(y.cpu().numpy().tobytes())
        assert ys[0] == ys[1], "the products of this handle are not reproducible"
    S = bsm.Svds(H, nsv=5, ncv=12, which="LM")
    runs = [S.solve(vd) for _ in range(2)] + [bsm.Svds(H, nsv=5, ncv=12, which="LM").solve(vd)]
    for s, U, V, info in runs[1:]:
        assert s.tobytes() == runs[0][0].tobytes() and U.cpu().numpy().tobytes() == runs[0][1].cpu().numpy().tobytes()
        assert V.cpu().numpy().tobytes() == runs[0][2].cpu().numpy().tobytes()
        for f in ("status", "nconv", "cycles", "a_products", "anorm"):
            assert getattr(info, f) == getattr(runs[0][3], f), f
        for f in ("estimate", "residual_av", "residual_ahu"):
            assert getattr(info, f).tobytes() == getattr(runs[0][3], f).tobytes(), f
    assert runs[0][3].cycles > 2  # restarts are part of what is compared


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_of_create(torch_cuda, bsm):
    from bsm_amd import _lib as L
    from _ctors import ctor_build
    f32, f64, c64, c128 = 0, 1, 2, 3
    p = svd_problem("blocksparse", np.float64)[0]
    H = handle(bsm, "blocksparse", np.float64)
    Hc = handle(bsm, "vbcrs", np.complex128)

    def refused(code, A, op, vt, nsv, ncv, null_out=False):
        rc, out = raw_svds_create(A, op, vt, nsv, ncv, null_out)
        assert rc == code and (null_out or not out.value), (rc, L.lib().bsm_last_error().decode())
    refused(ERR_INVALID, None, 0, f64, 4, 20)
    refused(ERR_INVALID, H, 0, f64, 4, 20, null_out=True)
    refused(ERR_INVALID, H, 3, f64, 4, 20)
    refused(ERR_INVALID, H, -1, f64, 4, 20)
    for vt in (4, 5, -1, 6):  # the mixed storage codes are no vector types
        refused(ERR_INVALID, H, 0, vt, 4, 20)
    refused(ERR_INVALID, H, 0, f32, 4, 20)   # a vector type other than the handle's own
    refused(ERR_INVALID, H, 0, c128, 4, 20)  # a real handle under a complex vdtype has no use here
    refused(ERR_INVALID, Hc, 0, f64, 4, 20)
    refused(ERR_INVALID, handle(bsm, "blocksparse", np.float64, storage=np.float32), 0, f32, 4, 20)  # mixed storage solves in double
    refused(ERR_UNSUPPORTED, Hc, 1, c128, 4, 20)  # transpose of a complex handle: op(A)^H would be conj(A)
    assert "conj(A)" in L.lib().bsm_last_error().decode()
    refused(ERR_UNSUPPORTED, handle(bsm, "vbcrs", np.complex128, storage=np.complex64), 1, c128, 4, 20)
    for nsv, ncv in [(0, 20), (-1, 20), (4, 5), (4, 4), (4, 0), (4, 129), (4, 400), (126, 127), (127, 128)]:
        refused(ERR_INVALID, H, 0, f64, nsv, ncv)
        refused(ERR_INVALID, H, 2, f64, nsv, ncv)
    p12, _ = diagonal_problem(np.float64, np.arange(1.0, 13.0))
    refused(ERR_INVALID, bsm.synthetic.build(p12), 0, f64, 4, 13)  # ncv > min(m, n)
    wide = dict(kind="vbcrs", blocks=[np.asfortranarray(np.ones((6, 9)))], rowstart=np.array([1], np.int64), colstart=np.array([1], np.int64),
                size=(6, 9))
    W = bsm.synthetic.build(wide)
    refused(ERR_INVALID, W, 0, f64, 1, 7)  # ncv > the SHORT side, whichever it is
    refused(ERR_INVALID, W, 2, f64, 1, 7)
    rc, ptr = raw_svds_create(W, 0, f64, 1, 6)  # not square: the point here
    assert rc == 0 and ptr.value and raw_svds_destroy(ptr) == 0
    refused(ERR_UNSUPPORTED, bsm.neumann(bsm.synthetic.build(p12), 0.1, 2), 0, f64, 2, 6)  # a composed handle
    assert "composed" in L.lib().bsm_last_error().decode()
    refused(ERR_UNSUPPORTED, ctor_build(bsm, "blocksparse", p, devices=[0, 0]), 0, f64, 4, 20)
    refused(ERR_DEVICE, bsm.synthetic.build(p, device=-2), 0, f64, 4, 20)
    pv = svd_problem("vbcrs", np.float64)[0]
    keep = [i for i, r0 in enumerate(pv["rowstart"]) if 101 <= r0 <= 201]
    sub = dict(kind="vbcrs", blocks=[pv["blocks"][i] for i in keep], rowstart=pv["rowstart"][keep], colstart=pv["colstart"][keep], size=pv["size"])
    refused(ERR_UNSUPPORTED, bsm.synthetic.build(sub, own=(101, 300)), 0, f64, 4, 20)
    assert "own a row range" in L.lib().bsm_last_error().decode()
    with pytest.raises(bsm._lib.BsmError, match="ncv"):
        bsm.Svds(H, nsv=4, ncv=401)
    with pytest.raises(bsm._lib.BsmError, match="conj"):
        bsm.Svds(bsm.transpose(Hc), nsv=4)
    with pytest.raises(ValueError, match="which"):
        bsm.Svds(H, which="LA")
    # the widest and the narrowest that pass
    for nsv, ncv in [(126, 128), (1, 3)]:
        rc, ptr = raw_svds_create(H, 0, f64, nsv, ncv)
        assert rc == 0 and ptr.value and raw_svds_destroy(ptr) == 0


def test_refusals_of_solve(torch_cuda, bsm):
    from bsm_amd import _lib as L
    torch = torch_cuda
    H = handle(bsm, "blocksparse", np.float64)
    v0 = svd_dense(np.float64)[4]
    rc, ptr = raw_svds_create(H, 0, 1, 4, 20)
    assert rc == 0
    try:
        vd = dev(torch, v0)
        ubuf = torch.full((5 * M600,), 7.0, dtype=torch.float64, device="cuda")
        vbuf = torch.full((5 * N400,), 7.0, dtype=torch.float64, device="cuda")
        v, u, w, st = vd.data_ptr(), ubuf.data_ptr(), vbuf.data_ptr(), torch.cuda.current_stream().cuda_stream
        good = (ptr, 4, v, u, M600, w, N400)
        for what, args, kw in [("null v0", (ptr, 4, None, u, M600, w, N400), {}), ("null U", (ptr, 4, v, None, M600, w, N400), {}),
                               ("null V", (ptr, 4, v, u, M600, None, N400), {}), ("ldu", (ptr, 4, v, u, M600 - 1, w, N400), {}),
                               ("ldv", (ptr, 4, v, u, M600, w, N400 - 1), {}), ("null p", good, dict(null=("p",))),
                               ("null info", good, dict(null=("info",))), ("null triplets", good, dict(null=("triplets",))),
                               ("struct size", good, dict(struct_size=24)), ("memspace", good, dict(memspace=2)), ("which", good, dict(which=2)),
                               ("which negative", good, dict(which=-1)), ("negative rtol", good, dict(rtol=-1e-3)),
                               ("NaN rtol", good, dict(rtol=float("nan"))), ("negative atol", good, dict(atol=-1.0)),
                               ("NaN atol", good, dict(atol=float("nan"))), ("maxcycles", good, dict(maxcycles=0)),
                               ("V inside U", (ptr, 4, v, u, M600, u + 8 * M600, N400), {}), ("U is V", (ptr, 4, v, u, M600, u, N400), {}),
                               ("V just into the last column of U", (ptr, 4, v, u, M600, u + 8 * (4 * M600 - 1), N400), {})]:
            assert raw_svds_solve(*args, stream=st, **kw)[0] == ERR_INVALID, what
        assert raw_svds_solve(None, 4, v, u, M600, w, N400, stream=st)[0] == ERR_INVALID  # null S
        # v0 inside U, inside V, and just behind the last column of V (no overlap)
        big = torch.zeros(5 * N400, dtype=torch.float64, device="cuda")
        big[3 * N400 + 5:4 * N400 + 5] = vd
        assert raw_svds_solve(ptr, 4, big.data_ptr() + (3 * N400 + 5) * 8, u, M600, big.data_ptr(), N400, stream=st)[0] == ERR_INVALID
        assert raw_svds_solve(ptr, 4, u + 16, u, M600, w, N400, stream=st)[0] == ERR_INVALID
        big[4 * N400:] = vd
        rc, info, _ = raw_svds_solve(ptr, 4, big.data_ptr() + 4 * N400 * 8, u, M600, big.data_ptr(), N400, stream=st)
        assert rc == 0 and info.status == 0
        ubuf.fill_(7.0)
        # a capturing stream
        torch.cuda.synchronize()
        scratch = torch.zeros(4, device="cuda")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            scratch.zero_()
            rc = raw_svds_solve(*good, stream=torch.cuda.current_stream().cuda_stream)[0]
            why = L.lib().bsm_last_error().decode()
        assert rc == ERR_INVALID and "graph-captured" in why
        torch.cuda.synchronize()
        assert bool((ubuf == 7.0).all()) and bool((vbuf == 7.0).all()), "a refused solve wrote U or V"
    finally:
        assert raw_svds_destroy(ptr) == 0
    # the Python layer's own checks
    S = bsm.Svds(H, nsv=4, ncv=20)
    with pytest.raises(ValueError, match="nsv"):
        S.solve(vd, U=torch.empty((3, M600), dtype=torch.float64, device="cuda").t())
    with pytest.raises((TypeError, ValueError)):
        S.solve(vd.to(torch.float32))
    with pytest.raises((TypeError, ValueError)):
        S.solve(dev(torch, np.ones(M600)))  # v0 has min(m, n) entries
