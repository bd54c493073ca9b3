"""Every device solver (Cg / COCG, BiCgStab, Minres, GmresMulti, Gmres: the table of _lockstep.py) on every kind of handle a
product can run on, and one solver object across new block values.  The solvers' own suites build every operator with
default options; here the product under the solver's padded workspace takes the other routes of bsm_mul_multi:

  A1  accumulate="gather" on A and M: five columns (the atomic path) and one (the bitwise reproducible gather workspace:
      same bytes from two solves on one solver and from a second solver object), float32 / complex64 included;
  A2  accumulate="colored" on A and M: acceptance, the same bytes twice, the pass count of a solve cut at its count;
  A3  transpose_image=True: transpose(A) / adjoint(A) run forward on the second image; pass count, both images counted;
  A4  device-resident blocks, on a side stream;
  A5  storage=float32 A with a coloured M; a real A from device blocks under complex B;
  B1  update_blocks(A, the blocks that hold a diagonal entry, ids=...), M.refresh(), the SAME solver again: acceptance on
      the new values D2 (_lockstep.shifted);  B2 on a transpose_image handle, solving with transpose(A);  B3 with
      device-resident blocks, everything on a side stream without a synchronisation in between;  B4 the bytes of the
      post-update solve against objects built fresh from D2, on the reproducible configurations of A1 / A2;  B5 a Cg and a
      GmresMulti on one pair of handles, called alternately;
  C   a handle that owns a row range only (own=(lo, hi), the per-rank handle of distributed.py) is refused by all five
      create calls -- its forward product defines the owned rows of y only --, the whole range (1, n) is accepted.

Acceptance is the solver's own (Solver.accept calls the helper of its suite: the count against the numpy twin within that
suite's slack, the true residual in complex128 within its factor); no tolerance is new.  test_solver_handles_cpu.py shows
that the update legs see stale values of A and of M, and that every mode builds.  Figures are printed in HANDSTAT lines.

Pass counts.  The expected figure is (passes of ONE plain bsm.mul of the same width on the handle) x info.a_products, with
info.a_products as the solver's own pass-count test states it; Gmres's suite has no such test, so no pass count is asserted
for it.  What one product costs follows from bsm_value_passes and the batch plan (csrc/bsm_plan.cpp): five columns of a
handle's own vector type are ONE batch of the multi-RHS kernels, on a coloured image too (one stream of the values however
many colour launches), and on a transpose_image handle op T is one batch on the second image; columns run one at a time,
five passes per product, where a coloured image keeps the interleaved pass away from a pair that has no multi-RHS kernels:
complex vectors under a real coloured image (the last leg of A2)."""
import numpy as np
import pytest

from _common import Cc, N, T, wrap
from _gpu import dev_copy, passes_of_one_product, same_bytes, same_products, torch_cuda  # noqa: F401
from _jacobi import CODE, uniform
from _krylov import ERR_UNSUPPORTED, exact_minv
from _lockstep import SINGLE_TYPES, WIDE_TYPES, case_id, shifted, solver_cases, solvers
from _submat import Truth
from _values import copied, on_device

pytestmark = pytest.mark.gpu

SHARED = ("blocksparse", "symmetric")  # kinds whose rows are shared by several blocks: the default mode uses atomics
LOCKSTEP = ("cg", "cocg", "bicgstab", "minres", "gmres_multi")


def name(dtype):
    return np.dtype(dtype).name


def op_of(D, op):
    return D if op == N else np.ascontiguousarray(D.T if op == T else D.conj().T)


@pytest.fixture(scope="module")
def twins():
    """get(R, c, kind, tag, D, P, B) -> the twin's runs on the columns of B with the exact block inverse of P; `tag` names
    (D, P, B) among the variants of one (solver, type): the dense operator of cg / cocg / bicgstab / minres does not depend
    on its cut, so their runs are shared between the kinds"""
    cache = {}

    def get(R, c, kind, tag, D, P, B, rtol=None):
        key = (R.name, kind if R.name in ("gmres", "gmres_multi") else None, name(B.dtype), tag)
        if key not in cache:
            cache[key] = R.runs(D, B, exact_minv(P, c.sets).astype(B.dtype), B.dtype.type, rtol)
        return cache[key]
    return get


def handles(bsm, c, akw=None, mkw=None, op=N, torch=None, p=None, pm=None):
    """-> (A, the handle M is built from, M = block_jacobi(op(that handle), sets)); torch: the blocks go to the device first.
    The handles hold COPIES of the problem's blocks: update_blocks writes into the blocks a handle was built from, and the
    problems are shared between the tests"""
    p, pm = c.p if p is None else p, c.pm if pm is None else pm
    same = pm is p
    move = copied if torch is None else (lambda q: on_device(torch, q))
    p = move(p)
    pm = p if same else move(pm)
    A = bsm.synthetic.build(p, **(akw or {}))
    Am = A if same else bsm.synthetic.build(pm, **(akw or {}))
    return A, Am, bsm.block_jacobi(wrap(bsm, Am, op), c.sets, **(mkw or {}))


def check_pass_count(torch, bsm, R, S, A, M, Aop, Bd, first, per, what):
    """the equality of the solver's own pass-count test on a solve cut at the count of the free-running `first`, every
    product counted `per` times (module docstring)"""
    assert passes_of_one_product(torch, bsm, A, Aop, Bd) == per[0] and passes_of_one_product(torch, bsm, M, M, Bd) == per[1], what
    before = A.value_passes(), M.value_passes()
    X, info = R.solve(S, Bd, maxiter=int(first.iterations))
    da, dm = A.value_passes() - before[0], M.value_passes() - before[1]
    print(f"HANDSTAT passes {R.name} {what}: {info.iterations} iterations, a_products {info.a_products}, passes over A {da} at {per[0]} "
          f"per product; m_products {info.m_products}, passes over M {dm} at {per[1]} per product")
    assert info.status == 0 and info.iterations == first.iterations
    assert info.a_products == R.passes(info, first) and da == per[0] * info.a_products
    if R.m_passes:
        assert info.m_products == info.iterations + 1 and dm == per[1] * info.m_products


# ---- A1. accumulate="gather" ---------------------------------------------------------------------------------------------
A1_FIVE = solver_cases(WIDE_TYPES + SINGLE_TYPES, SHARED, LOCKSTEP)
A1_ONE = solver_cases(WIDE_TYPES + SINGLE_TYPES, SHARED)


@pytest.mark.parametrize("case", A1_FIVE, ids=case_id)
def test_gather_handles_five_columns(torch_cuda, bsm, twins, case):
    torch, (sname, kind, dtype) = torch_cuda, case
    R = solvers()[sname]
    c = R.case(kind, dtype)
    A, _, M = handles(bsm, c, dict(accumulate="gather"), dict(accumulate="gather"))
    assert A.stats()["exclusive"] == 0
    X, info = R.solve(R.make(bsm, A, M), dev_copy(torch, c.B))
    R.accept(info, twins(R, c, kind, "N", c.D, c.P, c.B), c.D, X.cpu().numpy(), c.B, f"A1 gather x5 {kind} {name(dtype)}")


@pytest.mark.parametrize("case", A1_ONE, ids=case_id)
def test_gather_handles_one_column_reproduces_its_bytes(torch_cuda, bsm, twins, case):
    torch, (sname, kind, dtype) = torch_cuda, case
    R = solvers()[sname]
    c = R.case(kind, dtype)
    A, _, M = handles(bsm, c, dict(accumulate="gather"), dict(accumulate="gather"))
    b = np.asfortranarray(c.B[:, :1])
    Bd = dev_copy(torch, b)
    same_products(torch, bsm, Bd, A, M)
    S = R.make(bsm, A, M, nrhs=1)
    one, two, other = R.solve(S, Bd), R.solve(S, Bd), R.solve(R.make(bsm, A, M, nrhs=1), Bd)
    same_bytes(one, two, "two solves on one solver")
    same_bytes(one, other, "a second solver object")
    R.accept(one[1], twins(R, c, kind, "N", c.D, c.P, c.B)[:1], c.D, one[0].cpu().numpy(), b, f"A1 gather x1 {kind} {name(dtype)}")


# ---- A2. accumulate="colored" --------------------------------------------------------------------------------------------
A2 = solver_cases(WIDE_TYPES, SHARED)


@pytest.mark.parametrize("case", A2, ids=case_id)
def test_colored_handles(torch_cuda, bsm, twins, case):
    torch, (sname, kind, dtype) = torch_cuda, case
    R = solvers()[sname]
    c = R.case(kind, dtype)
    A, _, M = handles(bsm, c, dict(accumulate="colored"), dict(accumulate="colored"))
    Bd = dev_copy(torch, c.B)
    S = R.make(bsm, A, M)
    one, two = R.solve(S, Bd), R.solve(S, Bd)
    R.accept(one[1], twins(R, c, kind, "N", c.D, c.P, c.B), c.D, one[0].cpu().numpy(), c.B, f"A2 colored {kind} {name(dtype)}")
    same_bytes(one, two, "two solves on one solver")
    if R.passes is not None:
        check_pass_count(torch, bsm, R, S, A, M, A, Bd, one[1], (1, 1), f"A2 colored {kind} {name(dtype)}")


A2_CVEC = [("cg", "symmetric"), ("bicgstab", "blocksparse"), ("minres", "symmetric"), ("gmres_multi", "blocksparse")]


def complex_columns(B, seed):
    return np.asfortranarray((B + 1j * uniform(np.random.default_rng(seed), B.shape, np.float64)).astype(np.complex128))


@pytest.mark.parametrize("sname, kind", A2_CVEC, ids=[f"{s}-{k}" for s, k in A2_CVEC])
def test_colored_real_handles_under_complex_columns_run_them_one_at_a_time(torch_cuda, bsm, twins, sname, kind):
    torch, dtype = torch_cuda, np.float64
    R = solvers()[sname]
    c = R.case(kind, dtype)
    Bc = complex_columns(c.B, 4200)
    A, _, M = handles(bsm, c, dict(accumulate="colored"), dict(accumulate="colored"))
    Bd = dev_copy(torch, Bc)
    S = R.make(bsm, A, M, dtype=np.complex128)
    one, two = R.solve(S, Bd), R.solve(S, Bd)
    Dc = c.D.astype(np.complex128)
    runs = twins(R, c, kind, "complex B", Dc, c.P.astype(np.complex128), Bc)
    R.accept(one[1], runs, Dc, one[0].cpu().numpy(), Bc, f"A2 colored cvec {kind}")
    same_bytes(one, two, "two solves on one solver")
    check_pass_count(torch, bsm, R, S, A, M, A, Bd, one[1], (Bc.shape[1], Bc.shape[1]), f"A2 colored cvec {kind}")


# ---- A3. transpose_image=True ----------------------------------------------------------------------------------------------
A3 = [(s, k, dt, op) for s in ("bicgstab", "gmres_multi") for k in ("vbcrs", "blocksparse") for dt in WIDE_TYPES
      for op in ((T,) if dt is np.float64 else (T, Cc))] + [("cg", k, np.complex128, T) for k in ("vbcrs", "blocksparse")]
OPNAME = {N: "N", T: "T", Cc: "C"}


@pytest.mark.parametrize("case", A3, ids=[f"{s}-{k}-{name(dt)}-{OPNAME[op]}" for s, k, dt, op in A3])
def test_transposed_solves_on_the_second_image(torch_cuda, bsm, twins, case):
    """bicgstab / gmres_multi: D is not symmetric, so a forward product in place of the transposed one fails the acceptance;
    cg on the Hermitian variant: transpose(A) is conj(D), Hermitian again"""
    torch, (sname, kind, dtype, op) = torch_cuda, case
    R = solvers()[sname]
    c = R.case(kind, dtype)
    Dt, Pt = op_of(c.D, op), op_of(c.P, op)
    assert not np.array_equal(Dt, c.D)
    A, _, M = handles(bsm, c, dict(transpose_image=True), dict(transpose_image=True), op=op)
    Aop = wrap(bsm, A, op)
    Bd = dev_copy(torch, c.B)
    S = R.make(bsm, Aop, M)
    X, first = R.solve(S, Bd)
    what = f"A3 second image {kind} {name(dtype)} op {OPNAME[op]}"
    R.accept(first, twins(R, c, kind, OPNAME[op], Dt, Pt, c.B), Dt, X.cpu().numpy(), c.B, what)
    check_pass_count(torch, bsm, R, S, A, M, Aop, Bd, first, (1, 1), what)


# ---- A4. device-resident blocks, a side stream ---------------------------------------------------------------------------
A4 = [("cg", "vbcrs", np.float64), ("cg", "blocksparse", np.complex128), ("cocg", "symmetric", np.complex128),
      ("bicgstab", "blocksparse", np.float64), ("bicgstab", "vbcrs", np.complex128), ("minres", "symmetric", np.float64),
      ("minres", "vbcrs", np.complex128), ("gmres_multi", "vbcrs", np.float64), ("gmres_multi", "symmetric", np.complex128),
      ("gmres", "blocksparse", np.float64), ("gmres", "symmetric", np.complex128)]


@pytest.mark.parametrize("case", A4, ids=case_id)
def test_device_resident_blocks_on_a_side_stream(torch_cuda, bsm, twins, case):
    torch, (sname, kind, dtype) = torch_cuda, case
    R = solvers()[sname]
    c = R.case(kind, dtype)
    A, _, M = handles(bsm, c, torch=torch)
    Bd = dev_copy(torch, c.B)
    torch.cuda.synchronize()
    X, info = R.solve(R.make(bsm, A, M), Bd, stream=torch.cuda.Stream())
    R.accept(info, twins(R, c, kind, "N", c.D, c.P, c.B), c.D, X.cpu().numpy(), c.B, f"A4 device blocks {kind} {name(dtype)}")


# ---- A5. mixed cases ---------------------------------------------------------------------------------------------------------
A5 = [("minres", "symmetric"), ("gmres_multi", "blocksparse")]


@pytest.mark.parametrize("sname, kind", A5, ids=[f"{s}-{k}" for s, k in A5])
def test_single_precision_storage_with_a_colored_preconditioner(torch_cuda, bsm, twins, sname, kind):
    """the operator IS the rounded one (test_single_precision_storage_under_double_vectors of the solvers' suites): the twin
    runs on the blocks rounded to float32, M is built from the stored values"""
    torch, dtype = torch_cuda, np.float64
    R = solvers()[sname]
    c = R.case(kind, dtype)
    D32, P32 = Truth(c.p, np.float32).D, Truth(c.pm, np.float32).D
    A, _, M = handles(bsm, c, dict(storage=np.float32), dict(accumulate="colored"))
    X, info = R.solve(R.make(bsm, A, M), dev_copy(torch, c.B))
    assert X.dtype == torch.float64
    runs = twins(R, c, kind, "float32 storage", D32, P32, c.B)
    R.accept(info, runs, D32, X.cpu().numpy(), c.B, f"A5 float32 storage, coloured M, {kind}")


A5_CVEC = [("minres", "vbcrs"), ("gmres_multi", "blocksparse")]


@pytest.mark.parametrize("sname, kind", A5_CVEC, ids=[f"{s}-{k}" for s, k in A5_CVEC])
def test_real_device_blocks_under_complex_columns(torch_cuda, bsm, twins, sname, kind):
    torch, dtype = torch_cuda, np.float64
    R = solvers()[sname]
    c = R.case(kind, dtype)
    Bc = complex_columns(c.B, 4200)
    A, _, M = handles(bsm, c, torch=torch)
    X, info = R.solve(R.make(bsm, A, M, dtype=np.complex128), dev_copy(torch, Bc))
    assert X.dtype == torch.complex128
    Dc = c.D.astype(np.complex128)
    runs = twins(R, c, kind, "complex B", Dc, c.P.astype(np.complex128), Bc)
    R.accept(info, runs, Dc, X.cpu().numpy(), Bc, f"A5 device blocks, complex B, {kind}")


# ---- B. one solver object across new values --------------------------------------------------------------------------------
def update_and_solve_again(torch, bsm, twins, R, c, kind, what, akw=None, mkw=None, op=N, device=False, stream=None, ncols=None):
    """build from D1, solve, update_blocks with exactly the blocks that hold a diagonal entry, M.refresh(), the SAME solver
    again -> ((X, info) after the update, the objects (A, Am, M, S), the shift).  Acceptance on op(D1), then on op(D2)"""
    B = c.B if ncols is None else np.asfortranarray(c.B[:, :ncols])
    A, Am, M = handles(bsm, c, akw, mkw, op=op, torch=torch if device else None)
    S = R.make(bsm, wrap(bsm, A, op), M, nrhs=ncols)
    Bd = dev_copy(torch, B)
    torch.cuda.synchronize()
    X, info = R.solve(S, Bd, stream=stream)
    D1, P1 = op_of(c.D, op), op_of(c.P, op)
    R.accept(info, twins(R, c, kind, OPNAME[op], D1, P1, c.B)[:B.shape[1]], D1, X.cpu().numpy(), B, what + " before")
    sh = shifted(c)
    conv = (lambda b: dev_copy(torch, b)) if device else (lambda b: b)
    new, mnew = [conv(b) for b in sh.new], [conv(b) for b in sh.mnew]
    bsm.update_blocks(A, new, ids=sh.ids, stream=stream)
    if Am is not A:
        bsm.update_blocks(Am, mnew, ids=sh.mids, stream=stream)
    M.refresh(stream=stream)
    X2, info2 = R.solve(S, Bd, stream=stream)
    D2, P2 = op_of(sh.D2, op), op_of(sh.P2, op)
    R.accept(info2, twins(R, c, kind, "2" + OPNAME[op], D2, P2, c.B)[:B.shape[1]], D2, X2.cpu().numpy(), B, what + " after")
    return (X2, info2), (A, Am, M, S, Bd), sh


B1 = solver_cases()


@pytest.mark.parametrize("case", B1, ids=case_id)
def test_update_refresh_and_the_same_solver_again(torch_cuda, bsm, twins, case):
    sname, kind, dtype = case
    R = solvers()[sname]
    update_and_solve_again(torch_cuda, bsm, twins, R, R.case(kind, dtype), kind, f"B1 {kind} {name(dtype)}")


B2 = solver_cases(WIDE_TYPES, ("vbcrs", "blocksparse"), ("bicgstab", "gmres_multi"))


@pytest.mark.parametrize("case", B2, ids=case_id)
def test_update_reaches_the_second_image(torch_cuda, bsm, twins, case):
    """after the update the solve runs transpose(A) forward on the second image: a refill that missed it solves with D1^T"""
    sname, kind, dtype = case
    R = solvers()[sname]
    update_and_solve_again(torch_cuda, bsm, twins, R, R.case(kind, dtype), kind, f"B2 {kind} {name(dtype)}", dict(transpose_image=True),
                           dict(transpose_image=True), op=T)


@pytest.mark.parametrize("case", B1, ids=case_id)
def test_update_of_device_resident_blocks_on_a_side_stream(torch_cuda, bsm, twins, case):
    """update_blocks(A, device tensors, ids, stream=side), M.refresh(stream=side), S.solve(..., stream=side): nothing waits in
    between but the streams' own order"""
    sname, kind, dtype = case
    R = solvers()[sname]
    update_and_solve_again(torch_cuda, bsm, twins, R, R.case(kind, dtype), kind, f"B3 {kind} {name(dtype)}", device=True,
                           stream=torch_cuda.cuda.Stream())


B4 = [c + (m,) for c in solver_cases(WIDE_TYPES, SHARED) for m in ("gather-x1", "colored-x5")]


@pytest.mark.parametrize("case", B4, ids=case_id)
def test_updated_objects_give_the_bytes_of_fresh_ones(torch_cuda, bsm, twins, case):
    torch, (sname, kind, dtype, mode) = torch_cuda, case
    R = solvers()[sname]
    c = R.case(kind, dtype)
    acc = dict(accumulate=mode.split("-")[0])
    ncols = 1 if mode == "gather-x1" else None
    what = f"B4 {mode} {kind} {name(dtype)}"
    after, (A, _, M, _, Bd), sh = update_and_solve_again(torch, bsm, twins, R, c, kind, what, acc, acc, ncols=ncols)
    if mode == "gather-x1":
        same_products(torch, bsm, Bd, A, M)
    A2, _, M2 = handles(bsm, c, acc, acc, p=sh.p2, pm=sh.pm2)
    fresh = R.solve(R.make(bsm, A2, M2, nrhs=ncols), Bd)
    same_bytes(after, fresh, "updated objects against fresh ones")


def test_two_solver_objects_on_one_pair_of_handles(torch_cuda, bsm, twins):
    """Cg(A, M, nrhs=5) and GmresMulti(A, M, nrhs=3) on the SPD problem, alternately, three times each: each keeps passing its
    own acceptance; with one column each on gather handles, each reproduces its own bytes"""
    torch, dtype, kind = torch_cuda, np.float64, "blocksparse"
    cg, gm = solvers()["cg"], solvers()["gmres_multi"]
    c = cg.case(kind, dtype)
    B3 = np.asfortranarray(c.B[:, :3])
    A, _, M = handles(bsm, c)
    S5, S3 = cg.make(bsm, A, M, nrhs=5), gm.make(bsm, A, M, nrhs=3)
    B5d, B3d = dev_copy(torch, c.B), dev_copy(torch, B3)
    gruns = gm.runs(c.D, B3, exact_minv(c.P, c.sets), dtype)
    for turn in range(3):
        X, info = cg.solve(S5, B5d)
        cg.accept(info, twins(cg, c, kind, "N", c.D, c.P, c.B), c.D, X.cpu().numpy(), c.B, f"B5 cg turn {turn}")
        X, info = gm.solve(S3, B3d)
        gm.accept(info, gruns, c.D, X.cpu().numpy(), B3, f"B5 gmres_multi on the cg problem, turn {turn}")
    A, _, M = handles(bsm, c, dict(accumulate="gather"), dict(accumulate="gather"))
    b = np.asfortranarray(c.B[:, :1])
    Bd = dev_copy(torch, b)
    same_products(torch, bsm, Bd, A, M)
    S1, G1 = cg.make(bsm, A, M, nrhs=1), gm.make(bsm, A, M, nrhs=1)
    firsts = None
    for turn in range(3):
        got = cg.solve(S1, Bd), gm.solve(G1, Bd)
        if firsts is None:
            firsts = got
            cg.accept(got[0][1], twins(cg, c, kind, "N", c.D, c.P, c.B)[:1], c.D, got[0][0].cpu().numpy(), b, "B5 cg x1 gather")
            gm.accept(got[1][1], gruns[:1], c.D, got[1][0].cpu().numpy(), b, "B5 gmres_multi x1 gather")
        same_bytes(firsts[0], got[0], f"cg, turn {turn}")
        same_bytes(firsts[1], got[1], f"gmres_multi, turn {turn}")


# ---- C. the own-range slice ------------------------------------------------------------------------------------------------
def raw_creates(A, M, code):
    """the return code of every create entry point on (A, M); a solver that was created is destroyed"""
    from _bicgstab import raw_bicgstab_create, raw_bicgstab_destroy
    from _cg import raw_cg_create, raw_cg_destroy
    from _gmres_multi import raw_gm_create, raw_gm_destroy
    from _krylov import raw_gmres_create, raw_gmres_destroy
    from _minres import raw_minres_create, raw_minres_destroy
    calls = [("bsm_cg_create", lambda: raw_cg_create(A, 0, M, 0, code, 4), raw_cg_destroy),
             ("bsm_bicgstab_create", lambda: raw_bicgstab_create(A, 0, M, 0, code, 4), raw_bicgstab_destroy),
             ("bsm_minres_create", lambda: raw_minres_create(A, 0, M, 0, code, 4), raw_minres_destroy),
             ("bsm_gmres_multi_create", lambda: raw_gm_create(A, 0, M, 0, code, 4, 20), raw_gm_destroy),
             ("bsm_gmres_create", lambda: raw_gmres_create(A, 0, M, 0, code, 20), raw_gmres_destroy)]
    out = {}
    for entry, create, destroy in calls:
        rc, ptr = create()
        if rc == 0:
            assert destroy(ptr) == 0
        out[entry] = rc
    return out


@pytest.mark.parametrize("kind", ["vbcrs", "blocksparse", "symmetric"])
def test_a_handle_that_owns_a_row_range_is_refused(torch_cuda, bsm, kind):
    """the forward product of such a handle scales (and with the strong zero: defines) the owned rows of y only; the rows of
    Q = A P outside the range would keep what the previous iteration left in the workspace"""
    dtype = np.float64
    c = solvers()["cg"].case(kind, dtype)
    n = c.D.shape[0]
    whole, part = bsm.synthetic.build(c.p), bsm.synthetic.build(c.p, own=(101, 300))
    code = CODE[np.dtype(dtype)]
    assert set(raw_creates(whole, whole, code).values()) == {0}
    entries = ("bsm_cg_create", "bsm_bicgstab_create", "bsm_minres_create", "bsm_gmres_multi_create", "bsm_gmres_create")
    assert raw_creates(part, None, code) == raw_creates(part, whole, code) == raw_creates(whole, part, code) == \
        {e: ERR_UNSUPPORTED for e in entries}
    # the other two slices that are no whole range: from the first row, and up to the last
    for own in ((1, 300), (101, n)):
        assert set(raw_creates(bsm.synthetic.build(c.p, own=own), None, code).values()) == {ERR_UNSUPPORTED}
    for make in (bsm.Cg, bsm.BiCgStab, bsm.Minres, bsm.GmresMulti, bsm.Gmres):
        for args in ((part,), (part, whole), (whole, part)):
            with pytest.raises(bsm._lib.BsmError, match="own_lo / own_hi"):
                make(*args)


C_WHOLE = [("cg", "symmetric", np.float64), ("cocg", "vbcrs", np.complex128), ("bicgstab", "blocksparse", np.float64),
           ("minres", "blocksparse", np.complex128), ("gmres_multi", "symmetric", np.float64), ("gmres", "vbcrs", np.complex128)]


@pytest.mark.parametrize("case", C_WHOLE, ids=case_id)
def test_the_whole_own_range_is_accepted(torch_cuda, bsm, twins, case):
    torch, (sname, kind, dtype) = torch_cuda, case
    R = solvers()[sname]
    c = R.case(kind, dtype)
    A, _, M = handles(bsm, c, dict(own=(1, c.D.shape[0])))
    X, info = R.solve(R.make(bsm, A, M), dev_copy(torch, c.B))
    R.accept(info, twins(R, c, kind, "N", c.D, c.P, c.B), c.D, X.cpu().numpy(), c.B, f"C own=(1, n) {kind} {name(dtype)}")
