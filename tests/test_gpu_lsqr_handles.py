"""LSQR on every kind of handle a product can run on, and one Lsqr object across new block values: what
test_gpu_solver_handles.py does for the five older solvers.  Lsqr is the one solver that issues op(A)^H itself, once per
iteration, through bsm_mul_multi / bsm_mul_multi_cvec: every leg below runs the transposed multi-column route of its handle
mode as well as the forward one.  test_gpu_lsqr.py builds (nearly) every operator with default options.

  A1  accumulate="gather": five columns (the atomic path), and one (the gather workspace and, for op T / C, its inverted
      index: two plain products of A and of adjoint(A) give the same bytes, two solves on one solver and one on a second
      solver object give the same bytes of X and history);
  A2  accumulate="colored": acceptance, the same bytes twice, the pass count; a real coloured handle under complex128
      columns runs them one at a time, five passes per product;
  A3  transpose_image=True: one of the two products of every iteration runs on the second image; pass count, both images
      counted; on the VBCRS kind (conflict-free: exclusive stores on both images) the same bytes twice;
  A4  device-resident blocks, the solve on a side stream;
  A5  storage=float32 / complex64 under double vectors -- the adjoint of a mixed handle goes through the interleaved pass --
      against the twin on the ROUNDED operator; a real handle built from device blocks under complex columns;
  A6  the bordered problem (rows and columns no block covers) on default, gather, coloured and transpose_image handles: X is
      exactly zero where no block reaches, and on the reproducible configurations a solver that has just solved something
      else from a guess X0 (nonzero in those entries too) gives the bytes of a fresh one -- an entry of the workspace that a
      transposed product never defines and a kernel then reads would show;
  B1  update_blocks(A, new blocks, ids=...), the SAME solver again: acceptance on the old values, then on the new ones
      (VBCRS: block 1 negated; blocksparse: the ten blocks of the largest row set negated);  B2 on transpose_image handles,
      where every solve reads both images;  B3 device-resident new blocks, update and solve on a side stream with no
      synchronisation in between;  B4 on gather x 1 and coloured x 5 the post-update solve gives the bytes of objects built
      fresh from the new values;  B5 Lsqr(A) and Lsqr(adjoint(A)) on one handle, called alternately;
  C   a handle that owns a row range only is refused (raw call and bsm.Lsqr, on A and on adjoint(A)); own=(1, 600) solves.

Acceptance is _lsqr.check_columns exactly as test_gpu_lsqr.py uses it, with rtol = ntol = lsqr_rtol(dtype) and maxiter =
400; reproducibility is byte equality of X and history; no tolerance is new.  test_lsqr_handles_cpu.py pins the twin's counts
on every pair accepted against, shows that they keep to +-1 under permuted sums and that stale values, and a refill that
reached one image only, fail the acceptance.  Figures are printed in LSHSTAT lines before they are asserted.

Pass counts.  A solve of exactly k iterations without X0 issues k products with op(A) and k + 1 with op(A)^H: the handle's
value_passes() must grow by pf k + pa (k + 1), pf and pa being what ONE plain bsm.mul of the same width with the same wrapped
op adds on that handle.  k is the count of the free-running solve; the counted solve runs with rtol = ntol = 0, so that it
ends at maxiter = k and at nothing else (a solve that converges earlier has paid for the iteration enqueued ahead of its
last record, and on a handle whose transposed product uses atomics the count may move by one between two runs).  pf and pa
are also asserted against what csrc/bsm_plan.cpp prescribes: 1 and 1 for five columns of the handle's own type (coloured,
gather and second image included), for mixed storage and for complex columns under a real image (the interleaved pass), 5
and 5 for complex columns under a real coloured image."""
import numpy as np
import pytest

from _cg import ERR_UNSUPPORTED
from _gpu import dev_copy, passes_of_one_product, same_bytes, same_products, torch_cuda  # noqa: F401
from _jacobi import CODE, uniform
from _krylov import real_of
from _lsqr import (BORDER, LEGS, M600, N400, NB, bordered_problem, check_columns, check_products, leg_runs, leg_system, lsqr_problem, lsqr_rtol,
                   new_values, raw_lsqr_create, raw_lsqr_destroy, single_of, symmetric_problem, true_criteria)
from _values import copied, on_device

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64, np.complex64, np.complex128]
WIDE = [np.float64, np.complex128]
KINDS = ["vbcrs", "blocksparse"]


def name(dtype):
    return np.dtype(dtype).name


def problem_of(kind, dtype):
    """-> (problem, the operand of _lsqr.py's table it is the block form of)"""
    if kind == "symmetric":
        return symmetric_problem(dtype)[0], "symmetric"
    if kind == "bordered":
        return bordered_problem(dtype)[0], "bordered"
    return lsqr_problem(kind, dtype)[0], "base"


def wrapped(bsm, H, leg):
    return bsm.adjoint(H) if leg == "adjoint" else H


def wrapped_adjoint(bsm, H, leg):
    """op(A)^H of the leg's op(A), as a wrapper of the handle"""
    return H if leg == "adjoint" else bsm.adjoint(H)


def device_columns(torch, operand, dtype, leg, cols=NB):
    B = leg_system(operand, dtype, leg)[1]
    return dev_copy(torch, np.asfortranarray(B[:, :cols]))


def solve(S, Bd, dtype, **kw):
    r = lsqr_rtol(dtype)
    return S.solve(Bd, rtol=r, ntol=r, maxiter=400, **kw)


def accept(got, operand, dtype, leg, what):
    """_lsqr.check_columns on the columns of a solve (X, info) of the leg (operand, dtype, leg) against the twin's runs on them"""
    X, info = got
    A, B, rule = leg_system(operand, dtype, leg)
    r = lsqr_rtol(dtype)
    xh = X.cpu().numpy().reshape(A.shape[1], -1)
    k = xh.shape[1]
    runs = leg_runs(operand, dtype, leg)[:k]
    worst = max(true_criteria(A, xh[:, c], B[:, c], r * float(np.linalg.norm(B[:, c].astype(np.complex128))), r, float(info.anorm[c]))[rule - 1]
                for c in range(k))
    print(f"LSHSTAT {what}: worst rule {rule} criterion / threshold {worst:.3f}, iterations {[int(v) for v in info.column_iterations]}, "
          f"twin {[t.iterations for t in runs]}")
    check_columns(info, runs, A, xh, B[:, :k], r, r, what, rule)
    return xh


def check_pass_count(torch, bsm, H, leg, S, Bd, first, per, what):
    """module docstring, "Pass counts"; first: (X, info) of the free-running solve of S on Bd"""
    X1, info1 = first
    pf, pa = passes_of_one_product(torch, bsm, H, wrapped(bsm, H, leg), X1), passes_of_one_product(torch, bsm, H, wrapped_adjoint(bsm, H, leg), Bd)
    k = int(info1.iterations)
    before = H.value_passes()
    _, info = S.solve(Bd, rtol=0.0, ntol=0.0, maxiter=k)
    delta = H.value_passes() - before
    print(f"LSHSTAT passes {what}: pf {pf}, pa {pa}; {info.iterations} iterations, a_products {info.a_products}, passes over the values {delta}")
    assert (pf, pa) == per, what
    assert info.iterations == k and info.column_status.tolist() == [1] * Bd.shape[1]
    check_products(info)
    assert delta == pf * k + pa * (k + 1), (what, delta, pf, pa, k)


def build(bsm, kind, dtype, torch=None, copy=False, **kw):
    """-> (handle, operand name); torch: from device-resident blocks; copy: from copies of the problem's blocks (update_blocks
    writes into the blocks a handle was built from, and the problems are shared between the tests)"""
    p, operand = problem_of(kind, dtype)
    p = on_device(torch, p) if torch is not None else (copied(p) if copy else p)
    return bsm.synthetic.build(p, **kw), operand


def legs_of(kinds, dtypes, symmetric=()):
    return [(k, dt, leg) for k in kinds for dt in dtypes for leg in LEGS] + [("symmetric", dt, leg) for dt in symmetric for leg in LEGS]


def leg_id(c):
    return "-".join(name(v) if isinstance(v, type) else str(v) for v in c)


# ---- A1. accumulate="gather" ---------------------------------------------------------------------------------------------
A1 = legs_of(KINDS, DTYPES, symmetric=(np.float64, np.float32))


@pytest.mark.parametrize("case", A1, ids=leg_id)
def test_gather_handles_five_columns(torch_cuda, bsm, case):
    torch, (kind, dtype, leg) = torch_cuda, case
    H, operand = build(bsm, kind, dtype, accumulate="gather")
    assert H.stats()["exclusive"] == 0
    S = bsm.Lsqr(wrapped(bsm, H, leg), nrhs=NB)
    accept(solve(S, device_columns(torch, operand, dtype, leg), dtype), operand, dtype, leg, f"A1 gather x5 {leg_id(case)}")


@pytest.mark.parametrize("case", A1, ids=leg_id)
def test_gather_handles_one_column_reproduces_its_bytes(torch_cuda, bsm, case):
    """one column: the forward product sums the gather workspace in a fixed order, the transposed one through the handle's op-T
    inverted index; both are bitwise reproducible (include/bsm_rocm.h), and with them the solve"""
    torch, (kind, dtype, leg) = torch_cuda, case
    H, operand = build(bsm, kind, dtype, accumulate="gather")
    assert H.stats()["exclusive"] == 0
    Bd = device_columns(torch, operand, dtype, leg, 1)
    Hop, HopH = wrapped(bsm, H, leg), wrapped_adjoint(bsm, H, leg)
    same_products(torch, bsm, Bd, HopH)
    S = bsm.Lsqr(Hop, nrhs=1)
    one = solve(S, Bd, dtype)
    same_products(torch, bsm, one[0], Hop)
    two, other = solve(S, Bd, dtype), solve(bsm.Lsqr(Hop, nrhs=1), Bd, dtype)
    same_bytes(one, two, "two solves on one solver")
    same_bytes(one, other, "a second solver object")
    accept(one, operand, dtype, leg, f"A1 gather x1 {leg_id(case)}")


# ---- A2. accumulate="colored" --------------------------------------------------------------------------------------------
A2 = legs_of(KINDS, WIDE, symmetric=(np.float64,))


@pytest.mark.parametrize("case", A2, ids=leg_id)
def test_colored_handles(torch_cuda, bsm, case):
    torch, (kind, dtype, leg) = torch_cuda, case
    H, operand = build(bsm, kind, dtype, accumulate="colored")
    Bd = device_columns(torch, operand, dtype, leg)
    S = bsm.Lsqr(wrapped(bsm, H, leg), nrhs=NB)
    one, two = solve(S, Bd, dtype), solve(S, Bd, dtype)
    what = f"A2 colored {leg_id(case)}"
    accept(one, operand, dtype, leg, what)
    same_bytes(one, two, "two solves on one solver")
    check_pass_count(torch, bsm, H, leg, S, Bd, one, (1, 1), what)


A2_CVEC = [(k, leg) for k in KINDS for leg in LEGS]


@pytest.mark.parametrize("kind, leg", A2_CVEC, ids=[f"{k}-{leg}" for k, leg in A2_CVEC])
def test_colored_real_handles_under_complex_columns_run_them_one_at_a_time(torch_cuda, bsm, kind, leg):
    torch, dtype = torch_cuda, np.complex128
    H, _ = build(bsm, kind, np.float64, accumulate="colored")
    Bd = device_columns(torch, "cvec", dtype, leg)
    S = bsm.Lsqr(wrapped(bsm, H, leg), nrhs=NB, dtype=dtype)
    one, two = solve(S, Bd, dtype), solve(S, Bd, dtype)
    what = f"A2 colored cvec {kind} {leg}"
    accept(one, "cvec", dtype, leg, what)
    same_bytes(one, two, "two solves on one solver")
    check_pass_count(torch, bsm, H, leg, S, Bd, one, (NB, NB), what)


# ---- A3. transpose_image=True ----------------------------------------------------------------------------------------------
A3 = legs_of(KINDS, WIDE)


@pytest.mark.parametrize("case", A3, ids=leg_id)
def test_second_image_handles(torch_cuda, bsm, case):
    """op N runs on the first image, op C forward on the second: every iteration reads both.  No byte claim for blocksparse:
    its rows are shared, and nothing promises exclusive stores on both of its images"""
    torch, (kind, dtype, leg) = torch_cuda, case
    H, operand = build(bsm, kind, dtype, transpose_image=True)
    Bd = device_columns(torch, operand, dtype, leg)
    S = bsm.Lsqr(wrapped(bsm, H, leg), nrhs=NB)
    one = solve(S, Bd, dtype)
    what = f"A3 second image {leg_id(case)}"
    accept(one, operand, dtype, leg, what)
    if kind == "vbcrs":
        same_bytes(one, solve(S, Bd, dtype), "two solves on one solver")
    check_pass_count(torch, bsm, H, leg, S, Bd, one, (1, 1), what)


# ---- A4. device-resident blocks, a side stream ---------------------------------------------------------------------------
A4 = [("vbcrs", np.float32, "inconsistent"), ("blocksparse", np.float64, "adjoint"), ("vbcrs", np.complex64, "adjoint"),
      ("blocksparse", np.complex128, "inconsistent"), ("symmetric", np.float64, "adjoint"), ("symmetric", np.float32, "inconsistent")]


@pytest.mark.parametrize("case", A4, ids=leg_id)
def test_device_resident_blocks_on_a_side_stream(torch_cuda, bsm, case):
    torch, (kind, dtype, leg) = torch_cuda, case
    H, operand = build(bsm, kind, dtype, torch=torch)
    Bd = device_columns(torch, operand, dtype, leg)
    torch.cuda.synchronize()
    got = solve(bsm.Lsqr(wrapped(bsm, H, leg), nrhs=NB), Bd, dtype, stream=torch.cuda.Stream())
    accept(got, operand, dtype, leg, f"A4 device blocks {leg_id(case)}")


# ---- A5. mixed cases ---------------------------------------------------------------------------------------------------------
A5 = legs_of(KINDS, WIDE)


@pytest.mark.parametrize("case", A5, ids=leg_id)
def test_single_precision_storage_under_double_vectors(torch_cuda, bsm, case):
    """the operator IS the rounded one: the twin runs on the values rounded to single.  The adjoint leg is op C of a float32 /
    complex64 image under double vectors"""
    torch, (kind, dtype, leg) = torch_cuda, case
    H, _ = build(bsm, kind, dtype, storage=single_of(dtype))
    assert H.dtype == np.dtype(dtype) and H.storage_dtype == single_of(dtype)
    Bd = device_columns(torch, "rounded", dtype, leg)
    S = bsm.Lsqr(wrapped(bsm, H, leg), nrhs=NB)
    one = solve(S, Bd, dtype)
    assert one[0].dtype == Bd.dtype and one[0].cpu().numpy().dtype == np.dtype(dtype)
    what = f"A5 storage {name(single_of(dtype))} {leg_id(case)}"
    accept(one, "rounded", dtype, leg, what)
    check_pass_count(torch, bsm, H, leg, S, Bd, one, (1, 1), what)


A5_CVEC = [("vbcrs", np.complex64), ("blocksparse", np.complex128)]


@pytest.mark.parametrize("kind, dtype", A5_CVEC, ids=[f"{k}-{name(dt)}" for k, dt in A5_CVEC])
def test_real_device_blocks_under_complex_columns(torch_cuda, bsm, kind, dtype):
    """the adjoint of a real handle under complex columns: op C of the real image through bsm_mul_multi_cvec, one pass"""
    torch, leg = torch_cuda, "adjoint"
    H, _ = build(bsm, kind, real_of(dtype), torch=torch)
    Bd = device_columns(torch, "cvec", dtype, leg)
    S = bsm.Lsqr(wrapped(bsm, H, leg), nrhs=NB, dtype=dtype)
    one = solve(S, Bd, dtype)
    assert one[0].dtype == Bd.dtype
    what = f"A5 device blocks, complex columns, {kind} {name(dtype)}"
    accept(one, "cvec", dtype, leg, what)
    check_pass_count(torch, bsm, H, leg, S, Bd, one, (1, 1), what)


# ---- A6. the bordered problem ------------------------------------------------------------------------------------------------
A6_MODES = {"default": {}, "gather": dict(accumulate="gather"), "colored": dict(accumulate="colored"), "transpose_image": dict(transpose_image=True)}
A6 = [(m, dt, leg) for m in A6_MODES for dt in (np.float64, np.complex64) for leg in LEGS]


def uncovered(xh, leg):
    """the entries of X that belong to columns of op(A) no block reaches"""
    return xh[M600:] if leg == "adjoint" else xh[N400:]


@pytest.mark.parametrize("case", A6, ids=leg_id)
def test_rows_and_columns_no_block_covers(torch_cuda, bsm, case):
    """the transposed product defines those entries of its result as zeros (the strong zero), or nobody does: V, W and X then
    carry whatever the workspace held.  Reproducible configurations: gather with one column, coloured with five (the
    bordered kind is blocksparse: no byte claim on its transpose_image handle)"""
    torch, (mode, dtype, leg) = torch_cuda, case
    H, operand = build(bsm, "bordered", dtype, **A6_MODES[mode])
    assert H.size == (M600 + BORDER, N400 + BORDER)
    Hop = wrapped(bsm, H, leg)
    what = f"A6 bordered {leg_id(case)}"
    Bd = device_columns(torch, operand, dtype, leg)
    got = solve(bsm.Lsqr(Hop, nrhs=NB), Bd, dtype)
    xh = accept(got, operand, dtype, leg, what)
    assert len(uncovered(xh, leg)) == BORDER and not uncovered(xh, leg).any(), "X is not zero where no block reaches"
    cols = {"gather": 1, "colored": NB}.get(mode)
    if cols is None:
        return
    Bd = device_columns(torch, operand, dtype, leg, cols)
    rng = np.random.default_rng(4701)
    other = dev_copy(torch, np.asfortranarray(uniform(rng, (bsm.size(Hop)[0], cols), dtype)))
    X0 = dev_copy(torch, np.asfortranarray(uniform(rng, (bsm.size(Hop)[1], cols), dtype)))
    used = bsm.Lsqr(Hop, nrhs=cols)
    Xo, io = used.solve(other, X0=X0, rtol=0.0, ntol=0.0, maxiter=7)
    assert io.iterations == 7 and uncovered(Xo.cpu().numpy(), leg).all(), "the guess leaves the entries no block reaches as they are"
    after, fresh = solve(used, Bd, dtype), solve(bsm.Lsqr(Hop, nrhs=cols), Bd, dtype)
    assert not uncovered(after[0].cpu().numpy(), leg).any()
    same_bytes(after, fresh, "a solver that has solved something else against a fresh one")
    accept(after, operand, dtype, leg, what + f" x{cols} after another solve")


# ---- B. one solver object across new values --------------------------------------------------------------------------------
def update_and_solve_again(torch, bsm, kind, dtype, leg, what, device=False, stream=None, cols=NB, **kw):
    """build from the old values, solve, update_blocks with the new ones, the SAME solver again -> ((X, info) after the update,
    handle, Bd).  Acceptance on the old operator, then on the new one"""
    H, operand = build(bsm, kind, dtype, torch=torch if device else None, copy=True, **kw)
    S = bsm.Lsqr(wrapped(bsm, H, leg), nrhs=cols)
    Bd = device_columns(torch, operand, dtype, leg, cols)
    torch.cuda.synchronize()
    accept(solve(S, Bd, dtype, stream=stream), operand, dtype, leg, what + " before")
    ids, new, _, operand2 = new_values(kind, dtype)
    if device:
        new = [dev_copy(torch, b) for b in new]
    bsm.update_blocks(H, new, ids=ids, stream=stream)
    after = solve(S, Bd, dtype, stream=stream)
    accept(after, operand2, dtype, leg, what + " after")
    return after, H, Bd


B1 = legs_of(KINDS, DTYPES)


@pytest.mark.parametrize("case", B1, ids=leg_id)
def test_update_and_the_same_solver_again(torch_cuda, bsm, case):
    kind, dtype, leg = case
    update_and_solve_again(torch_cuda, bsm, kind, dtype, leg, f"B1 {leg_id(case)}")


B2 = legs_of(KINDS, WIDE)


@pytest.mark.parametrize("case", B2, ids=leg_id)
def test_update_reaches_both_images(torch_cuda, bsm, case):
    """every iteration reads both images: a refill that missed one of them leaves an operator whose forward and adjoint
    products disagree, on which LSQR does not converge (test_lsqr_handles_cpu.py: test_a_half_refill_is_visible)"""
    kind, dtype, leg = case
    update_and_solve_again(torch_cuda, bsm, kind, dtype, leg, f"B2 {leg_id(case)}", transpose_image=True)


B3 = [("vbcrs", np.float64, "adjoint"), ("blocksparse", np.complex128, "inconsistent"), ("vbcrs", np.complex64, "inconsistent"),
      ("blocksparse", np.float32, "adjoint")]


@pytest.mark.parametrize("case", B3, ids=leg_id)
def test_update_of_device_resident_blocks_on_a_side_stream(torch_cuda, bsm, case):
    """update_blocks(A, device tensors, ids, stream=side), S.solve(..., stream=side): nothing waits in between but the stream's
    own order"""
    kind, dtype, leg = case
    update_and_solve_again(torch_cuda, bsm, kind, dtype, leg, f"B3 {leg_id(case)}", device=True, stream=torch_cuda.cuda.Stream())


B4 = [c + (m,) for c in legs_of(KINDS, WIDE) for m in ("gather-x1", "colored-x5")]


@pytest.mark.parametrize("case", B4, ids=leg_id)
def test_updated_objects_give_the_bytes_of_fresh_ones(torch_cuda, bsm, case):
    torch, (kind, dtype, leg, mode) = torch_cuda, case
    kw = dict(accumulate=mode.split("-")[0])
    cols = 1 if mode == "gather-x1" else NB
    after, H, Bd = update_and_solve_again(torch, bsm, kind, dtype, leg, f"B4 {leg_id(case)}", cols=cols, **kw)
    if cols == 1:
        same_products(torch, bsm, Bd, wrapped_adjoint(bsm, H, leg))
        same_products(torch, bsm, after[0], wrapped(bsm, H, leg))
    H2 = bsm.synthetic.build(new_values(kind, dtype)[2], **kw)
    fresh = solve(bsm.Lsqr(wrapped(bsm, H2, leg), nrhs=cols), Bd, dtype)
    same_bytes(after, fresh, "updated objects against fresh ones")


@pytest.mark.parametrize("kind", KINDS)
def test_a_solver_of_A_and_one_of_its_adjoint_on_one_handle(torch_cuda, bsm, kind):
    """Lsqr(A, nrhs=5) and Lsqr(adjoint(A), nrhs=5) on one handle, alternately, three times each: each keeps passing its
    acceptance; with one column each on a gather handle, each reproduces its own bytes"""
    torch, dtype = torch_cuda, np.float64
    H, operand = build(bsm, kind, dtype)
    solvers = {leg: bsm.Lsqr(wrapped(bsm, H, leg), nrhs=NB) for leg in LEGS}
    Bs = {leg: device_columns(torch, operand, dtype, leg) for leg in LEGS}
    for turn in range(3):
        for leg in LEGS:
            accept(solve(solvers[leg], Bs[leg], dtype), operand, dtype, leg, f"B5 {kind} {leg} turn {turn}")
    H, operand = build(bsm, kind, dtype, accumulate="gather")
    solvers = {leg: bsm.Lsqr(wrapped(bsm, H, leg), nrhs=1) for leg in LEGS}
    Bs = {leg: device_columns(torch, operand, dtype, leg, 1) for leg in LEGS}
    firsts = {}
    for turn in range(3):
        for leg in LEGS:
            got = solve(solvers[leg], Bs[leg], dtype)
            if leg not in firsts:
                firsts[leg] = got
                accept(got, operand, dtype, leg, f"B5 {kind} {leg} x1 gather")
            same_bytes(firsts[leg], got, f"{leg}, turn {turn}")


# ---- C. the own-range slice ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_a_handle_that_owns_a_row_range_is_refused(torch_cuda, bsm, kind):
    """both products of such a handle define (or, transposed, read) the owned rows only; the workspace vectors would keep what
    the previous iteration left outside them"""
    from bsm_amd import _lib as L
    dtype = np.float64
    p = lsqr_problem(kind, dtype)[0]
    code = CODE[np.dtype(dtype)]
    for own in ((1, 300), (101, M600)):
        part = bsm.synthetic.build(p, own=own)
        for op, wrap in ((0, lambda a: a), (2, bsm.adjoint)):
            rc, out = raw_lsqr_create(part, op, code, 4)
            assert rc == ERR_UNSUPPORTED and not out.value, (own, op, rc)
            assert "own a row range" in L.lib().bsm_last_error().decode()
            with pytest.raises(bsm._lib.BsmError, match="own a row range"):
                bsm.Lsqr(wrap(part), nrhs=4)
    whole = bsm.synthetic.build(p, own=(1, M600))
    for op in (0, 2):
        rc, ptr = raw_lsqr_create(whole, op, code, 4)
        assert rc == 0 and ptr.value and raw_lsqr_destroy(ptr) == 0


C_WHOLE = [("vbcrs", np.float64, "inconsistent"), ("vbcrs", np.complex64, "adjoint"), ("blocksparse", np.float64, "adjoint"),
           ("blocksparse", np.complex64, "inconsistent")]


@pytest.mark.parametrize("case", C_WHOLE, ids=leg_id)
def test_the_whole_own_range_is_accepted(torch_cuda, bsm, case):
    torch, (kind, dtype, leg) = torch_cuda, case
    H, operand = build(bsm, kind, dtype, own=(1, M600))
    got = solve(bsm.Lsqr(wrapped(bsm, H, leg), nrhs=NB), device_columns(torch, operand, dtype, leg), dtype)
    accept(got, operand, dtype, leg, f"C own=(1, 600) {leg_id(case)}")
