"""CPU companion of test_gpu_solver_handles.py: what that suite takes for granted, shown without a GPU.

  1. The solver table of _lockstep.py describes the problems it names: the dense operator is the sum of the blocks, the row
     scaling replayed from the generators IS the problems' W, the twins converge on every column.
  2. The update legs can see stale values.  D2 = D1 + W diag(SHIFT * J) W (_lockstep.shifted).  For every (solver, kind,
     type) of the table: the twin's solution on D2 misses D1 by more than 100 tolerances on every column and the other way
     round (a solve on stale A fails the acceptance); with the OLD block inverse on D2 the twin leaves the count its
     acceptance allows by at least two more (+-1 solvers: 3 or more off on some column), or does not converge at all
     (GMRES(20) stagnates) -- a stale M fails the acceptance.  SHIFT = 128: at the 8 a first draft used, cg, cocg and
     bicgstab do not show a stale M (figures at _lockstep.SHIFT).
  3. Every (problem, handle mode) the GPU suite builds exists: analysis-only builds (device=NODEV) of A and of
     block_jacobi in accumulate="gather" / "colored", transpose_image=True, storage=float32 and own=(101, 300) / (1, n),
     and the partial-ids update of an analysis-only A, read back entry by entry against D2 on both images.
"""
import numpy as np
import pytest

from _cg import column_tol, is_complex
from _common import NODEV
from _krylov import exact_minv, true_residual
from _lockstep import SHIFT, SINGLE_TYPES, WIDE_TYPES, case_id, shifted, solver_cases, solvers
from _submat import Truth

CASES = solver_cases()
ALL_TYPES = solver_cases(WIDE_TYPES + SINGLE_TYPES)


def test_the_table_names_what_the_issue_lists():
    rows = solvers()
    assert list(rows) == ["cg", "cocg", "bicgstab", "minres", "gmres_multi", "gmres"]
    assert [r.cls for r in rows.values()] == ["Cg", "Cg", "BiCgStab", "Minres", "GmresMulti", "Gmres"]
    # the two combinations that do not exist by construction
    assert ("minres", "symmetric", np.complex128) not in CASES and ("cg", "symmetric", np.complex128) not in CASES
    assert not any(name == "bicgstab" and kind == "symmetric" for name, kind, _ in CASES)
    assert len(CASES) == 29


@pytest.mark.parametrize("case", ALL_TYPES, ids=case_id)
def test_problems_of_the_table(case):
    name, kind, dtype = case
    R = solvers()[name]
    c = R.case(kind, dtype)
    n = c.D.shape[0]
    assert c.D.dtype == np.dtype(dtype) and c.B.dtype == np.dtype(dtype) and c.B.shape == (n, R.nrhs)
    assert np.array_equal(Truth(c.p).D, c.D) and np.array_equal(Truth(c.pm).D, c.P)
    if name in ("gmres", "gmres_multi"):
        assert np.all(c.w == 1) and np.all(c.sign == 1)
        return
    # W: D / (w w^T) is S + s J with |S| < 1 and s = 24 / 36
    s = 36.0 if is_complex(dtype) else 24.0
    core = c.D.astype(np.complex128) / (c.w[:, None] * c.w[None, :]) - s * np.diag(c.sign)
    assert np.max(np.abs(core.real)) < 1 and np.max(np.abs(core.imag)) < 1
    assert set(np.unique(c.w)) <= {2.0 ** k for k in range(-3, 4)} and len(np.unique(c.w)) > 1
    assert (name == "minres") == bool(np.any(c.sign < 0))


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_stale_values_are_visible(case):
    name, kind, dtype = case
    R = solvers()[name]
    c = R.case(kind, dtype)
    sh = shifted(c)
    ids, new, D2, P2 = sh.ids, sh.new, sh.D2, sh.P2
    assert (sh.pm2 is sh.p2) == (c.pm is c.p)
    diff = D2 - c.D
    assert np.array_equal(diff, np.diag(np.diag(diff))) and np.all(np.diag(diff).real * c.sign > 0)
    # exactly the blocks that hold a diagonal entry, and not all of them
    nblocks = len(c.p.get("blocks", ())) if c.p["kind"] != "symmetric" else len(c.p["diagonals"]) + len(c.p["offdiagonals"])
    assert 0 < len(ids) < nblocks and len(ids) == len(set(ids)) == len(new)
    rtol, k = R.rtol(dtype), c.B.shape[1]
    tols = [column_tol(c.B[:, j], rtol) for j in range(k)]
    M1, M2 = exact_minv(c.P, c.sets), exact_minv(P2, c.sets)
    r1, r2, stale = R.runs(c.D, c.B, M1, dtype), R.runs(D2, c.B, M2, dtype), R.runs(D2, c.B, M1, dtype)
    assert all(r.status == 0 for r in r1 + r2)
    old_on_new = min(true_residual(D2, r1[j].x, c.B[:, j]) / tols[j] for j in range(k))
    new_on_old = min(true_residual(c.D, r2[j].x, c.B[:, j]) / tols[j] for j in range(k))
    print(f"HANDSTAT stale {case_id(case)}: shift {SHIFT}, {len(ids)} of {nblocks} blocks; residual / tol of the old solution on D2 "
          f"{old_on_new:.2e}, of the new one on D1 {new_on_old:.2e}; counts fresh {[r.iterations for r in r2]}, old M "
          f"{[r.iterations for r in stale]} (status {[r.status for r in stale]})")
    assert old_on_new > 100 and new_on_old > 100
    # a stale M: right solution (where it converges), wrong count
    seen = False
    for j, (s, r) in enumerate(zip(stale, r2)):
        below, above = R.slack(r.iterations)
        seen |= s.status != 0 or s.iterations >= r.iterations + above + 2 or s.iterations <= r.iterations - below - 2
        if s.status == 0:
            assert true_residual(D2, s.x, c.B[:, j]) <= 2 * tols[j]
    assert seen, "a stale preconditioner would pass the acceptance"


# ---- analysis-only builds of every mode the GPU suite uses -------------------------------------------------------------
MODES = ["gather", "colored", "transpose_image", "storage", "own-slice", "own-all"]


def mode_applies(mode, kind, dtype):
    if mode in ("gather", "colored"):
        return kind in ("blocksparse", "symmetric") and (mode == "gather" or dtype in WIDE_TYPES)
    if mode == "transpose_image":
        return kind in ("vbcrs", "blocksparse") and dtype in WIDE_TYPES
    return dtype in WIDE_TYPES


BUILDS = [c + (m,) for c in ALL_TYPES for m in MODES if mode_applies(m, c[1], c[2])]


@pytest.mark.parametrize("case", BUILDS, ids=case_id)
def test_every_mode_builds_analysis_only(bsm, case):
    name, kind, dtype, mode = case
    R = solvers()[name]
    c = R.case(kind, dtype)
    n = c.D.shape[0]
    akw, mkw = dict(device=NODEV), {}
    if mode in ("gather", "colored"):
        akw["accumulate"] = mkw["accumulate"] = mode
    elif mode == "transpose_image":
        akw["transpose_image"] = mkw["transpose_image"] = True
    elif mode == "storage":
        akw["storage"] = np.float32 if not is_complex(dtype) else np.complex64
        mkw["accumulate"] = "colored"
    elif mode.startswith("own"):
        akw["own"] = (101, 300) if mode == "own-slice" else (1, n)
    A = bsm.synthetic.build(c.p, **akw)
    Am = A if c.pm is c.p else bsm.synthetic.build(c.pm, **akw)
    src = bsm.transpose(Am) if mode == "transpose_image" else Am
    M = bsm.block_jacobi(src, c.sets, **mkw)
    assert A.size == (n, n) and M.size == (n, n) and A.device is None and M.device is None
    if mode == "gather":
        assert A.stats()["exclusive"] == 0, "every row of this kind belongs to one block: the default mode would not use atomics"
    # the preconditioner of an analysis-only handle is the block inverse (of the rounded values under storage=).  A sanity
    # bound, not an accuracy test (test_invert_blocks_cpu.py has that): the blocks' condition numbers are below 10, a
    # backward stable inverse of order <= 129 is then within 10 n eps of the exact one, relative to its largest entry
    P = Truth(c.pm, akw.get("storage")).D
    Pt = P.T if mode == "transpose_image" else P
    rows = np.arange(n)
    got = M[rows, rows]
    want = exact_minv(Pt.astype(c.P.dtype), c.sets)
    assert np.max(np.abs(got - want)) <= 64 * n * np.finfo(dtype).eps * np.max(np.abs(want))


UPDATES = [c + (t,) for c in CASES for t in ("one-image", "two-images") if t == "one-image" or c[1] != "symmetric"]


@pytest.mark.parametrize("case", UPDATES, ids=case_id)
def test_partial_update_of_an_analysis_only_handle(bsm, case):
    """update_blocks(A, blocks that hold a diagonal entry, ids=...) as the GPU legs call it, on the host image: op(A)[I, J]
    read back is D2 for op = N and T (the second image of a transpose_image handle answers T)"""
    name, kind, dtype, images = case
    timage = images == "two-images"
    R = solvers()[name]
    c = R.case(kind, dtype)
    sh = shifted(c)
    ids, new, D2 = sh.ids, sh.new, sh.D2
    A = bsm.synthetic.build(c.p, device=NODEV, **(dict(transpose_image=True) if timage else {}))
    bsm.update_blocks(A, new, ids=ids)
    rows = np.arange(c.D.shape[0])
    tol = 4 * np.finfo(dtype).eps * np.max(np.abs(D2))
    assert np.max(np.abs(A[rows, rows] - D2)) <= tol
    assert np.max(np.abs(bsm.transpose(A)[rows, rows] - D2.T)) <= tol
