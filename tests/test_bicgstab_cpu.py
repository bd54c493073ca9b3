"""CPU suite of the BiCGSTAB layer: the numpy twin that the GPU suite measures bsm_bicgstab_solve against must itself
solve the test problems with the counts the GPU tests expect, keep them under permuted sums and reach its four statuses
(so that no GPU test rests on an oracle that fails alone); the ctypes prototypes must be there with the struct layout the
header asserts; and bsm_bicgstab_create must answer without a device what it can."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from _bicgstab import (EDGE_N, ERR_DEVICE, ERR_INVALID, MAX_RHS, NB, NBI, SIGMA_ZERO, TS_ZERO, bicgstab_problem, bicgstab_twin,
                       breakdown_problem, column_tol, edge_case, exact_minv, raw_bicgstab_create, raw_bicgstab_destroy,
                       raw_bicgstab_solve, rtol_of, staggered, third_iterate_spread, true_residual)
from _jacobi import CODE, DTYPES

NODEV = -2  # BSM_DEVICE_NONE
IDS = [np.dtype(d).name for d in DTYPES]
HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bsm_rocm.h")
# iterations of the five columns of the main problem with block-Jacobi at rtol 1e-4 (single) / 1e-10 (double)
COUNTS = {"float32": [8, 9, 9, 9, 9], "float64": [17, 17, 17, 17, 18], "complex64": [7, 7, 7, 7, 7], "complex128": [15, 15, 15, 15, 15]}
STAGGERED = {"float32": [8, 7, 6, 4, 0], "float64": [17, 14, 9, 4, 0]}
# (min, max) iterations over the 16 columns of the layout-edge operators, per n of EDGE_N
EDGE_COUNTS = {
    "float32": [(1, 1), (2, 2), (3, 5), (3, 4), (4, 4), (3, 5), (3, 5), (3, 4), (3, 4)],
    "float64": [(1, 1), (2, 2), (8, 9), (7, 8), (8, 9), (8, 9), (8, 10), (8, 9), (8, 10)],
    "complex64": [(1, 1), (2, 2), (4, 5), (4, 5), (4, 5), (4, 5), (5, 5), (4, 5), (4, 5)],
    "complex128": [(1, 1), (2, 2), (10, 11), (10, 10), (10, 11), (10, 11), (11, 12), (11, 11), (11, 12)],
}


@pytest.fixture(scope="module")
def problems():
    """dtype name -> (D, B, Minv); the dense operator does not depend on the kind it is cut into"""
    out = {}
    for dt in DTYPES:
        _, sets, D, B = bicgstab_problem("vbcrs", dt)
        out[np.dtype(dt).name] = (D, B, exact_minv(D, sets))
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_twin_solves_the_main_problem(problems, dtype):
    name = np.dtype(dtype).name
    D, B, Minv = problems[name]
    rtol = rtol_of(dtype)
    assert not np.array_equal(D, D.T) and not np.array_equal(D, D.conj().T), "the operator is meant to be nonsymmetric"
    runs = [bicgstab_twin(D, B[:, c], Minv, rtol, 0.0, 100, dtype) for c in range(NB)]
    ratios = [true_residual(D, r.x, B[:, c]) / column_tol(B[:, c], rtol) for c, r in enumerate(runs)]
    counts = [r.iterations for r in runs]
    print(f"BICGSTAT twin {name}: cond {np.linalg.cond(D.astype(np.complex128)):.2e}, iterations {counts}, true residual / tol "
          f"{min(ratios):.2f} .. {max(ratios):.2f}")
    assert all(r.status == 0 for r in runs) and counts == COUNTS[name]
    assert max(ratios) <= 1
    for seed in range(4):
        order = np.random.default_rng(seed).permutation(NBI)
        assert [bicgstab_twin(D, B[:, c], Minv, rtol, 0.0, 100, dtype, order=order).iterations for c in range(NB)] == counts, seed


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_missing_preconditioner_is_visible(problems, dtype):
    D, B, _ = problems[np.dtype(dtype).name]
    run = bicgstab_twin(D, B[:, 0], None, rtol_of(dtype), 0.0, 60, dtype)
    rel = run.history[-1] / run.bnorm
    print(f"BICGSTAT twin without M, {np.dtype(dtype).name}: relative residual after 60 iterations {rel:.3g}")
    assert run.status == 1 and run.iterations == 60 and rel > 1e-3


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_twin_on_staggered_columns(problems, dtype):
    name = np.dtype(dtype).name
    D, B, Minv = problems[name]
    Bs, atol = staggered(B, dtype)
    counts = [bicgstab_twin(D, Bs[:, c], Minv, 0.0, atol, 100, dtype).iterations for c in range(NB)]
    assert counts == STAGGERED[name]
    order = np.random.default_rng(2).permutation(NBI)
    assert [bicgstab_twin(D, Bs[:, c], Minv, 0.0, atol, 100, dtype, order=order).iterations for c in range(NB)] == counts


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_twin_on_the_layout_edge_operators(dtype):
    """every n of the table, all 16 columns: status 0, true residual <= tol, the counts of EDGE_COUNTS -- one iteration at
    n = 1 (through the sn <= tol exit: the half step solves a 1 x 1 system), two at n = 2, 3 .. 5 (float32), 7 .. 10
    (float64), 4 .. 5 (complex64), 10 .. 12 (complex128) otherwise -- and the same counts under a permutation of every sum
    (dense operator, n <= 257)"""
    name, rtol, table, worst = np.dtype(dtype).name, rtol_of(dtype), [], 0.0
    for n in EDGE_N:
        _, Dop, B, runs = edge_case(n, dtype)
        Dw = Dop.astype(np.complex128)
        counts = [r.iterations for r in runs]
        table.append((min(counts), max(counts)))
        for c, r in enumerate(runs):
            assert r.status == 0, (n, c)
            true = float(np.linalg.norm(B[:, c].astype(np.complex128) - Dw @ r.x.astype(np.complex128)))
            worst = max(worst, true / column_tol(B[:, c], rtol))
        if n <= 257:
            D, order = Dop.dense(), np.random.default_rng(n).permutation(n)
            assert [bicgstab_twin(D, B[:, c], None, rtol, 0.0, 200, dtype, order=order).iterations for c in range(MAX_RHS)] == counts, n
    print(f"BICGSTAT twin layout edges {name}: (min, max) iterations per n {dict(zip(EDGE_N, table))}, largest true residual / tol "
          f"{worst:.3f}")
    assert table == EDGE_COUNTS[name]
    assert worst <= 1


def test_twin_statuses():
    D, b = np.array([[4.0, 1.0], [-1.0, 3.0]]), np.array([1.0, 2.0])
    run = bicgstab_twin(D, b, None, 1e-12, 0.0, 10, np.float64)
    assert run.status == 0 and run.iterations == 2 and np.allclose(D @ run.x, b)
    assert bicgstab_twin(D, b, None, 1e-12, 0.0, 1, np.float64).status == 1
    nan = bicgstab_twin(D, np.array([1.0, np.nan]), None, 1e-12, 0.0, 10, np.float64)
    assert nan.status == 2 and nan.iterations == 0
    zero = bicgstab_twin(D, np.zeros(2), None, 1e-12, 0.0, 10, np.float64)
    assert zero.status == 0 and zero.iterations == 0
    # n = 1: alpha = 1 / a solves the system in the half step; t = a s = 0 gives tt == 0, which the order of the checks
    # must not turn into a breakdown
    one = bicgstab_twin(np.array([[3.0]]), np.array([2.0]), None, 1e-12, 0.0, 10, np.float64)
    assert one.status == 0 and one.iterations == 1 and one.residual == 0 and one.x[0] == 2.0 / 3.0


@pytest.mark.parametrize("dtype", [np.float64, np.complex64], ids=["float64", "complex64"])
def test_twin_breakdowns(dtype):
    for block, its, x0 in ((SIGMA_ZERO, 0, 0.0), (TS_ZERO, 1, 1.0)):
        _, D, B = breakdown_problem(block, dtype)
        brk = bicgstab_twin(D, B[:, 0], None, 1e-6, 0.0, 50, dtype)
        assert (brk.status, brk.iterations, brk.residual) == (3, its, 1.0), block
        assert brk.x[0] == x0 and np.all(brk.x[1:] == 0) and np.all(np.isfinite(brk.x))
        good = bicgstab_twin(D, B[:, 1], None, 1e-6, 0.0, 50, dtype)
        assert good.status == 0 and 1 <= good.iterations <= 10 and true_residual(D, good.x, B[:, 1]) <= 2 * column_tol(B[:, 1], 1e-6)


def test_third_iterate_under_permuted_summation_orders():
    """the figure test_gpu_bicgstab.py takes its bound from (4 times this): how far the twin's third iterate moves when
    every form and product is summed in another order, on the well-conditioned layout-edge operator at n = 256.  (On the
    unpreconditioned main problem the same measurement gives tens to hundreds of eps: BiCGSTAB is far more sensitive
    there than CG, which is why this operator was picked.)"""
    run, worst = third_iterate_spread()
    print(f"BICGSTAT twin third iterate, eight permuted summation orders: {worst:.2f} eps max|x|")
    assert run.status == 1 and run.iterations == 3
    assert 0 < worst <= 64  # eps-sized: rounding, not another method


# ---- the C ABI without a device ----------------------------------------------------------------------------------------------
def test_prototypes_and_struct_layouts():
    from bsm_amd import _lib as L
    hdr = re.sub(r"\s+", " ", open(HDR).read())
    for text in ("sizeof(bsm_cg_params) == 40 && offsetof(bsm_cg_params, rtol) == 8 && offsetof(bsm_cg_params, maxiter) == 24",
                 "sizeof(bsm_cg_info) == 48 && offsetof(bsm_cg_info, iterations) == 8 && offsetof(bsm_cg_info, a_products) == 16 && "
                 "offsetof(bsm_cg_info, workspace) == 40",
                 "sizeof(bsm_cg_column) == 32 && offsetof(bsm_cg_column, iterations) == 8 && offsetof(bsm_cg_column, residual) == 16",
                 "int bsm_bicgstab_create(bsm_matrix_t A, int opA, bsm_matrix_t M, int opM, int vdtype, int32_t nrhs_max, "
                 "struct bsm_bicgstab_s **out);",
                 "const bsm_cg_params *p, bsm_cg_info *info, bsm_cg_column *cols"):
        assert text in hdr, text
    assert C.sizeof(L.BsmCgParams) == 40 and C.sizeof(L.BsmCgInfo) == 48 and C.sizeof(L.BsmCgColumn) == 32
    for name in ("bsm_bicgstab_create", "bsm_bicgstab_solve", "bsm_bicgstab_destroy"):
        assert name in L.EXPORTS and hasattr(L.lib(), name) and getattr(L.lib(), name).restype is C.c_int
    assert len(L.lib().bsm_bicgstab_create.argtypes) == 7 and L.lib().bsm_bicgstab_solve.argtypes == L.lib().bsm_cg_solve.argtypes


@pytest.fixture(scope="module")
def handles(bsm):
    """analysis-only handles: the float64 operator, its block-Jacobi preconditioner, an operator of another order, a
    non-square one, a complex one"""
    p, sets, _, _ = bicgstab_problem("blocksparse", np.float64)
    A = bsm.synthetic.build(p, device=NODEV)
    M = bsm.block_jacobi(A, sets)
    small = bsm.BlockSparseMatrix([np.eye(3)], [[1, 2, 3]], [[1, 2, 3]], (3, 3), device=NODEV)
    rect = bsm.BlockSparseMatrix([np.ones((2, 3))], [[1, 2]], [[1, 2, 3]], (4, 5), device=NODEV)
    pc, _, _, _ = bicgstab_problem("vbcrs", np.complex128)
    return A, M, small, rect, bsm.synthetic.build(pc, device=NODEV)


def test_create_refuses_analysis_only_handles(bsm, handles):
    A, M, *_ = handles
    for m in (None, M):
        rc, ptr = raw_bicgstab_create(A, 0, m, 0, CODE[np.dtype(np.float64)], 5)
        assert rc == ERR_DEVICE and not ptr.value
    with pytest.raises(bsm._lib.BsmError, match="no device image"):
        bsm.BiCgStab(A, M, nrhs=3)
    with pytest.raises(bsm._lib.BsmError, match="no device image"):
        bsm.bicgstab(A, np.zeros(NBI))


def test_create_argument_checks(bsm, handles):
    A, M, small, rect, Ac = handles
    f64, c128, f32, c64 = (CODE[np.dtype(t)] for t in (np.float64, np.complex128, np.float32, np.complex64))
    bad = [
        ("nrhs_max 0", (A, 0, M, 0, f64, 0)),
        ("nrhs_max 17", (A, 0, M, 0, f64, MAX_RHS + 1)),
        ("negative nrhs_max", (A, 0, None, 0, f64, -1)),
        ("non-square operator", (rect, 0, None, 0, f64, 1)),
        ("M of another order", (A, 0, small, 0, f64, 1)),
        ("bad opA", (A, 3, None, 0, f64, 1)),
        ("bad opM", (A, 0, M, -1, f64, 1)),
        ("mixed storage code as vdtype", (A, 0, None, 0, 4, 1)),
        ("bad vdtype", (A, 0, None, 0, 9, 1)),
        ("a float64 operator under float32 vectors", (A, 0, None, 0, f32, 1)),
        ("a float64 operator under complex64 vectors", (A, 0, None, 0, c64, 1)),
        ("a complex operator under real vectors", (Ac, 0, None, 0, f64, 1)),
        ("a complex preconditioner under real vectors", (A, 0, Ac, 0, f64, 1)),
        ("null operator", (None, 0, None, 0, f64, 1)),
    ]
    for what, args in bad:
        rc, ptr = raw_bicgstab_create(*args)
        assert rc == ERR_INVALID and not ptr.value, what
    from bsm_amd import _lib as L
    assert L.lib().bsm_bicgstab_create(A._h.ptr, 0, None, 0, f64, 1, None) == ERR_INVALID  # null out
    # what is acceptable up to the missing device answers BSM_ERR_DEVICE
    for what, args in [("real operator, complex vectors", (A, 0, M, 0, c128, MAX_RHS)), ("adjoint", (A, 2, M, 2, f64, 1)),
                       ("transpose of a complex operator", (Ac, 1, None, 0, c128, 8))]:
        rc, ptr = raw_bicgstab_create(*args)
        assert rc == ERR_DEVICE and not ptr.value, what
    assert raw_bicgstab_destroy(None) == 0
    assert raw_bicgstab_solve(None, 1, 0x1000, 4, 0x2000, 4)[0] == ERR_INVALID
    with pytest.raises(TypeError):
        bsm.BiCgStab(np.eye(3))
    with pytest.raises(TypeError):
        bsm.BiCgStab(A, M=np.eye(3))
    with pytest.raises(bsm._lib.BsmError, match="nrhs_max"):
        bsm.BiCgStab(A, nrhs=17)


def test_mixed_storage_handles_count_with_their_double_vectors(bsm):
    p, _, _, _ = bicgstab_problem("vbcrs", np.float64)
    A = bsm.synthetic.build(p, device=NODEV, storage=np.float32)
    assert raw_bicgstab_create(A, 0, None, 0, CODE[np.dtype(np.float64)], 5)[0] == ERR_DEVICE
    assert raw_bicgstab_create(A, 0, None, 0, CODE[np.dtype(np.float32)], 5)[0] == ERR_INVALID
    assert raw_bicgstab_create(A, 0, None, 0, CODE[np.dtype(np.complex128)], 5)[0] == ERR_INVALID
