"""CPU suite of the CG layer: the numpy twin that the GPU suite measures bsm_cg_solve against must itself solve the test
problems and reach its four statuses (so that no GPU test rests on an oracle that fails alone), the ctypes mirrors must
have the layout the header asserts, and bsm_cg_create must answer without a device what it can."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from _cg import (CG, COCG, ERR_DEVICE, ERR_INVALID, MAX_RHS, NB, cg_problem, cg_twin, column_tol, exact_minv, is_complex, raw_cg_create,
                 raw_cg_destroy, raw_cg_solve, rtol_of, spd_problem, true_residual)
from _jacobi import CODE, DTYPES

NODEV = -2  # BSM_DEVICE_NONE
IDS = [np.dtype(d).name for d in DTYPES]
HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bsm_rocm.h")
# (dtype, Hermitian variant): SPD CG for the real types, COCG for the complex symmetric ones, CG for the Hermitian ones
VARIANTS = [(np.float32, False), (np.float64, False), (np.complex64, False), (np.complex128, False), (np.complex64, True),
            (np.complex128, True)]
VIDS = ["float32", "float64", "complex64-cocg", "complex128-cocg", "complex64-herm", "complex128-herm"]


def conj_of(dtype, herm):
    return herm or not is_complex(dtype)


@pytest.fixture(scope="module")
def problems():
    """(dtype name, herm) -> (D, B, Minv); the dense operator does not depend on the kind it is cut into"""
    out = {}
    for dt, herm in VARIANTS:
        _, sets, D, B = cg_problem("vbcrs", dt, herm)
        out[np.dtype(dt).name, herm] = (D, B, exact_minv(D, sets))
    return out


@pytest.mark.parametrize("dtype, herm", VARIANTS, ids=VIDS)
def test_twin_solves_every_problem(problems, dtype, herm):
    D, B, Minv = problems[np.dtype(dtype).name, herm]
    rtol = rtol_of(dtype)
    assert np.array_equal(D, D.conj().T if herm else D.T), "the operator is not symmetric to the bit"
    cond = np.linalg.cond(D.astype(np.complex128))
    counts, ratios, shuffled = [], [], []
    order = np.random.default_rng(1).permutation(len(D))
    for c in range(NB):
        run = cg_twin(D, B[:, c], Minv, conj_of(dtype, herm), rtol, 0.0, 100, dtype)
        assert run.status == 0 and 1 <= run.iterations <= 60
        tol = column_tol(B[:, c], rtol)
        ratios.append(true_residual(D, run.x, B[:, c]) / tol)
        counts.append(run.iterations)
        shuffled.append(cg_twin(D, B[:, c], Minv, conj_of(dtype, herm), rtol, 0.0, 100, dtype, order=order).iterations)
    print(f"CGSTAT twin {VIDS[VARIANTS.index((dtype, herm))]}: cond {cond:.2e}, iterations {counts}, with permuted sums {shuffled}, "
          f"true residual / tol {min(ratios):.2f} .. {max(ratios):.2f}")
    assert max(ratios) <= 2
    assert all(abs(a - b) <= 1 for a, b in zip(counts, shuffled))


@pytest.mark.parametrize("dtype, herm", [(np.float64, False), (np.complex64, False)], ids=["float64", "complex64-cocg"])
def test_a_missing_preconditioner_is_visible(problems, dtype, herm):
    D, B, _ = problems[np.dtype(dtype).name, herm]
    run = cg_twin(D, B[:, 0], None, conj_of(dtype, herm), rtol_of(dtype), 0.0, 60, dtype)
    rel = run.history[-1] / run.bnorm
    print(f"CGSTAT twin without M, {np.dtype(dtype).name}: relative residual after 60 iterations {rel:.3g}")
    assert run.status == 1 and run.iterations == 60 and rel > 1e-3


def test_twin_statuses():
    D, B = np.array([[4.0, 1.0], [1.0, 3.0]]), np.array([1.0, 2.0])
    run = cg_twin(D, B, None, True, 1e-12, 0.0, 10, np.float64)
    assert run.status == 0 and run.iterations == 2
    assert cg_twin(D, B, None, True, 1e-12, 0.0, 1, np.float64).status == 1
    nan = cg_twin(D, np.array([1.0, np.nan]), None, True, 1e-12, 0.0, 10, np.float64)
    assert nan.status == 2 and nan.iterations == 0
    # <p, A p> = 0 in iteration 1: breakdown, no iteration completed, x untouched
    brk = cg_twin(np.array([[0.0, 1.0], [1.0, 0.0]]), np.array([1.0, 0.0]), None, True, 1e-12, 0.0, 10, np.float64)
    assert brk.status == 3 and brk.iterations == 0 and np.all(brk.x == 0)
    zero = cg_twin(D, np.zeros(2), None, True, 1e-12, 0.0, 10, np.float64)
    assert zero.status == 0 and zero.iterations == 0


def test_twin_on_two_summation_orders_at_maxiter_3(problems):
    """the case test_gpu_cg.py compares its third iterate against (float64, column 0, no preconditioner: a preconditioner
    inverted on the device is another matrix than the twin's in its last bits): 8 eps max|x| covers a change of the
    summation order of every product and form"""
    D, B, _ = problems["float64", False]
    a = cg_twin(D, B[:, 0], None, True, 0.0, 0.0, 3, np.float64)
    assert a.status == 1 and a.iterations == 3
    worst = 0.0
    for seed in range(4):
        b = cg_twin(D, B[:, 0], None, True, 0.0, 0.0, 3, np.float64, order=np.random.default_rng(seed).permutation(len(D)))
        worst = max(worst, np.max(np.abs(a.x - b.x)) / (np.finfo(np.float64).eps * np.max(np.abs(a.x))))
    print(f"CGSTAT twin third iterate, permuted summation orders: {worst:.2f} eps max|x|")
    assert worst <= 8


def test_block_diagonal_twin_operator():
    p, Dop = spd_problem(np.random.default_rng(5), 21, np.complex128)
    v = np.random.default_rng(6).uniform(-1, 1, 21) + 0j
    assert np.allclose(Dop @ v, Dop.dense() @ v) and len(p["blocks"]) == 3
    assert np.array_equal(Dop.dense(), Dop.dense().conj().T)


# ---- the C ABI without a device ----------------------------------------------------------------------------------------------
def test_struct_layouts_match_the_header():
    from bsm_amd import _lib as L
    hdr = re.sub(r"\s+", " ", open(HDR).read())
    for text in ("sizeof(bsm_cg_params) == 40 && offsetof(bsm_cg_params, rtol) == 8 && offsetof(bsm_cg_params, maxiter) == 24",
                 "sizeof(bsm_cg_info) == 48 && offsetof(bsm_cg_info, iterations) == 8 && offsetof(bsm_cg_info, a_products) == 16 && "
                 "offsetof(bsm_cg_info, workspace) == 40",
                 "sizeof(bsm_cg_column) == 32 && offsetof(bsm_cg_column, iterations) == 8 && offsetof(bsm_cg_column, residual) == 16",
                 "#define BSM_CG_MAX_RHS 16", "BSM_CG_METHOD_CG = 0, BSM_CG_METHOD_COCG = 1"):
        assert text in hdr, text
    assert C.sizeof(L.BsmCgParams) == 40 and L.BsmCgParams.rtol.offset == 8 and L.BsmCgParams.maxiter.offset == 24
    assert C.sizeof(L.BsmCgInfo) == 48 and L.BsmCgInfo.iterations.offset == 8 and L.BsmCgInfo.a_products.offset == 16
    assert L.BsmCgInfo.workspace.offset == 40
    assert C.sizeof(L.BsmCgColumn) == 32 and L.BsmCgColumn.iterations.offset == 8 and L.BsmCgColumn.residual.offset == 16
    assert (L.BSM_CG_MAX_RHS, L.BSM_CG_METHOD_CG, L.BSM_CG_METHOD_COCG) == (MAX_RHS, CG, COCG)
    for name in ("bsm_cg_create", "bsm_cg_solve", "bsm_cg_destroy"):
        assert name in L.EXPORTS and hasattr(L.lib(), name)


@pytest.fixture(scope="module")
def handles(bsm):
    """analysis-only handles: the float64 operator, its block-Jacobi preconditioner, an operator of another order, a
    non-square one, a complex one"""
    p, sets, _, _ = cg_problem("blocksparse", np.float64)
    A = bsm.synthetic.build(p, device=NODEV)
    M = bsm.block_jacobi(A, sets)
    small = bsm.BlockSparseMatrix([np.eye(3)], [[1, 2, 3]], [[1, 2, 3]], (3, 3), device=NODEV)
    rect = bsm.BlockSparseMatrix([np.ones((2, 3))], [[1, 2]], [[1, 2, 3]], (4, 5), device=NODEV)
    pc, _, _, _ = cg_problem("vbcrs", np.complex128)
    return A, M, small, rect, bsm.synthetic.build(pc, device=NODEV)


def test_create_refuses_analysis_only_handles(bsm, handles):
    A, M, *_ = handles
    for m in (None, M):
        for method in (CG, COCG):
            rc, ptr = raw_cg_create(A, 0, m, 0, CODE[np.dtype(np.float64)], 5, method)
            assert rc == ERR_DEVICE and not ptr.value
    with pytest.raises(bsm._lib.BsmError, match="no device image"):
        bsm.Cg(A, M, nrhs=3)


def test_create_argument_checks(bsm, handles):
    A, M, small, rect, Ac = handles
    f64, c128, f32, c64 = (CODE[np.dtype(t)] for t in (np.float64, np.complex128, np.float32, np.complex64))
    bad = [
        ("nrhs_max 0", (A, 0, M, 0, f64, 0)),
        ("nrhs_max 17", (A, 0, M, 0, f64, MAX_RHS + 1)),
        ("negative nrhs_max", (A, 0, None, 0, f64, -1)),
        ("bad method", (A, 0, None, 0, f64, 1, 2)),
        ("negative method", (A, 0, None, 0, f64, 1, -1)),
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
        rc, ptr = raw_cg_create(*args)
        assert rc == ERR_INVALID and not ptr.value, what
    # what is acceptable up to the missing device answers BSM_ERR_DEVICE
    for what, args in [("real operator, complex vectors", (A, 0, M, 0, c128, MAX_RHS)), ("adjoint, COCG", (A, 2, M, 2, f64, 1, COCG)),
                       ("a complex operator", (Ac, 1, None, 0, c128, 8, COCG))]:
        rc, ptr = raw_cg_create(*args)
        assert rc == ERR_DEVICE and not ptr.value, what
    assert raw_cg_destroy(None) == 0
    assert raw_cg_solve(None, 1, 0x1000, 4, 0x2000, 4)[0] == ERR_INVALID
    with pytest.raises(ValueError, match="method"):
        bsm.Cg(A, method="minres")
    with pytest.raises(TypeError):
        bsm.Cg(np.eye(3))
    with pytest.raises(bsm._lib.BsmError, match="nrhs_max"):
        bsm.Cg(A, nrhs=17)


def test_mixed_storage_handles_count_with_their_double_vectors(bsm):
    p, _, _, _ = cg_problem("vbcrs", np.float64)
    A = bsm.synthetic.build(p, device=NODEV, storage=np.float32)
    assert raw_cg_create(A, 0, None, 0, CODE[np.dtype(np.float64)], 5)[0] == ERR_DEVICE
    assert raw_cg_create(A, 0, None, 0, CODE[np.dtype(np.float32)], 5)[0] == ERR_INVALID
    assert raw_cg_create(A, 0, None, 0, CODE[np.dtype(np.complex128)], 5)[0] == ERR_INVALID
