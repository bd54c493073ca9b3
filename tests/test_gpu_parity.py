"""GPU suite (-m gpu): the HIP path, called through the C ABI (libbsmrocm.so via the host
mirror), against the CPU oracle on identical inputs.

Tolerances (the reference's own norm max|y - y_ref| / max|y_ref|, test/test_vbcrs.jl:35):
    fp64 / complex128 : 1e-12   (BASELINE.json north_star; the reference's tests use 1e-13 on
                                 ~1e3-sized fixtures and `isapprox` rtol 1.5e-8 for products)
    fp32 / complex64  : 1e-5   (observed <= 2e-6)
Bookkeeping (perm / rowptr / colindices / rowindices / colour classes) is bit-exact and is
covered in the CPU suite (tests/test_host_logic.py), which needs no GPU.
"""
import numpy as np
import pytest

from _common import (Cc, N, T, fixture_as_blocksparse, fixture_problem, lens, oracle_mul, rand_vec, relerr,
                     scipy_mul, wrap)
from _gpu import TOL, gpu_mul, torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu
OPS = [N, T, Cc]


def check_all(torch, bsm, oracle, problem, A, dtype, ops=OPS, seeds=(0,), host_too=True):
    dtype = np.dtype(dtype)
    for seed in seeds:
        rng = np.random.default_rng(seed)
        for op in ops:
            if op == Cc and dtype.kind != "c":
                continue
            xl, yl = lens(problem, op)
            x, y0 = rand_vec(rng, xl, dtype), rand_vec(rng, yl, dtype)
            ab = [(1, 0, True), (0.75, -1.5, False)]
            if dtype.kind == "c":
                ab.append((1j, 2j, False))  # mul!(x, A, y, im, 2im), test_blockmatrix.jl:65
            for alpha, beta, strong in ab:
                ref = oracle_mul(oracle, problem, op, x, y0, alpha, beta, strong)
                got = gpu_mul(torch, bsm, A, op, x, y0, alpha, beta, strong)
                assert relerr(got, ref) < TOL[dtype], (op, alpha, beta, strong)
            if host_too:
                ref = oracle_mul(oracle, problem, op, x, y0, 1, 0, True)
                got = gpu_mul(torch, bsm, A, op, x, y0, 1, 0, True, host=True)
                assert relerr(got, ref) < TOL[dtype]


# ---- the reference's fixture ------------------------------------------------------------------
@pytest.mark.parametrize("key", ["cuboid", "sphere"])
@pytest.mark.parametrize("dtype,part", [(np.complex128, "full"), (np.float64, "real"),
                                        (np.float32, "imag"), (np.complex64, "full")])
def test_symmetric_fixture(torch_cuda, bsm, oracle, key, dtype, part):
    p = fixture_problem(key, dtype, part)
    for sched in (bsm.SerialScheduler(), bsm.DynamicScheduler()):
        A = bsm.synthetic.build(p, scheduler=sched)
        check_all(torch_cuda, bsm, oracle, p, A, dtype, seeds=(0, 1))
    # the reference's own check: A*x ~ sparse(A)*x  (test_symmetricblockmatrix.jl:67-71)
    rng = np.random.default_rng(5)
    x = rand_vec(rng, p["size"][1], dtype)
    got = gpu_mul(torch_cuda, bsm, A, N, x, np.zeros(p["size"][0], dtype), 1, 0, True)
    assert relerr(got, scipy_mul(p, N, x, np.zeros(p["size"][0], dtype))) < TOL[np.dtype(dtype)]


@pytest.mark.parametrize("key", ["cuboid", "sphere"])
@pytest.mark.parametrize("acc", ["auto", "atomic"])
def test_blocksparse_fixture(torch_cuda, bsm, oracle, key, acc):
    p = fixture_as_blocksparse(key)
    A = bsm.synthetic.build(p, accumulate=acc)
    assert A.stats()["exclusive"] == (1 if acc == "auto" else 0)
    check_all(torch_cuda, bsm, oracle, p, A, np.complex128)


@pytest.mark.parametrize("key", ["cuboid", "sphere"])
def test_vbcrs_from_symmetric_matches_symmetric(torch_cuda, bsm, oracle, key):
    # reference test/test_vbcrs.jl:52-88 (structure; the contiguous-index fixture is missing from the
    # mount, so a contiguous synthetic symmetric operator stands in for it)
    p = bsm.synthetic.config5(n=3000, lo=1, hi=40, halfband=3, seed=0xB5A5 + (key == "sphere"))
    S = bsm.synthetic.build(p)
    # the view (off-diagonal blocks stored once) and the reference-style materialised conversion
    for V in (bsm.VariableBlockCompressedRowStorage(S),
              bsm.VariableBlockCompressedRowStorage(S, materialize=True)):
        assert bsm.nnz(S) == bsm.nnz(V)
        rng = np.random.default_rng(2)
        for _ in range(3):
            x = rand_vec(rng, p["size"][1], np.float64)
            # the ORACLE's symmetric product (src/symmetricblockmatrix.jl:386-435) is what both are held to -- S and V
            # run the same HIP kernels, so V against S alone would compare the HIP path with itself
            ref = oracle_mul(oracle, p, N, x, np.zeros_like(x))
            sx = gpu_mul(torch_cuda, bsm, S, N, x, np.zeros_like(x), 1, 0, True)
            assert relerr(sx, ref) < 1e-12
            for op in (N, T, Cc):
                vx = gpu_mul(torch_cuda, bsm, V, op if op != Cc else T, x, np.zeros_like(x), 1, 0, True)
                assert relerr(vx, ref) < 1e-12
                assert relerr(vx, sx) < 1e-12


# ---- synthetic configs of BASELINE.json -----------------------------------------------------------
def test_config1_blocksparse(torch_cuda, bsm, oracle):
    p = bsm.synthetic.config1()
    for sched in (bsm.SerialScheduler(), bsm.DynamicScheduler()):
        A = bsm.synthetic.build(p, scheduler=sched)
        check_all(torch_cuda, bsm, oracle, p, A, np.float64)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_config2_vbcrs_full_size(torch_cuda, bsm, oracle, dtype):
    p = bsm.synthetic.config2(dtype=dtype)
    A = bsm.synthetic.build(p)
    st = A.stats()
    assert st["exclusive"] == 1
    check_all(torch_cuda, bsm, oracle, p, A, dtype, host_too=False)
    # VBCRS vs the BlockSparseMatrix on the same blocks (test_vbcrs.jl:31-39)
    ri = [np.arange(r, r + b.shape[0]) for r, b in zip(p["rowstart"], p["blocks"])]
    ci = [np.arange(c, c + b.shape[1]) for c, b in zip(p["colstart"], p["blocks"])]
    B = bsm.BlockSparseMatrix(p["blocks"], ri, ci, p["size"])
    assert bsm.nnz(B) == bsm.nnz(A)
    x = p["x"]
    for op in (N, T):
        a = gpu_mul(torch_cuda, bsm, A, op, x, np.zeros_like(x), 1, 0, True)
        b = gpu_mul(torch_cuda, bsm, B, op, x, np.zeros_like(x), 1, 0, True)
        assert relerr(a, b) < TOL[np.dtype(dtype)]


def test_config3_symmetric_reduced_and_properties(torch_cuda, bsm, oracle):
    p = bsm.synthetic.config3(nseg=200)
    A = bsm.synthetic.build(p)
    check_all(torch_cuda, bsm, oracle, p, A, np.float64, host_too=False)
    # size-independent properties: S == S^T (docs/src/symmetric.md:109), linearity
    rng = np.random.default_rng(11)
    n = p["size"][0]
    x, z = rand_vec(rng, n, np.float64), rand_vec(rng, n, np.float64)
    zero = np.zeros(n)
    sx = gpu_mul(torch_cuda, bsm, A, N, x, zero, 1, 0, True)
    stx = gpu_mul(torch_cuda, bsm, A, T, x, zero, 1, 0, True)
    assert relerr(stx, sx) < 1e-12
    sz = gpu_mul(torch_cuda, bsm, A, N, z, zero, 1, 0, True)
    sxz = gpu_mul(torch_cuda, bsm, A, N, 2 * x - 3 * z, zero, 1, 0, True)
    assert relerr(sxz, 2 * sx - 3 * sz) < 1e-12
    assert abs(np.dot(z, sx) - np.dot(sz, x)) < 1e-10 * abs(np.dot(z, sx))


def test_config3_symmetric_full_size(torch_cuda, bsm, oracle):
    p = bsm.synthetic.config3()
    A = bsm.synthetic.build(p)
    n = p["size"][0]
    x = p["x"]
    ref = oracle_mul(oracle, p, N, x, np.zeros(n))
    got = gpu_mul(torch_cuda, bsm, A, N, x, np.zeros(n), 1, 0, True)
    assert relerr(got, ref) < 1e-12
    y0 = rand_vec(np.random.default_rng(1), n, np.float64)
    ref = oracle_mul(oracle, p, N, x, y0, -0.5, 2.0, False)
    got = gpu_mul(torch_cuda, bsm, A, N, x, y0, -0.5, 2.0, False)
    assert relerr(got, ref) < 1e-12


def test_config4_vbcrs_f32_one_rank_slice(torch_cuda, bsm, oracle):
    # 1/64 of C4's block rows (the slice one GPU of eight would own is 8x this): 256 MB of deep
    # (512 KB) row groups.  Auto mode schedules them as 32 KB work items with atomics; "direct" keeps
    # the exclusive one-launch schedule, which is bitwise reproducible run to run.
    p = bsm.synthetic.config4(ngrid=15625, row_lo=0, row_hi=244)
    A = bsm.synthetic.build(p)
    assert A.stats()["exclusive"] == 0
    check_all(torch_cuda, bsm, oracle, p, A, np.float32, ops=[N, T], host_too=False)
    D = bsm.synthetic.build(p, accumulate="direct")
    assert D.stats()["exclusive"] == 1
    check_all(torch_cuda, bsm, oracle, p, D, np.float32, ops=[N, T], host_too=False)
    rng = np.random.default_rng(44)
    x, y0 = rand_vec(rng, p["size"][1], np.float32), rand_vec(rng, p["size"][0], np.float32)
    first = gpu_mul(torch_cuda, bsm, D, N, x, y0, 0.5, 2.0, False)
    for _ in range(3):
        assert np.array_equal(first, gpu_mul(torch_cuda, bsm, D, N, x, y0, 0.5, 2.0, False))


def test_config5_symmetric_reduced(torch_cuda, bsm, oracle):
    p = bsm.synthetic.config5(n=200_000)
    A = bsm.synthetic.build(p)
    check_all(torch_cuda, bsm, oracle, p, A, np.float64, host_too=False)


# ---- edge cases the reference's semantics imply ------------------------------------------------------
def test_strong_zero_beta_on_gpu(torch_cuda, bsm):
    p = bsm.synthetic.config2(n=3000, nblocks=100)
    A = bsm.synthetic.build(p)
    x = p["x"]
    ynan = np.full(p["size"][0], np.nan)
    y = gpu_mul(torch_cuda, bsm, A, N, x, ynan, 1, 0, True)
    assert np.all(np.isfinite(y))          # Bool false: overwritten (src/abstractblockmatrix.jl:27-34)
    y = gpu_mul(torch_cuda, bsm, A, N, x, ynan, 1, 0.0, False)
    assert np.all(np.isnan(y))             # numeric 0.0 multiplies
    yt = gpu_mul(torch_cuda, bsm, A, T, x, ynan, 1, 0, True)
    assert np.all(np.isfinite(yt))         # fill!(y, 0) of the 3-arg transpose form, src/vbcrs.jl:339


def test_edge_cases_blocksparse(torch_cuda, bsm, oracle):
    rng = np.random.default_rng(3)
    blocks = [rng.standard_normal((1, 1)), np.zeros((0, 3)), np.zeros((2, 0)),
              rng.standard_normal((130, 7)), rng.standard_normal((5, 9)), rng.standard_normal((5, 3)),
              rng.standard_normal((3, 2)), rng.standard_normal((70, 300))]
    rows = [[7], [], [1, 2], list(range(20, 150)), [1, 3, 5, 7, 9], [1, 3, 5, 7, 9], [200, 200, 201],
            list(range(140, 210))]
    cols = [[9], [1, 2, 3], [], [4, 3, 2, 1, 10, 11, 12], list(range(50, 59)), [2, 4, 6], [1, 1],
            list(rng.permutation(300) + 1)]
    p = dict(kind="blocksparse", blocks=[np.asfortranarray(b) for b in blocks], rowindices=rows,
             colindices=cols, size=(210, 300))
    A = bsm.synthetic.build(p)
    check_all(torch_cuda, bsm, oracle, p, A, np.float64)


def test_vbcrs_unequal_heights_and_overlap(torch_cuda, bsm, oracle):
    rng = np.random.default_rng(4)
    blocks = [rng.standard_normal((4, 4)), rng.standard_normal((6, 2)), rng.standard_normal((3, 5))]
    p = dict(kind="vbcrs", blocks=[np.asfortranarray(b) for b in blocks],
             rowstart=np.array([1, 1, 3]), colstart=np.array([1, 5, 2]), size=(8, 8))
    A = bsm.synthetic.build(p)
    check_all(torch_cuda, bsm, oracle, p, A, np.float64)


def test_getindex_matches_sparse(torch_cuda, bsm):
    # A[:, :] vs sparse(A)  (test_blockmatrix.jl:38-49), small operator
    p = bsm.synthetic.config1(n=60, nblocks=6, bs=7)
    A = bsm.synthetic.build(p)
    assert np.max(np.abs(A[:, :] - bsm.sparse(A).toarray())) < 1e-13
    assert np.max(np.abs(bsm.transpose(A)[:, :] - bsm.sparse(A).toarray().T)) < 1e-13


def test_run_to_run_determinism_of_exclusive_path(torch_cuda, bsm):
    p = bsm.synthetic.config2(n=20000, nblocks=1000)
    A = bsm.synthetic.build(p)
    assert A.stats()["exclusive"] == 1
    x = p["x"]
    a = gpu_mul(torch_cuda, bsm, A, N, x, np.zeros_like(x), 1, 0, True)
    for _ in range(3):
        assert np.array_equal(a, gpu_mul(torch_cuda, bsm, A, N, x, np.zeros_like(x), 1, 0, True))


# ---- coloured accumulation: one launch per colour class, plain RMW, bitwise reproducible --------------
@pytest.mark.parametrize("key", ["cuboid", "sphere"])
def test_coloured_mode_parity_and_determinism(torch_cuda, bsm, oracle, key):
    p = fixture_problem(key)
    A = bsm.synthetic.build(p, accumulate="colored")
    check_all(torch_cuda, bsm, oracle, p, A, np.complex128, host_too=False)
    rng = np.random.default_rng(17)
    n = p["size"][0]
    x, y0 = rand_vec(rng, n, np.complex128), rand_vec(rng, n, np.complex128)
    for op in OPS:
        first = gpu_mul(torch_cuda, bsm, A, op, x, y0, 0.5, 2.0, False)
        for _ in range(3):
            assert np.array_equal(first, gpu_mul(torch_cuda, bsm, A, op, x, y0, 0.5, 2.0, False))


def test_coloured_mode_config3_reduced(torch_cuda, bsm, oracle):
    p = bsm.synthetic.config3(nseg=120)
    A = bsm.synthetic.build(p, accumulate="colored")
    check_all(torch_cuda, bsm, oracle, p, A, np.float64, host_too=False)
    q = bsm.synthetic.config1()
    B = bsm.synthetic.build(q, accumulate="colored")
    check_all(torch_cuda, bsm, oracle, q, B, np.float64, host_too=False)


# ---- second ordering: transposed products as a forward launch on a transposed image -------------------
def test_transpose_image_parity_and_determinism(torch_cuda, bsm, oracle):
    p = bsm.synthetic.config2(n=30000, nblocks=1500)
    A = bsm.synthetic.build(p, transpose_image=True)
    check_all(torch_cuda, bsm, oracle, p, A, np.float64, host_too=False)
    x = p["x"]
    first = gpu_mul(torch_cuda, bsm, A, T, x, np.zeros_like(x), 1, 0, True)
    for _ in range(3):  # no atomics on this path: bitwise reproducible
        assert np.array_equal(first, gpu_mul(torch_cuda, bsm, A, T, x, np.zeros_like(x), 1, 0, True))
    q = fixture_as_blocksparse("sphere")
    B = bsm.synthetic.build(q, transpose_image=True)
    check_all(torch_cuda, bsm, oracle, q, B, np.complex128, host_too=False)
    r = bsm.synthetic.config1()
    Cm = bsm.synthetic.build(r, transpose_image=True)
    check_all(torch_cuda, bsm, oracle, r, Cm, np.float64, host_too=False)


# ---- multi right-hand-side product: A * X, mul!(Y, A, X, a, b) with matrices ---------------------------
def _check_multi(torch, bsm, oracle, problem, A, dtype, nrhs_list=(1, 3, 4, 8, 13), ops=OPS):
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(21)
    for op in ops:
        if op == Cc and dtype.kind != "c":
            continue
        xl, yl = lens(problem, op)
        Aop = wrap(bsm, A, op)
        for k in nrhs_list:
            X = np.asfortranarray(np.stack([rand_vec(rng, xl, dtype) for _ in range(k)], axis=1))
            Y0 = np.asfortranarray(np.stack([rand_vec(rng, yl, dtype) for _ in range(k)], axis=1))
            for alpha, beta, strong in ((1, 0, True), (0.5, -2.0, False)):
                # the reference semantics: LinearMaps applies _unsafe_mul! column by column
                ref = np.stack([oracle_mul(oracle, problem, op, X[:, j].copy(), Y0[:, j].copy(), alpha, beta, strong)
                                for j in range(k)], axis=1)
                Xd = torch.from_numpy(X.T.copy()).cuda().t()       # column-major device matrices
                Yd = torch.from_numpy(Y0.T.copy()).cuda().t()
                bsm.mul(Yd, Aop, Xd, alpha, False if strong else beta)
                torch.cuda.synchronize()
                got = Yd.cpu().numpy()
                assert relerr(got.ravel(), ref.ravel()) < TOL[dtype], (op, k, alpha, beta)
            # host matrices (BSM_MEM_HOST) and the `A * X` form
            ref = np.stack([oracle_mul(oracle, problem, op, X[:, j].copy(), np.zeros(yl, dtype)) for j in range(k)], axis=1)
            got = Aop @ X
            assert got.shape == (yl, k) and relerr(got.ravel(), ref.ravel()) < TOL[dtype]


def test_multi_rhs_vbcrs(torch_cuda, bsm, oracle):
    p = bsm.synthetic.config2(n=20000, nblocks=1000)
    _check_multi(torch_cuda, bsm, oracle, p, bsm.synthetic.build(p), np.float64)
    _check_multi(torch_cuda, bsm, oracle, p, bsm.synthetic.build(p, transpose_image=True), np.float64, nrhs_list=(5,))
    q = bsm.synthetic.config2(n=20000, nblocks=1000, dtype=np.float32)
    _check_multi(torch_cuda, bsm, oracle, q, bsm.synthetic.build(q), np.float32, nrhs_list=(8, 5))


@pytest.mark.parametrize("key", ["cuboid"])
def test_multi_rhs_symmetric_and_blocksparse_fixture(torch_cuda, bsm, oracle, key):
    p = fixture_problem(key)
    _check_multi(torch_cuda, bsm, oracle, p, bsm.synthetic.build(p), np.complex128, nrhs_list=(4, 9))
    _check_multi(torch_cuda, bsm, oracle, p, bsm.synthetic.build(p, accumulate="colored"), np.complex128, nrhs_list=(8,))
    q = fixture_as_blocksparse(key)
    _check_multi(torch_cuda, bsm, oracle, q, bsm.synthetic.build(q), np.complex128, nrhs_list=(12,))
    r = bsm.synthetic.config3(nseg=60)
    _check_multi(torch_cuda, bsm, oracle, r, bsm.synthetic.build(r), np.float64, nrhs_list=(8, 6), ops=[N, T])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_multi_rhs_real_sixteen_column_passes_on_the_matrix_pipe(torch_cuda, bsm, oracle, dtype):
    """Real element types with 9 and more right-hand sides: batches of 16 (and padded remainders) run on
    v_mfma_*_16x16x4 (csrc/bsm_multi.hip: kMfmaReal) -- fused symmetric (atomic and coloured launches), exclusive
    VBCRS (plain stores, beta fused, groups combined in LDS), BlockSparseMatrix, the reference's fixture (short
    scattered panels: from 15 columns on), ops N / T, numeric and strong-zero beta, every column against the oracle."""
    r = bsm.synthetic.config3(nseg=40, dtype=dtype)
    _check_multi(torch_cuda, bsm, oracle, r, bsm.synthetic.build(r), dtype, nrhs_list=(16, 11, 35), ops=[N, T])
    _check_multi(torch_cuda, bsm, oracle, r, bsm.synthetic.build(r, accumulate="colored"), dtype, nrhs_list=(16,), ops=[N])
    v = bsm.synthetic.config2(n=12000, nblocks=600, dtype=dtype)
    _check_multi(torch_cuda, bsm, oracle, v, bsm.synthetic.build(v), dtype, nrhs_list=(16, 9), ops=[N, T])
    _check_multi(torch_cuda, bsm, oracle, v, bsm.synthetic.build(v, transpose_image=True), dtype, nrhs_list=(13,), ops=[T])
    f = fixture_problem("cuboid", dtype, "real")
    _check_multi(torch_cuda, bsm, oracle, f, bsm.synthetic.build(f), dtype, nrhs_list=(16, 15, 17), ops=[N])
    q = fixture_as_blocksparse("cuboid", dtype, "real")
    _check_multi(torch_cuda, bsm, oracle, q, bsm.synthetic.build(q), dtype, nrhs_list=(16,), ops=[N, T])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_multi_rhs_real_fused_and_transposed_tile_pipeline(torch_cuda, bsm, oracle, dtype):
    """The 8-column fused / transposed kernels in real arithmetic prefetch their matrix tiles into LDS
    (global_load_lds, counted vmcnt, deferred atomics): every strip height (8 / 16 / 32 / 64 rows, heights that
    are no power of two), gathered and contiguous columns, panels shorter than one iteration, 8 + 4 + 1 splits."""
    p = fixture_problem("cuboid", dtype, "real")                       # gathered column lists
    _check_multi(torch_cuda, bsm, oracle, p, bsm.synthetic.build(p), dtype, nrhs_list=(8, 13), ops=[N, T])
    _check_multi(torch_cuda, bsm, oracle, p, bsm.synthetic.build(p, accumulate="colored"), dtype, nrhs_list=(8,), ops=[N])
    q = fixture_as_blocksparse("cuboid", dtype, "real")                # transposed-only launch, index lists
    _check_multi(torch_cuda, bsm, oracle, q, bsm.synthetic.build(q), dtype, nrhs_list=(8,), ops=[N, T])
    for lo, hi in ((3, 9), (10, 40), (16, 200)):                       # contiguous segments of every height class
        r = bsm.synthetic.config5(n=6000 if hi < 100 else 30000, lo=lo, hi=hi, halfband=3, dtype=dtype)
        _check_multi(torch_cuda, bsm, oracle, r, bsm.synthetic.build(r), dtype, nrhs_list=(8, 16), ops=[N, T])
    v = bsm.synthetic.config2(n=9000, nblocks=500, dtype=dtype)        # VBCRS: transposed product on the single image
    _check_multi(torch_cuda, bsm, oracle, v, bsm.synthetic.build(v), dtype, nrhs_list=(8,), ops=[T])


def test_multi_rhs_interleaved_pass_state_and_ownership(torch_cuda, bsm, oracle):
    """The interleaved multi-RHS pass (csrc/bsm_il.hip: panel_kernel_il -- X and the accumulated Y row-major in work
    arrays of the handle, csrc/bsm_internal.h: LocalOperator::il, claimed by csrc/bsm_capi.cpp: Claim): what the oracle
    comparisons of the other multi-RHS tests do not reach --
      * the work arrays are kept and re-used: alternating ops, batch widths and component counts (8 / 16 per index) on ONE
        handle, rectangular operator (x and y of different lengths), the accumulator must be zero again after every pass;
      * one product in flight per handle: two streams issuing on the same handle without synchronisation -- the one that
        does not get the claim takes the ordinary kernels -- both against the oracle;
      * a handle that owns a row range (bsm_options.own_lo / own_hi): beta applies to the owned rows only, rows outside it
        that blocks reach receive their sums on top of what was there (the single product's semantics)."""
    torch = torch_cuda
    rng = np.random.default_rng(31)
    # rectangular BlockSparseMatrix with index lists, complex: atomics in both directions
    nr, nc, nb = 700, 1100, 60
    blocks, ri, ci = [], [], []
    for b in range(nb):
        m_, n_ = int(rng.integers(3, 30)), int(rng.integers(2, 70))
        blocks.append(np.asfortranarray(rng.standard_normal((m_, n_)) + 1j * rng.standard_normal((m_, n_))))
        ri.append(np.sort(rng.choice(nr, m_, replace=False)) + 1)
        ci.append(rng.choice(nc, n_, replace=False) + 1)
    p = dict(kind="blocksparse", blocks=blocks, rowindices=ri, colindices=ci, size=(nr, nc))
    A = bsm.synthetic.build(p)
    for op, k in ((N, 8), (T, 3), (Cc, 8), (N, 2), (T, 13), (N, 4), (Cc, 5), (N, 8)):
        xl, yl = lens(p, op)
        X = np.asfortranarray(rng.standard_normal((xl, k)) + 1j * rng.standard_normal((xl, k)))
        Y0 = np.asfortranarray(rng.standard_normal((yl, k)) + 1j * rng.standard_normal((yl, k)))
        Xd, Yd = torch.from_numpy(X.T.copy()).cuda().t(), torch.from_numpy(Y0.T.copy()).cuda().t()
        bsm.mul(Yd, wrap(bsm, A, op), Xd, 0.5 - 1j, 2j)
        torch.cuda.synchronize()
        ref = np.stack([oracle_mul(oracle, p, op, X[:, j].copy(), Y0[:, j].copy(), 0.5 - 1j, 2j, False) for j in range(k)], axis=1)
        assert relerr(Yd.cpu().numpy().ravel(), ref.ravel()) < 1e-12, (op, k)
    # two streams, one handle, no synchronisation in between
    f = fixture_problem("cuboid")
    F = bsm.synthetic.build(f)
    n = f["size"][0]
    Xs = [np.asfortranarray(rng.standard_normal((n, 8)) + 1j * rng.standard_normal((n, 8))) for _ in range(2)]
    Xd = [torch.from_numpy(x.T.copy()).cuda().t() for x in Xs]
    Yd = [torch.full((8, n), float("nan"), dtype=torch.complex128, device="cuda").t() for _ in range(2)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for rep in range(6):
        for q in range(2):
            with torch.cuda.stream(streams[q]):
                bsm.mul(Yd[q], F, Xd[q])
    torch.cuda.synchronize()
    for q in range(2):
        ref = np.stack([oracle_mul(oracle, f, N, Xs[q][:, j].copy(), np.zeros(n, np.complex128)) for j in range(8)], axis=1)
        assert relerr(Yd[q].cpu().numpy().ravel(), ref.ravel()) < 1e-12, q
    # a handle that owns the middle rows only
    s_ = bsm.synthetic.config5(n=9000, lo=8, hi=40, halfband=3)
    n = s_["size"][0]
    own = (3001, 6000)
    S = bsm.synthetic.build(s_, own=own)
    for k in (8, 16, 5):
        X = np.asfortranarray(rng.standard_normal((n, k)))
        Y0 = np.asfortranarray(rng.standard_normal((n, k)))
        Xd, Yd = torch.from_numpy(X.T.copy()).cuda().t(), torch.from_numpy(Y0.T.copy()).cuda().t()
        bsm.mul(Yd, S, Xd, 0.75, -1.5)
        torch.cuda.synchronize()
        got = Yd.cpu().numpy()
        for j in range(k):  # the single product through the same handle defines the semantics outside the owned range
            y1 = torch.from_numpy(Y0[:, j].copy()).cuda()
            bsm.mul(y1, S, torch.from_numpy(X[:, j].copy()).cuda(), 0.75, -1.5)
            assert relerr(got[:, j], y1.cpu().numpy()) < 1e-12, (k, j)
        ref = oracle_mul(oracle, s_, N, X[:, 0].copy(), Y0[:, 0].copy(), 0.75, -1.5, False)
        assert relerr(got[own[0] - 1:own[1], 0], ref[own[0] - 1:own[1]]) < 1e-12


@pytest.mark.parametrize("kind", ["symmetric", "vbcrs", "fixture"])
def test_multi_rhs_padded_batches_touch_only_their_columns(torch_cuda, bsm, oracle, kind):
    """2, 3 and 5-7 right-hand sides run as PADDED 4- / 8-column passes (idle slots repeat the last column and
    are never written): every count 1..9 against the oracle, with NaN columns of X and sentinel columns of Y
    right behind the ones the call owns."""
    torch = torch_cuda
    if kind == "symmetric":
        p = bsm.synthetic.config5(n=12000, lo=16, hi=160, halfband=3)
    elif kind == "vbcrs":
        p = bsm.synthetic.config2(n=12000, nblocks=700)
    else:
        p = fixture_problem("cuboid", np.float64, "real")
    A = bsm.synthetic.build(p)
    n = p["size"][0]
    rng = np.random.default_rng(17)
    for op in (N, T):
        Aop = wrap(bsm, A, op)
        for k in range(1, 10):
            X = np.full((n, k + 2), np.nan)
            X[:, :k] = rng.standard_normal((n, k))
            Y0 = np.full((n, k + 2), 7.25)
            Y0[:, :k] = rng.standard_normal((n, k))
            Xd = torch.from_numpy(np.ascontiguousarray(X.T)).cuda().t()   # column-major n x (k + 2)
            Yd = torch.from_numpy(np.ascontiguousarray(Y0.T)).cuda().t()
            bsm.mul(Yd[:, :k], Aop, Xd[:, :k], 0.5, -2.0)
            torch.cuda.synchronize()
            got = Yd.cpu().numpy()
            assert np.all(got[:, k:] == 7.25), (op, k)
            ref = np.stack([oracle_mul(oracle, p, op, X[:, j].copy(), Y0[:, j].copy(), 0.5, -2.0, False) for j in range(k)], axis=1)
            assert relerr(got[:, :k].ravel(), ref.ravel()) < 1e-12, (op, k)


# ---- BASELINE.json's big configs at the size ONE GPU of eight owns: size-independent properties ------
def _dot(a, b):
    return float(np.dot(a.astype(np.float64), b.astype(np.float64)))


def test_config4_one_gpu_share_properties(torch_cuda, bsm):
    # C4: 1/8 of the block rows (2.06 GB fp32).  The oracle check of a smaller slice is above; here:
    # adjoint identity <A x, z> = <x, A^T z>, linearity, and the second ordering against atomics.
    p = bsm.synthetic.config4(row_lo=0, row_hi=1953)
    A = bsm.synthetic.build(p, transpose_image=True)
    rng = np.random.default_rng(31)
    n = p["size"][0]
    x, z = rand_vec(rng, n, np.float32), rand_vec(rng, n, np.float32)
    zero = np.zeros(n, np.float32)
    ax = gpu_mul(torch_cuda, bsm, A, N, x, zero, 1, 0, True)
    atz = gpu_mul(torch_cuda, bsm, A, T, z, zero, 1, 0, True)          # forward launch on the second ordering
    assert abs(_dot(ax, z) - _dot(x, atz)) < 1e-4 * abs(_dot(ax, z))
    az = gpu_mul(torch_cuda, bsm, A, N, z, zero, 1, 0, True)
    both = gpu_mul(torch_cuda, bsm, A, N, (2 * x - 3 * z).astype(np.float32), zero, 1, 0, True)
    # (not a comparison with the oracle: two fp32 results combined in fp32 against a product of the fp32-ROUNDED
    # combination 2x - 3z -- three roundings of size eps * 5 max|x| on top of the product's own error)
    assert relerr(both, 2 * ax - 3 * az) < 2e-5
    del A
    B = bsm.synthetic.build(p)                                          # single image: atomics
    atz2 = gpu_mul(torch_cuda, bsm, B, T, z, zero, 1, 0, True)
    assert relerr(atz2, atz) < 1e-5
    rows_touched = np.zeros(n, bool)
    rows_touched[:1953 * 128] = True
    assert not np.any(ax[~rows_touched])                                # rows without blocks are exactly zero


def test_config5_one_gpu_share_properties(torch_cuda, bsm):
    # C5: the first 1/8 of the rows (3.6 GB fp64, sizes 16-256): symmetry S x = S^T x, <S x, z> = <x, S z>,
    # linearity; VBCRS view of the same operator.
    p = bsm.synthetic.config5(n=625_000)
    S = bsm.synthetic.build(p)
    rng = np.random.default_rng(32)
    n = p["size"][0]
    x, z = rand_vec(rng, n, np.float64), rand_vec(rng, n, np.float64)
    zero = np.zeros(n)
    sx = gpu_mul(torch_cuda, bsm, S, N, x, zero, 1, 0, True)
    stx = gpu_mul(torch_cuda, bsm, S, T, x, zero, 1, 0, True)
    assert relerr(stx, sx) < 1e-12
    sz = gpu_mul(torch_cuda, bsm, S, N, z, zero, 1, 0, True)
    assert abs(np.dot(sx, z) - np.dot(x, sz)) < 1e-11 * abs(np.dot(sx, z))
    comb = gpu_mul(torch_cuda, bsm, S, N, 2 * x - 3 * z, zero, 1, 0, True)
    assert relerr(comb, 2 * sx - 3 * sz) < 1e-12
    y0 = rand_vec(rng, n, np.float64)
    ab = gpu_mul(torch_cuda, bsm, S, N, x, y0, -0.5, 2.0, False)
    assert relerr(ab, -0.5 * sx + 2.0 * y0) < 1e-12
    V = bsm.VariableBlockCompressedRowStorage(S)                        # view: blocks stored once
    assert bsm.nnz(V) == bsm.nnz(S)
    assert relerr(gpu_mul(torch_cuda, bsm, V, N, x, zero, 1, 0, True), sx) < 1e-12


# ---- more edge cases ------------------------------------------------------------------------------------
def test_degenerate_shapes_and_scalars(torch_cuda, bsm, oracle):
    rng = np.random.default_rng(41)
    # no blocks at all: y = beta*y (LinearMaps would still call _unsafe_mul!)
    E0 = bsm.BlockSparseMatrix([], [], [], (7, 5))
    y = gpu_mul(torch_cuda, bsm, E0, N, np.ones(5), np.arange(7.0), 1, 2.0, False)
    assert np.array_equal(y, 2.0 * np.arange(7.0))
    y = gpu_mul(torch_cuda, bsm, E0, T, np.ones(7), np.full(5, np.nan), 1, 0, True)
    assert np.array_equal(y, np.zeros(5))
    # one very wide row, one very tall column, one big dense block, a 1x1, all rectangular
    blocks = [rng.standard_normal((1, 5000)), rng.standard_normal((3000, 1)), rng.standard_normal((700, 900)),
              rng.standard_normal((1, 1))]
    p = dict(kind="blocksparse", blocks=[np.asfortranarray(b) for b in blocks],
             rowindices=[[4000], list(range(1, 3001)), list(range(3100, 3800)), [3900]],
             colindices=[list(range(1, 5001)), [77], list(range(4000, 4900)), [5000]], size=(4000, 5000))
    A = bsm.synthetic.build(p)
    check_all(torch_cuda, bsm, oracle, p, A, np.float64, host_too=False)
    At = bsm.synthetic.build(p, transpose_image=True)
    check_all(torch_cuda, bsm, oracle, p, At, np.float64, ops=[T], host_too=False)
    # alpha = 0, beta = true (1): y unchanged; alpha = true, beta = true accumulates
    x, y0 = rand_vec(rng, 5000, np.float64), rand_vec(rng, 4000, np.float64)
    assert np.array_equal(gpu_mul(torch_cuda, bsm, A, N, x, y0, 0.0, True, False), y0)
    ref = oracle_mul(oracle, p, N, x, y0, 1, 1, False)
    assert relerr(gpu_mul(torch_cuda, bsm, A, N, x, y0, True, True, False), ref) < 1e-12
    # NaN / Inf in x propagate exactly where the reference's arithmetic puts them
    xn = x.copy()
    xn[76] = np.inf  # column 77: feeds the tall 3000 x 1 block only
    yn = gpu_mul(torch_cuda, bsm, A, N, xn, np.zeros(4000), 1, 0, True)
    refn = oracle_mul(oracle, p, N, xn, np.zeros(4000))
    assert np.array_equal(np.isfinite(yn), np.isfinite(refn))


@pytest.mark.parametrize("wave_bytes", ["24576", "11000"])
def test_fat_waves_of_long_low_fill_launches(torch_cuda, bsm, oracle, monkeypatch, wave_bytes):
    # long launches of row groups that do not fill their lanes get 10-24 KB waves (several 8 KB
    # iterations and several x chunks per wave, one or two waves per row group); forced here through
    # BSM_WAVE_BYTES on operators the oracle finishes in seconds: every op, every accumulate mode,
    # several right-hand sides, the reference's fixture included
    monkeypatch.setenv("BSM_WAVE_BYTES", wave_bytes)
    p = bsm.synthetic.config5(n=20000, lo=8, hi=28, halfband=6)
    thin = None
    for acc in ("auto", "colored", "gather"):
        A = bsm.synthetic.build(p, accumulate=acc)
        check_all(torch_cuda, bsm, oracle, p, A, np.float64, host_too=False)
        thin = thin or A.stats()["ntasks"]
    _check_multi(torch_cuda, bsm, oracle, p, bsm.synthetic.build(p), np.float64, nrhs_list=(8, 3), ops=[N, T])
    q = fixture_problem("cuboid")
    check_all(torch_cuda, bsm, oracle, q, bsm.synthetic.build(q), np.complex128, host_too=False)
    r = fixture_as_blocksparse("cuboid")
    check_all(torch_cuda, bsm, oracle, r, bsm.synthetic.build(r), np.complex128, host_too=False)
    v = bsm.synthetic.config2(n=20000, lo=20, hi=64, nblocks=1500, dtype=np.float32)
    check_all(torch_cuda, bsm, oracle, v, bsm.synthetic.build(v, transpose_image=True), np.float32, host_too=False)
    monkeypatch.delenv("BSM_WAVE_BYTES")
    assert bsm.synthetic.build(p).stats()["ntasks"] > thin  # (the default for an operator this small: 8 KB)


def test_vbcrs_wide_block_row_many_blocks(torch_cuda, bsm, oracle):
    # a block row with many blocks (> 3 column runs -> cols pool path) and unsorted input order
    rng = np.random.default_rng(42)
    nb = 40
    cs = rng.permutation(np.arange(nb)) * 50 + 1
    blocks = [np.asfortranarray(rng.standard_normal((20, int(w)))) for w in rng.integers(1, 50, nb)]
    blocks += [np.asfortranarray(rng.standard_normal((9, 33)))]
    p = dict(kind="vbcrs", blocks=blocks, rowstart=np.array([5] * nb + [100]), colstart=np.append(cs, 7),
             size=(120, nb * 50))
    A = bsm.synthetic.build(p)
    assert A.stats()["exclusive"] == 1
    check_all(torch_cuda, bsm, oracle, p, A, np.float64)
    _check_multi(torch_cuda, bsm, oracle, p, A, np.float64, nrhs_list=(8,), ops=[N, T])


def test_symmetric_getindex_and_adjoint_semantics(torch_cuda, bsm):
    # test_symmetricblockmatrix.jl:46-64: sparse(b[:, :]) vs sparse(b), adjoint(b)[:, :] vs conj(transpose),
    # transpose(b)[:, :] vs transpose -- on a small complex-symmetric operator with non-symmetric blocks
    rng = np.random.default_rng(51)
    d1 = rng.standard_normal((3, 3)) + 1j * rng.standard_normal((3, 3))   # deliberately NOT symmetric
    d2 = rng.standard_normal((2, 2)) + 1j * rng.standard_normal((2, 2))
    o1 = rng.standard_normal((3, 2)) + 1j * rng.standard_normal((3, 2))
    o2 = rng.standard_normal((2, 4)) + 1j * rng.standard_normal((2, 4))
    S = bsm.SymmetricBlockMatrix([d1, d2], [[1, 4, 2], [7, 9]], [o1, o2], [[1, 4, 2], [7, 9]],
                                 [[9, 7], [3, 5, 6, 8]], (9, 9), scheduler=bsm.SerialScheduler())
    ref = bsm.sparse(S).toarray()
    assert np.max(np.abs(S[:, :] - ref)) < 1e-13
    # reference semantics of the wrappers (src/symmetricblockmatrix.jl:219-237): the transpose map uses
    # transpose(D) on the diagonal and swaps the off-diagonal roles, the adjoint map conjugates as well
    assert np.max(np.abs(bsm.transpose(S)[:, :] - ref.T)) < 1e-13
    assert np.max(np.abs(bsm.adjoint(S)[:, :] - ref.conj().T)) < 1e-13
    assert np.max(np.abs(bsm.sparse(bsm.transpose(S)).toarray() - ref.T)) < 1e-13
    assert np.max(np.abs(bsm.sparse(bsm.adjoint(S)).toarray() - ref.conj().T)) < 1e-13


# ---- boundary properties promised by include/bsm_rocm.h ----------------------------------------------------
def test_mul_is_graph_capturable_and_stream_ordered(torch_cuda, bsm, oracle):
    # bsm_mul with BSM_MEM_DEVICE only enqueues work: no allocation, no synchronisation
    torch = torch_cuda
    p = bsm.synthetic.config3(nseg=40)
    A = bsm.synthetic.build(p)              # symmetric: scale kernel + fused kernel (2 launches)
    n = p["size"][0]
    x = torch.from_numpy(p["x"]).cuda()
    y = torch.zeros(n, dtype=torch.float64, device="cuda")
    plan = bsm.MulPlan(y, A, x, 0.5, 2.0)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        plan()                               # warm-up outside capture
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            plan()
    torch.cuda.current_stream().wait_stream(s)
    rng = np.random.default_rng(61)
    for _ in range(3):
        xh, yh = rand_vec(rng, n, np.float64), rand_vec(rng, n, np.float64)
        x.copy_(torch.from_numpy(xh))
        y.copy_(torch.from_numpy(yh))
        g.replay()
        torch.cuda.synchronize()
        ref = oracle_mul(oracle, p, N, xh, yh, 0.5, 2.0, False)
        assert relerr(y.cpu().numpy(), ref) < 1e-12


def test_concurrent_mul_on_two_streams_and_threads(torch_cuda, bsm, oracle):
    # a handle is immutable: concurrent products with distinct y on distinct streams are legal
    import threading
    torch = torch_cuda
    p = bsm.synthetic.config2(n=30000, nblocks=1500)
    A = bsm.synthetic.build(p)
    n = p["size"][0]
    rng = np.random.default_rng(62)
    xs = [rand_vec(rng, n, np.float64) for _ in range(2)]
    refs = [oracle_mul(oracle, p, N, xv, np.zeros(n)) for xv in xs]
    outs = [None, None]

    def work(k):
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            xd = torch.from_numpy(xs[k]).cuda()
            yd = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
            for _ in range(50):
                bsm.mul(yd, A, xd)
            st.synchronize()
            outs[k] = yd.cpu().numpy()

    th = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for k in range(2):
        assert relerr(outs[k], refs[k]) < 1e-12


def test_row_partitioned_single_rank_path(torch_cuda, bsm, oracle):
    # distributed.RowPartitioned with world size 1 (no process group): the local product only
    from bsm_amd import distributed as D
    torch = torch_cuda
    p = bsm.synthetic.config2(n=20000, nblocks=800)
    local, own = D.split_vbcrs(p, 0, 1)
    A = bsm.synthetic.build(local, own=own)
    P = D.RowPartitioned(A, own)
    x = torch.from_numpy(p["x"]).cuda()
    y = torch.full((p["size"][0],), float("nan"), dtype=torch.float64, device="cuda")
    P.mul(y, x)
    torch.cuda.synchronize()
    assert relerr(y.cpu().numpy(), oracle_mul(oracle, p, N, p["x"], np.zeros(p["size"][0]))) < 1e-12


def test_multi_rhs_padded_leading_dimension(torch_cuda, bsm, oracle):
    # X / Y stored with ldx, ldy larger than the vector length (views into bigger Julia matrices)
    torch = torch_cuda
    p = bsm.synthetic.config2(n=8000, nblocks=400)
    A = bsm.synthetic.build(p)
    n, k = 8000, 6
    rng = np.random.default_rng(71)
    X = np.stack([rand_vec(rng, n, np.float64) for _ in range(k)], axis=1)
    Xbig = torch.zeros((k, n + 7), dtype=torch.float64, device="cuda")
    Ybig = torch.full((k, n + 13), float("nan"), dtype=torch.float64, device="cuda")
    Xbig[:, :n] = torch.from_numpy(X.T.copy()).cuda()
    Xd, Yd = Xbig.t()[:n], Ybig.t()[:n]          # column-major views: stride (1, n+7) / (1, n+13)
    bsm.mul(Yd, A, Xd)
    torch.cuda.synchronize()
    ref = np.stack([oracle_mul(oracle, p, N, X[:, j].copy(), np.zeros(n)) for j in range(k)], axis=1)
    assert relerr(Yd.cpu().numpy().ravel(), ref.ravel()) < 1e-12
    assert torch.isnan(Ybig[:, n:]).all()           # the padding rows of Y are not touched


# ---- gather accumulation: no atomics, fixed-order sums, bitwise reproducible --------------------------------
@pytest.mark.parametrize("key", ["cuboid", "sphere"])
def test_gather_mode_parity_and_determinism(torch_cuda, bsm, oracle, key):
    p = fixture_problem(key)
    A = bsm.synthetic.build(p, accumulate="gather")
    check_all(torch_cuda, bsm, oracle, p, A, np.complex128)
    rng = np.random.default_rng(81)
    n = p["size"][0]
    x, y0 = rand_vec(rng, n, np.complex128), rand_vec(rng, n, np.complex128)
    for op in OPS:
        first = gpu_mul(torch_cuda, bsm, A, op, x, y0, 0.5, 2.0, False)
        for _ in range(3):
            assert np.array_equal(first, gpu_mul(torch_cuda, bsm, A, op, x, y0, 0.5, 2.0, False))
        # one column through bsm_mul_multi (an (n, 1) Y) is bsm_mul: the same gather path, bitwise
        Y = torch_cuda.from_numpy(y0.copy()).cuda()[:, None]
        bsm.mul(Y, wrap(bsm, A, op), torch_cuda.from_numpy(x).cuda()[:, None], 0.5, 2.0)
        torch_cuda.cuda.synchronize()
        assert np.array_equal(first, Y[:, 0].cpu().numpy())


def test_gather_mode_other_types(torch_cuda, bsm, oracle):
    r = bsm.synthetic.config3(nseg=150)
    check_all(torch_cuda, bsm, oracle, r, bsm.synthetic.build(r, accumulate="gather"), np.float64, host_too=False)
    q = bsm.synthetic.config1()
    check_all(torch_cuda, bsm, oracle, q, bsm.synthetic.build(q, accumulate="gather"), np.float64, host_too=False)
    v = bsm.synthetic.config2(n=20000, nblocks=1000, dtype=np.float32)
    check_all(torch_cuda, bsm, oracle, v, bsm.synthetic.build(v, accumulate="gather", transpose_image=True),
              np.float32, host_too=False)
    c5 = bsm.synthetic.config5(n=60000)
    A = bsm.synthetic.build(c5, accumulate="gather")
    check_all(torch_cuda, bsm, oracle, c5, A, np.float64, host_too=False)
    _check_multi(torch_cuda, bsm, oracle, c5, A, np.float64, nrhs_list=(5,), ops=[N])  # multi-RHS: atomic path


def test_gather_mode_two_streams_share_one_workspace(torch_cuda, bsm, oracle):
    # the gather workspace belongs to the handle: a product that finds another one in flight on a
    # different stream must not touch it (it takes the atomic path for that call)
    torch = torch_cuda
    p = bsm.synthetic.config5(n=40000, lo=16, hi=96, halfband=3)
    A = bsm.synthetic.build(p, accumulate="gather")
    n = p["size"][0]
    rng = np.random.default_rng(91)
    xs = [rand_vec(rng, n, np.float64) for _ in range(2)]
    refs = [oracle_mul(oracle, p, N, xv, np.zeros(n)) for xv in xs]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    xd = [torch.from_numpy(v).cuda() for v in xs]
    yd = [torch.full((n,), float("nan"), dtype=torch.float64, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    for it in range(40):
        for k in range(2):  # alternate the streams without waiting in between
            with torch.cuda.stream(streams[k]):
                bsm.mul(yd[k], A, xd[k])
    torch.cuda.synchronize()
    for k in range(2):
        assert relerr(yd[k].cpu().numpy(), refs[k]) < 1e-12


def test_streamed_upload_matches_one_shot_upload(torch_cuda, bsm, oracle, monkeypatch):
    # large operators are packed window by window into pinned staging and copied while the next
    # window is packed (bsm_operator.cpp DeviceSink); forced here on small operators with tiny windows
    monkeypatch.setenv("BSM_STREAM_MIN_BYTES", "1")
    monkeypatch.setenv("BSM_UPLOAD_WINDOW_BYTES", "20000")
    for p, dt, kw in ((bsm.synthetic.config2(n=20000, nblocks=900), np.float64, {"transpose_image": True}),
                      (bsm.synthetic.config5(n=30000, lo=8, hi=90, halfband=3), np.float64, {}),
                      (fixture_problem("cuboid"), np.complex128, {"accumulate": "gather"}),
                      (bsm.synthetic.config1(), np.float64, {})):
        A = bsm.synthetic.build(p, **kw)
        check_all(torch_cuda, bsm, oracle, p, A, dt, host_too=False)


@pytest.mark.parametrize("dtype,part", [(np.complex128, "full"), (np.float64, "real")])
def test_bem_fixture_tiled_along_the_diagonal(torch_cuda, bsm, oracle, dtype, part):
    """The reference's real BEM structure at a size where the launch has several rounds of workgroups
    (tools/bem_real.py's operator, 12 tiles instead of 300): the "cuboid" fixture repeated along the
    diagonal -- 3-28-row leaves, scattered near-field columns, the LDS y window of locality-packed
    workgroups -- fused symmetric product and both wrappers against the oracle."""
    K = 12
    p = fixture_problem("cuboid", dtype, part)
    n0 = p["size"][0]

    def tile(lists):
        return [l + k * n0 for k in range(K) for l in lists]

    prob = dict(kind="symmetric", diagonals=p["diagonals"] * K, diagonalindices=tile(p["diagonalindices"]),
                offdiagonals=p["offdiagonals"] * K, rowindices=tile(p["rowindices"]),
                colindices=tile(p["colindices"]), size=(n0 * K, n0 * K))
    A = bsm.synthetic.build(prob)
    assert bsm.nnz(A) == K * (sum(b.size for b in p["diagonals"]) + 2 * sum(b.size for b in p["offdiagonals"]))
    check_all(torch_cuda, bsm, oracle, prob, A, dtype, host_too=False)
    for acc in ("gather", "colored"):  # the bitwise reproducible modes on the same structure
        B = bsm.synthetic.build(prob, accumulate=acc)
        check_all(torch_cuda, bsm, oracle, prob, B, dtype, ops=[N], host_too=False)
