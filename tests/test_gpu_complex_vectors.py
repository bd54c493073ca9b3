"""GPU suite (-m gpu): complex vectors under a real handle (bsm_mul_cvec / bsm_mul_multi_cvec) -- a float64 operator
applied to complex128 vectors, a float32 one to complex64, in one pass over the matrix.  The reference is the CPU
oracle run on the same problem with the real blocks promoted to complex128.

    (float64, complex128): <= 1e-13 relative        (float32, complex64): <= 1e-5 relative
"""
import ctypes as C

import numpy as np
import pytest

from _common import Cc, N, NODEV, T, fixture_as_blocksparse, fixture_problem, get_image, lens, oracle_mul, rand_vec, relerr, wrap
from _ctors import ctor_build, ctor_oracle_problem, ctor_problem
from _fuzz import cast_blocks
from _gpu import dev_mat, gpu_mul, outside_bytes, torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu
OPS = [N, T, Cc]
PAIRS = [(np.float64, np.complex128), (np.float32, np.complex64)]
ACCS = ["auto", "colored", "atomic", "gather"]
CTORS = ["vbcrs", "vbcrs_from_symmetric", "blocksparse", "symmetric"]
TOL = {np.dtype(np.complex128): 1e-13, np.dtype(np.complex64): 1e-5}
# the generators' keywords per constructor route; FULL: C2 and C3 at full size
SIZES = {"blocksparse": dict(n=600, nblocks=60, bs=16), "vbcrs": dict(n=4000, nblocks=200, lo=4, hi=48),
         "symmetric": dict(nseg=16, bs=24, halfband=2), "vbcrs_from_symmetric": dict(nseg=16, bs=24, halfband=2)}
FULL = {"vbcrs": {}, "symmetric": {}}


def _complex_problem(ctor, p):
    """the problem as the oracle takes it, blocks promoted to complex128"""
    return cast_blocks(ctor_oracle_problem(ctor, p), np.complex128)


def _orc(oracle, q, op, x, y0, alpha=1, beta=0, strong=True):
    c = np.complex128
    return oracle_mul(oracle, q, op, np.asarray(x, c), np.asarray(y0, c), alpha, beta, strong)


# (transpose_image applies to VBCRS / BlockSparseMatrix operators without symmetric pieces)
CTOR_TIMAGE = [(c, t) for c in CTORS for t in (0, 1) if t == 0 or c in ("vbcrs", "blocksparse")]


@pytest.mark.parametrize("acc", ACCS)
@pytest.mark.parametrize("R_, C_", PAIRS)
@pytest.mark.parametrize("ctor, timage", CTOR_TIMAGE)
def test_cvec_product_matrix(torch_cuda, bsm, oracle, ctor, timage, R_, C_, acc):
    p = ctor_problem(bsm, ctor, R_, SIZES)
    A = ctor_build(bsm, ctor, p, accumulate=acc, transpose_image=timage)
    q = _complex_problem(ctor, p)
    rng = np.random.default_rng(1)
    tol = TOL[np.dtype(C_)]
    for op in OPS:
        xl, yl = lens(p, op)
        x, y0 = rand_vec(rng, xl, C_), rand_vec(rng, yl, C_)
        got = gpu_mul(torch_cuda, bsm, A, op, x, y0)
        assert got.dtype == np.dtype(C_)
        assert relerr(got, _orc(oracle, q, op, x, y0)) <= tol, op
        got = gpu_mul(torch_cuda, bsm, A, op, x, y0, 0.5, 2.0, False)
        assert relerr(got, _orc(oracle, q, op, x, y0, 0.5, 2.0, False)) <= tol, op
        if acc in ("colored", "gather"):  # bitwise reproducible run to run
            a = gpu_mul(torch_cuda, bsm, A, op, x, y0, 0.5, 2.0, False)
            assert a.tobytes() == got.tobytes(), op


@pytest.mark.parametrize("R_, C_", PAIRS)
@pytest.mark.parametrize("ctor", ["vbcrs", "symmetric"])
def test_cvec_complex_scalars_strong_and_numeric_zero(torch_cuda, bsm, oracle, ctor, R_, C_):
    p = ctor_problem(bsm, ctor, R_, SIZES)
    A = ctor_build(bsm, ctor, p)
    q = _complex_problem(ctor, p)
    rng = np.random.default_rng(2)
    n = p["size"][0]
    tol = TOL[np.dtype(C_)]
    x = rand_vec(rng, n, C_)
    ynan = np.full(n, np.nan, dtype=C_)
    alpha, beta = 0.5 - 0.25j, 1.5 + 0.5j
    for op in OPS:
        got = gpu_mul(torch_cuda, bsm, A, op, x, ynan, alpha, 0, True)  # strong zero: the NaN must vanish
        assert np.all(np.isfinite(got))
        assert relerr(got, _orc(oracle, q, op, x, ynan, alpha, 0, True)) <= tol
        got = gpu_mul(torch_cuda, bsm, A, op, x, ynan, alpha, 0.0, False)  # numeric zero multiplies: NaN stays
        assert np.all(np.isnan(got))
        y0 = rand_vec(rng, n, C_)
        got = gpu_mul(torch_cuda, bsm, A, op, x, y0, alpha, beta, False)
        assert relerr(got, _orc(oracle, q, op, x, y0, alpha, beta, False)) <= tol
        # MulPlan, A @ x
        xd = torch_cuda.from_numpy(x).cuda()
        yd = torch_cuda.from_numpy(y0.copy()).cuda()
        bsm.MulPlan(yd, wrap(bsm, A, op), xd, alpha, beta)()
        torch_cuda.cuda.synchronize()
        assert relerr(yd.cpu().numpy(), got) <= tol  # (atomic paths: not bitwise run to run)
        if op == N:
            z = A @ xd
            assert z.dtype == xd.dtype
            assert relerr(z.cpu().numpy(), _orc(oracle, q, N, x, np.zeros(n))) <= tol


@pytest.mark.parametrize("R_, C_", PAIRS)
def test_cvec_host_and_device_vectors_and_owned_rows(torch_cuda, bsm, oracle, R_, C_):
    torch = torch_cuda
    tol = TOL[np.dtype(C_)]
    prob = cast_blocks(bsm.synthetic.config2(n=4000, nblocks=150), R_)
    A = bsm.synthetic.build(prob)
    q = cast_blocks(prob, np.complex128)
    rng = np.random.default_rng(3)
    for op in OPS:
        x, y0 = rand_vec(rng, 4000, C_), rand_vec(rng, 4000, C_)
        h = y0.copy()
        bsm.mul(h, wrap(bsm, A, op), x.copy(), 0.25 + 1j, -1.0 + 0.5j)  # host (numpy) vectors
        d = gpu_mul(torch, bsm, A, op, x, y0, 0.25 + 1j, -1.0 + 0.5j, False)
        assert relerr(h, _orc(oracle, q, op, x, y0, 0.25 + 1j, -1.0 + 0.5j, False)) <= tol
        assert relerr(h, d) <= tol
    # a handle that owns a row range: rows outside it come back bit-unchanged, host path and device path
    keep = [b for b, r in enumerate(prob["rowstart"]) if 1000 <= r < 2500]
    sub = dict(kind="vbcrs", blocks=[prob["blocks"][b] for b in keep], rowstart=prob["rowstart"][keep],
               colstart=prob["colstart"][keep], size=prob["size"])
    lo = int(min(sub["rowstart"]))
    hi = int(max(r + b.shape[0] - 1 for r, b in zip(sub["rowstart"], sub["blocks"])))
    Ao = bsm.synthetic.build(sub, own=(lo, hi))
    x = rand_vec(rng, 4000, C_)
    ref = _orc(oracle, cast_blocks(sub, np.complex128), N, x, np.zeros(4000))
    for first in (3.5 - 1.25j, -7.25 + 2j):
        y = np.full(4000, first, dtype=C_)
        bsm.mul(y, Ao, x.copy())
        assert y[:lo - 1].tobytes() == np.full(lo - 1, first, C_).tobytes()
        assert y[hi:].tobytes() == np.full(4000 - hi, first, C_).tobytes()
        assert relerr(y[lo - 1:hi], ref[lo - 1:hi]) <= tol
        yd = torch.full((4000,), first, dtype=torch.from_numpy(y).dtype, device="cuda")
        bsm.mul(yd, Ao, torch.from_numpy(x).cuda())
        torch.cuda.synchronize()
        assert yd.cpu().numpy().tobytes() == y.tobytes()
        # several right-hand sides (the interleaved pass over an exclusive forward image): the same rows untouched
        k = 8
        X = np.asfortranarray(np.stack([rand_vec(rng, 4000, C_) for _ in range(k)], axis=1))
        Y = np.asfortranarray(np.full((4000, k), first, dtype=C_))
        bsm.mul(Y, Ao, X)
        assert Y[:lo - 1].tobytes() == np.full((lo - 1, k), first, C_).tobytes()
        assert Y[hi:].tobytes() == np.full((4000 - hi, k), first, C_).tobytes()
        for j in range(k):
            r = _orc(oracle, cast_blocks(sub, np.complex128), N, X[:, j], np.zeros(4000))
            assert relerr(Y[lo - 1:hi, j], r[lo - 1:hi]) <= tol, j


@pytest.mark.parametrize("R_, C_", PAIRS)
@pytest.mark.parametrize("key", ["cuboid", "sphere"])
def test_cvec_golden_fixtures_real_part(torch_cuda, bsm, oracle, key, R_, C_):
    """the real part of the reference's BEM fixtures (ComplexF64 near fields), as a symmetric and as a block-sparse
    operator, times complex vectors"""
    tol = TOL[np.dtype(C_)]
    rng = np.random.default_rng(4)
    for p in (fixture_problem(key, dtype=R_, part="real"), fixture_as_blocksparse(key, dtype=R_, part="real")):
        A = bsm.synthetic.build(p)
        q = cast_blocks(p, np.complex128)
        for op in OPS:
            xl, yl = lens(p, op)
            x, y0 = rand_vec(rng, xl, C_), rand_vec(rng, yl, C_)
            got = gpu_mul(torch_cuda, bsm, A, op, x, y0, 1 - 0.5j, 0.5j, False)
            assert relerr(got, _orc(oracle, q, op, x, y0, 1 - 0.5j, 0.5j, False)) <= tol, (p["kind"], op)


@pytest.mark.parametrize("R_, C_", PAIRS)
def test_cvec_lds_window_longer_than_a_complex_window(torch_cuda, bsm, oracle, R_, C_):
    """The analysis of a real image cuts its LDS y windows for the REAL element size; a complex window of the same
    4 KB holds half the entries.  The operator must have windows beyond that bound, and the complex product must
    still be exact (bsm_one.hip: panel_kernel clamps the window of complex vectors under a real image)."""
    p = fixture_problem("sphere", dtype=R_, part="real")
    twin = bsm.synthetic.build(p, device=NODEV)
    waves = get_image(twin)[3]
    bound = 4096 // np.dtype(C_).itemsize  # entries of a complex window of 4 KB: 256 complex128, 512 complex64
    assert np.any(waves["win_span8"].astype(np.int64) * 8 > bound)
    A = bsm.synthetic.build(p)
    q = cast_blocks(p, np.complex128)
    rng = np.random.default_rng(5)
    n = p["size"][0]
    for op in OPS:
        x, y0 = rand_vec(rng, n, C_), rand_vec(rng, n, C_)
        got = gpu_mul(torch_cuda, bsm, A, op, x, y0, 0.75, -1.5j, False)
        assert relerr(got, _orc(oracle, q, op, x, y0, 0.75, -1.5j, False)) <= TOL[np.dtype(C_)], op


@pytest.mark.parametrize("R_, C_", PAIRS)
@pytest.mark.parametrize("ctor", ["vbcrs", "symmetric"])
def test_cvec_gather_handle_is_bitwise_reproducible(torch_cuda, bsm, ctor, R_, C_):
    p = ctor_problem(bsm, ctor, R_, SIZES)
    A = ctor_build(bsm, ctor, p, accumulate="gather")
    rng = np.random.default_rng(6)
    for op in OPS:
        xl, yl = lens(p, op)
        x, y0 = rand_vec(rng, xl, C_), rand_vec(rng, yl, C_)
        a = gpu_mul(torch_cuda, bsm, A, op, x, y0, 0.5 + 0.5j, 2.0, False)
        b = gpu_mul(torch_cuda, bsm, A, op, x, y0, 0.5 + 0.5j, 2.0, False)
        assert a.tobytes() == b.tobytes(), op


@pytest.mark.parametrize("R_, C_", PAIRS)
@pytest.mark.parametrize("ctor", ["vbcrs", "symmetric", "blocksparse"])
def test_cvec_multi_rhs(torch_cuda, bsm, oracle, ctor, R_, C_):
    torch = torch_cuda
    p = ctor_problem(bsm, ctor, R_, SIZES)
    A = ctor_build(bsm, ctor, p)
    q = _complex_problem(ctor, p)
    tol = TOL[np.dtype(C_)]
    rng = np.random.default_rng(7)
    alpha, beta = 0.5 - 1j, 0.25 + 0.5j
    for op in (N, Cc):
        xl, yl = lens(p, op)
        for k in (1, 2, 4, 5, 8, 9, 17):
            xb, X = dev_mat(torch, np.stack([rand_vec(rng, xl, C_) for _ in range(k)], axis=1), 13)
            yb, Y = dev_mat(torch, np.stack([rand_vec(rng, yl, C_) for _ in range(k)], axis=1), 7)
            X0, Y0 = X.cpu().numpy(), Y.cpu().numpy()
            bsm.mul(Y, wrap(bsm, A, op), X, alpha, beta)
            torch.cuda.synchronize()
            assert np.all(np.isnan(np.frombuffer(outside_bytes(yb, yl, yl + 7, k), dtype=C_))), (op, k)  # the padding rows are untouched
            assert np.all(np.isnan(np.frombuffer(outside_bytes(xb, xl, xl + 13, k), dtype=C_)))
            got = Y.cpu().numpy()
            for j in range(k):
                one = gpu_mul(torch, bsm, A, op, X0[:, j], Y0[:, j], alpha, beta, False)
                assert relerr(got[:, j], one) <= tol, (op, k, j)
                assert relerr(got[:, j], _orc(oracle, q, op, X0[:, j], Y0[:, j], alpha, beta, False)) <= tol, (op, k, j)
    # A @ X: a complex column-major result
    X = np.asfortranarray(np.stack([rand_vec(rng, p["size"][1], C_) for _ in range(3)], axis=1))
    Z = A @ X
    assert Z.dtype == np.dtype(C_) and Z.shape == (p["size"][0], 3)


@pytest.mark.parametrize("R_, C_", PAIRS)
def test_cvec_graph_capture(torch_cuda, bsm, R_, C_):
    torch = torch_cuda
    p = ctor_problem(bsm, "symmetric", R_, SIZES)
    A = ctor_build(bsm, "symmetric", p, accumulate="colored")
    n = p["size"][0]
    rng = np.random.default_rng(8)
    tol = TOL[np.dtype(C_)]
    x = torch.from_numpy(rand_vec(rng, n, C_)).cuda()
    y = torch.zeros(n, dtype=x.dtype, device="cuda")
    eager = torch.zeros_like(y)
    bsm.mul(eager, A, x, 0.5 + 0.5j)
    k = 8
    X = torch.from_numpy(np.stack([rand_vec(rng, n, C_) for _ in range(k)])).cuda().t()
    Y = torch.zeros((k, n), dtype=x.dtype, device="cuda").t()
    eager_m = torch.zeros((k, n), dtype=x.dtype, device="cuda").t()
    bsm.mul(eager_m, A, X, 0.5 + 0.5j)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up outside the capture
        bsm.mul(y, A, x, 0.5 + 0.5j)
        bsm.mul(Y, A, X, 0.5 + 0.5j)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        bsm.mul(y, A, x, 0.5 + 0.5j)
        bsm.mul(Y, A, X, 0.5 + 0.5j)
    reps = []
    for _ in range(2):
        y.fill_(float("nan"))
        Y.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert y.cpu().numpy().tobytes() == eager.cpu().numpy().tobytes()
        reps.append(Y.cpu().numpy())
        assert relerr(reps[-1], eager_m.cpu().numpy()) <= tol
    assert reps[0].tobytes() == reps[1].tobytes()


@pytest.mark.parametrize("ctor", ["vbcrs", "symmetric"])
def test_cvec_full_size_c2_c3(torch_cuda, bsm, oracle, ctor):
    """C2 (VBCRS, 100 k rows) and C3 (symmetric, 200 k rows) at full size, float64 with complex128 vectors"""
    p = ctor_problem(bsm, ctor, np.float64, FULL)
    A = ctor_build(bsm, ctor, p)
    q = cast_blocks(p, np.complex128)
    rng = np.random.default_rng(9)
    x = rand_vec(rng, p["size"][1], np.complex128)
    y0 = np.full(p["size"][0], np.nan, dtype=np.complex128)
    got = gpu_mul(torch_cuda, bsm, A, N, x, y0)
    assert relerr(got, _orc(oracle, q, N, x, y0)) <= 1e-13


def test_cvec_refused_on_mixed_and_multi_device_handles(torch_cuda, bsm):
    """a mixed-storage handle and a multi-device handle (a real context of two virtual devices):
    BSM_ERR_UNSUPPORTED from the C ABI, TypeError from the mirror"""
    from bsm_amd import _lib as L
    p = ctor_problem(bsm, "vbcrs", np.float64, SIZES)
    n = p["size"][0]
    x = torch_cuda.from_numpy(rand_vec(np.random.default_rng(10), n, np.complex128)).cuda()
    y = torch_cuda.zeros_like(x)
    one = C.c_int64(n)
    for A in (ctor_build(bsm, "vbcrs", p, storage=np.float32), ctor_build(bsm, "vbcrs", p, devices=[0, 0])):
        assert L.lib().bsm_mul_cvec(A._h.ptr, N, x.data_ptr(), y.data_ptr(), None, None, 1, 1, None) == -2
        assert L.lib().bsm_mul_multi_cvec(A._h.ptr, N, 1, x.data_ptr(), one, y.data_ptr(), one, None, None, 1, 1,
                                          None) == -2
        with pytest.raises(TypeError):
            bsm.mul(y, A, x)
