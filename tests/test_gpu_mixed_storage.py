"""GPU suite (-m gpu): mixed-precision handles (BSM_F64_F32, BSM_C128_C64) -- values stored as float32 / complex64,
x, y, alpha, beta and every sum in float64 / complex128.

    mixed y  vs a pure double-precision handle of the ROUNDED blocks : <= 1e-13 (a sum kept in fp32 would miss by 1e6)
    mixed y  vs the oracle on the ORIGINAL blocks                    : within single-precision rounding (<= 1e-5)
"""
import numpy as np
import pytest

from _common import Cc, N, T, lens, oracle_mul, rand_vec, relerr, wrap
from _ctors import CTORS, ctor_build, ctor_oracle_problem, ctor_problem
from _fuzz import cast_blocks, rounded
from _gpu import gpu_mul, torch_cuda  # noqa: F401
from _values import on_device

pytestmark = pytest.mark.gpu
OPS = [N, T, Cc]
PAIRS = [(np.float64, np.float32), (np.complex128, np.complex64)]
ACCS = ["auto", "atomic", "colored", "gather", "direct"]
# the generators' keywords per constructor route; FULL: C2 and C3 at full size
SIZES = {"blocksparse": dict(n=600, nblocks=60, bs=16), "vbcrs": dict(n=4000, nblocks=200, lo=4, hi=48),
         "vbcrs_from_blocksparse": dict(n=3000, nblocks=150, lo=4, hi=48), "symmetric": dict(nseg=16, bs=24, halfband=2),
         "vbcrs_from_symmetric": dict(nseg=16, bs=24, halfband=2)}
FULL = {"vbcrs": {}, "symmetric": {}}


# (transpose_image applies to VBCRS / BlockSparseMatrix operators without symmetric pieces)
CTOR_TIMAGE = [(c, t) for c in CTORS for t in (0, 1) if t == 0 or c not in ("symmetric", "vbcrs_from_symmetric")]


@pytest.mark.parametrize("acc", ACCS)
@pytest.mark.parametrize("T_, S_", PAIRS)
@pytest.mark.parametrize("ctor, timage", CTOR_TIMAGE)
def test_mixed_product_matrix(torch_cuda, bsm, oracle, ctor, timage, T_, S_, acc):
    p = ctor_problem(bsm, ctor, T_, SIZES)
    A = ctor_build(bsm, ctor, p, storage=S_, accumulate=acc, transpose_image=timage)
    R = ctor_build(bsm, ctor, rounded(p, S_), accumulate=acc, transpose_image=timage)  # pure T, rounded blocks
    rng = np.random.default_rng(1)
    for op in OPS:
        xl, yl = lens(p, op)
        x = rand_vec(rng, xl, T_)
        y0 = rand_vec(rng, yl, T_)
        for alpha, beta, strong in ((1, 0, True), (0.5, 2.0, False)):
            got = gpu_mul(torch_cuda, bsm, A, op, x, y0, alpha, beta, strong)
            ref = gpu_mul(torch_cuda, bsm, R, op, x, y0, alpha, beta, strong)
            assert relerr(got, ref) <= 1e-13, (op, alpha, beta)
        orc = oracle_mul(oracle, ctor_oracle_problem(ctor, p), op, x, y0)
        assert relerr(gpu_mul(torch_cuda, bsm, A, op, x, y0), orc) <= 1e-5
        # bitwise reproducible run to run: coloured and gather products always, DIRECT where it takes the exclusive
        # stores (op N of a conflict-free operator; otherwise it is the atomic path, like AUTO)
        if acc in ("colored", "gather") or (acc == "direct" and op == N and A.stats()["exclusive"] == 1):
            a = gpu_mul(torch_cuda, bsm, A, op, x, y0, 0.5, 2.0, False)
            b = gpu_mul(torch_cuda, bsm, A, op, x, y0, 0.5, 2.0, False)
            assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("T_, S_", PAIRS)
@pytest.mark.parametrize("ctor", ["vbcrs", "symmetric"])
def test_mixed_alpha_beta_strong_zero_nan(torch_cuda, bsm, oracle, ctor, T_, S_):
    p = ctor_problem(bsm, ctor, T_, SIZES)
    A = ctor_build(bsm, ctor, p, storage=S_)
    orc_p = ctor_oracle_problem(ctor, rounded(p, S_))
    rng = np.random.default_rng(2)
    n = p["size"][0]
    x = rand_vec(rng, n, T_)
    ynan = np.full(n, np.nan, dtype=T_)
    cplx = np.dtype(T_).kind == "c"
    alpha = 0.5 - 0.25j if cplx else -0.75
    for op in OPS:
        got = gpu_mul(torch_cuda, bsm, A, op, x, ynan, alpha, 0, True)  # strong zero: the NaN must not propagate
        assert np.all(np.isfinite(got))
        assert relerr(got, oracle_mul(oracle, orc_p, op, x, ynan, alpha, 0, True)) <= 1e-13
        got = gpu_mul(torch_cuda, bsm, A, op, x, ynan, alpha, 0.0, False)  # numeric zero multiplies: NaN stays
        assert np.all(np.isnan(got))
        y0 = rand_vec(rng, n, T_)
        beta = 1.5 + 0.5j if cplx else 1.5
        got = gpu_mul(torch_cuda, bsm, A, op, x, y0, alpha, beta, False)
        assert relerr(got, oracle_mul(oracle, orc_p, op, x, y0, alpha, beta, False)) <= 1e-13


@pytest.mark.parametrize("T_, S_", PAIRS)
@pytest.mark.parametrize("ctor", CTORS)
def test_mixed_rowcolvals_host_and_device_blocks(torch_cuda, bsm, ctor, T_, S_):
    p = ctor_problem(bsm, ctor, T_, SIZES)
    if np.dtype(T_) == np.float64:  # subnormal, overflowing and tie-breaking entries round alike on both packers
        key = "blocks" if "blocks" in p else "offdiagonals"
        b = p[key][0].copy(order="F")
        b.flat[:6] = [1e-40, -3e-42, 1e39, 1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24, 2.0 ** -149]
        p[key] = [b] + list(p[key][1:])
    Ah = ctor_build(bsm, ctor, p, storage=S_)
    Ad = ctor_build(bsm, ctor, on_device(torch_cuda, p), storage=S_)
    rh, ch, vh = (t.cpu().numpy() for t in bsm.rowcolvals_device(Ah))
    rd, cd, vd = (t.cpu().numpy() for t in bsm.rowcolvals_device(Ad))
    assert vh.dtype == np.dtype(T_)
    assert np.array_equal(rh, rd) and np.array_equal(ch, cd) and vh.tobytes() == vd.tobytes()
    # exactly astype(S).astype(T) of the pure single-precision handle's values
    with np.errstate(over="ignore"):
        As = ctor_build(bsm, ctor, cast_blocks(p, S_))
    rs, cs, vs = (t.cpu().numpy() for t in bsm.rowcolvals_device(As))
    assert np.array_equal(rh, rs) and np.array_equal(ch, cs)
    assert vh.tobytes() == vs.astype(T_).tobytes()


@pytest.mark.parametrize("T_, S_", PAIRS)
@pytest.mark.parametrize("ctor", ["vbcrs", "symmetric", "blocksparse"])
def test_mixed_mul_multi_is_column_by_column(torch_cuda, bsm, ctor, T_, S_):
    torch = torch_cuda
    p = ctor_problem(bsm, ctor, T_, SIZES)
    A = ctor_build(bsm, ctor, p, storage=S_, accumulate="colored")
    n, k = p["size"][0], 5
    rng = np.random.default_rng(4)
    X = np.stack([rand_vec(rng, n, T_) for _ in range(k)], axis=1)
    for op in OPS:
        Xd = torch.from_numpy(np.ascontiguousarray(X.T)).cuda().t()
        Yd = torch.zeros((k, n), dtype=Xd.dtype, device="cuda").t()
        bsm.mul(Yd, wrap(bsm, A, op), Xd)
        torch.cuda.synchronize()
        Y = Yd.cpu().numpy()
        for j in range(k):
            col = gpu_mul(torch, bsm, A, op, X[:, j].copy(), np.zeros(n, T_))
            assert Y[:, j].tobytes() == col.tobytes(), (op, j)


@pytest.mark.parametrize("T_, S_", PAIRS)
def test_mixed_graph_replay(torch_cuda, bsm, T_, S_):
    torch = torch_cuda
    p = ctor_problem(bsm, "symmetric", T_, SIZES)
    A = ctor_build(bsm, "symmetric", p, storage=S_, accumulate="colored")
    n = p["size"][0]
    rng = np.random.default_rng(5)
    x = torch.from_numpy(rand_vec(rng, n, T_)).cuda()
    y = torch.zeros(n, dtype=x.dtype, device="cuda")
    eager = torch.zeros_like(y)
    bsm.mul(eager, A, x)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        bsm.mul(y, A, x)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        bsm.mul(y, A, x)
    for _ in range(2):
        y.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert y.cpu().numpy().tobytes() == eager.cpu().numpy().tobytes()


@pytest.mark.parametrize("ctor", ["vbcrs", "symmetric"])
def test_mixed_full_size_c2_c3(torch_cuda, bsm, oracle, ctor):
    """C2 (VBCRS, 100 k rows) and C3 (symmetric, 200 k rows) at full size, device-block creates"""
    p = ctor_problem(bsm, ctor, np.float64, FULL)
    A = ctor_build(bsm, ctor, on_device(torch_cuda, p), storage=np.float32)
    st = A.stats()
    assert st["alg_bytes"] < st["stored_entries"] * 8  # the value stream is counted in float32
    orc_p = rounded(p, np.float32)
    x = p["x"] if "x" in p else rand_vec(np.random.default_rng(6), p["size"][1], np.float64)
    y0 = np.full(p["size"][0], np.nan)
    got = gpu_mul(torch_cuda, bsm, A, N, x, y0)
    assert relerr(got, oracle_mul(oracle, orc_p, N, x, y0)) <= 1e-13
    y1 = rand_vec(np.random.default_rng(7), p["size"][1], np.float64)
    got = gpu_mul(torch_cuda, bsm, A, T, x[:p["size"][0]], y1, 0.5, 2.0, False)
    assert relerr(got, oracle_mul(oracle, orc_p, T, x[:p["size"][0]], y1, 0.5, 2.0, False)) <= 1e-13


def test_mixed_refused_on_a_context(torch_cuda, bsm):
    """multi-device handles: BSM_ERR_UNSUPPORTED from the C ABI with a real context"""
    import ctypes as C
    from bsm_amd import _lib as L
    from bsm_amd.matrices import Context, SerialScheduler, _options
    o = _options(SerialScheduler(), 0, "auto")
    o.ctx = Context.get([0, 0]).ptr
    blk = np.asfortranarray(np.ones((2, 2)))
    one, two = np.array([1], dtype=np.int64), np.array([2], dtype=np.int64)
    I = C.POINTER(C.c_int64)
    h = C.c_void_p()
    rc = L.lib().bsm_vbcrs_create(L.BSM_F64_F32, 2, 2, 1, (C.c_void_p * 1)(blk.ctypes.data), two.ctypes.data_as(I),
                                  two.ctypes.data_as(I), two.ctypes.data_as(I), one.ctypes.data_as(I),
                                  one.ctypes.data_as(I), C.byref(o), C.byref(h))
    assert rc == -2 and not h.value
