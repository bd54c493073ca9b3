"""GPU suite (-m gpu): mixed-precision handles (BSM_F64_F32, BSM_C128_C64) -- values stored as float32 / complex64,
x, y, alpha, beta and every sum in float64 / complex128.

    mixed y  vs a pure double-precision handle of the ROUNDED blocks : <= 1e-13 (a sum kept in fp32 would miss by 1e6)
    mixed y  vs the oracle on the ORIGINAL blocks                    : within single-precision rounding (<= 1e-5)
"""
import numpy as np
import pytest

from _common import Cc, N, T, oracle_mul, rand_vec, relerr

pytestmark = pytest.mark.gpu
OPS = [N, T, Cc]
PAIRS = [(np.float64, np.float32), (np.complex128, np.complex64)]
ACCS = ["auto", "atomic", "colored", "gather", "direct"]
CTORS = ["blocksparse", "vbcrs", "symmetric", "vbcrs_from_blocksparse", "vbcrs_from_symmetric"]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    from bsm_amd import _lib as L
    L.lib()
    return torch


def _complexify(blocks, seed):
    rng = np.random.default_rng(seed)
    return [np.asfortranarray(b + 1j * rng.standard_normal(b.shape)) for b in blocks]


def _problem(bsm, ctor, dt, big=False):
    S = bsm.synthetic
    if ctor == "blocksparse":
        p = S.config1(n=600, nblocks=60, bs=16)
        keys = ["blocks"]
    elif ctor == "vbcrs":
        p = S.config2() if big else S.config2(n=4000, nblocks=200, lo=4, hi=48)
        keys = ["blocks"]
    elif ctor == "vbcrs_from_blocksparse":
        v = S.config2(n=3000, nblocks=150, lo=4, hi=48)
        p = dict(kind="blocksparse", blocks=v["blocks"], size=v["size"],
                 rowindices=[np.arange(r, r + b.shape[0], dtype=np.int64) for r, b in zip(v["rowstart"], v["blocks"])],
                 colindices=[np.arange(c, c + b.shape[1], dtype=np.int64) for c, b in zip(v["colstart"], v["blocks"])])
        keys = ["blocks"]
    else:
        p = S.config3() if big else S.config3(nseg=16, bs=24, halfband=2)
        keys = ["diagonals", "offdiagonals"]
    if np.dtype(dt).kind == "c":
        for i, k in enumerate(keys):
            p[k] = _complexify(p[k], 7 + i)
    return p


def _cast(p, dt):
    q = dict(p)
    for k in ("blocks", "diagonals", "offdiagonals"):
        if k in p:
            q[k] = [np.asfortranarray(b.astype(dt)) for b in p[k]]
    return q


def _rounded(p, S):
    return _cast(_cast(p, S), np.result_type(S, np.float64))


def _build(bsm, ctor, p, **kw):
    M = bsm.matrices
    tim = kw.pop("transpose_image", False)
    if ctor == "blocksparse":
        return M.BlockSparseMatrix(p["blocks"], p["rowindices"], p["colindices"], p["size"], transpose_image=tim, **kw)
    if ctor == "vbcrs":
        return M.VariableBlockCompressedRowStorage(p["blocks"], p["rowstart"], p["colstart"], p["size"],
                                                   transpose_image=tim, **kw)
    if ctor == "symmetric":
        return M.SymmetricBlockMatrix(p["diagonals"], p["diagonalindices"], p["offdiagonals"], p["rowindices"],
                                      p["colindices"], p["size"], **kw)
    if ctor == "vbcrs_from_blocksparse":
        B = M.BlockSparseMatrix(p["blocks"], p["rowindices"], p["colindices"], p["size"])
        return M.VariableBlockCompressedRowStorage(B, transpose_image=tim, **kw)
    Sm = M.SymmetricBlockMatrix(p["diagonals"], p["diagonalindices"], p["offdiagonals"], p["rowindices"],
                                p["colindices"], p["size"])
    return M.VariableBlockCompressedRowStorage(Sm, **kw)


def _oracle_problem(ctor, p):
    if ctor == "vbcrs_from_blocksparse":
        return dict(p, kind="blocksparse")
    if ctor == "vbcrs_from_symmetric":
        d, o = p["diagonals"], p["offdiagonals"]
        first = lambda lists: [int(v[0]) for v in lists]  # noqa: E731
        rs = first(p["diagonalindices"]) + first(p["rowindices"]) + first(p["colindices"])
        cs = first(p["diagonalindices"]) + first(p["colindices"]) + first(p["rowindices"])
        return dict(kind="vbcrs", blocks=list(d) + list(o) + [np.asfortranarray(b.T) for b in o],
                    rowstart=np.array(rs, dtype=np.int64), colstart=np.array(cs, dtype=np.int64), size=p["size"])
    return p


def _wrap(bsm, A, op):
    return A if op == N else (bsm.transpose(A) if op == T else bsm.adjoint(A))


def _gpu(torch, bsm, A, op, x, y0, alpha=1, beta=0, strong=True):
    xd = torch.from_numpy(x).cuda()
    yd = torch.from_numpy(np.array(y0, copy=True)).cuda()
    bsm.mul(yd, _wrap(bsm, A, op), xd, alpha, False if strong else beta)
    torch.cuda.synchronize()
    return yd.cpu().numpy()


# (transpose_image applies to VBCRS / BlockSparseMatrix operators without symmetric pieces)
CTOR_TIMAGE = [(c, t) for c in CTORS for t in (0, 1) if t == 0 or c not in ("symmetric", "vbcrs_from_symmetric")]


@pytest.mark.parametrize("acc", ACCS)
@pytest.mark.parametrize("T_, S_", PAIRS)
@pytest.mark.parametrize("ctor, timage", CTOR_TIMAGE)
def test_mixed_product_matrix(torch_cuda, bsm, oracle, ctor, timage, T_, S_, acc):
    p = _problem(bsm, ctor, T_)
    A = _build(bsm, ctor, p, storage=S_, accumulate=acc, transpose_image=timage)
    R = _build(bsm, ctor, _rounded(p, S_), accumulate=acc, transpose_image=timage)  # pure T, rounded blocks
    rng = np.random.default_rng(1)
    nr, nc = p["size"]
    for op in OPS:
        xl, yl = (nc, nr) if op == N else (nr, nc)
        x = rand_vec(rng, xl, T_)
        y0 = rand_vec(rng, yl, T_)
        for alpha, beta, strong in ((1, 0, True), (0.5, 2.0, False)):
            got = _gpu(torch_cuda, bsm, A, op, x, y0, alpha, beta, strong)
            ref = _gpu(torch_cuda, bsm, R, op, x, y0, alpha, beta, strong)
            assert relerr(got, ref) <= 1e-13, (op, alpha, beta)
        orc = oracle_mul(oracle, _oracle_problem(ctor, p), op, x, y0)
        assert relerr(_gpu(torch_cuda, bsm, A, op, x, y0), orc) <= 1e-5
        # bitwise reproducible run to run: coloured and gather products always, DIRECT where it takes the exclusive
        # stores (op N of a conflict-free operator; otherwise it is the atomic path, like AUTO)
        if acc in ("colored", "gather") or (acc == "direct" and op == N and A.stats()["exclusive"] == 1):
            a = _gpu(torch_cuda, bsm, A, op, x, y0, 0.5, 2.0, False)
            b = _gpu(torch_cuda, bsm, A, op, x, y0, 0.5, 2.0, False)
            assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("T_, S_", PAIRS)
@pytest.mark.parametrize("ctor", ["vbcrs", "symmetric"])
def test_mixed_alpha_beta_strong_zero_nan(torch_cuda, bsm, oracle, ctor, T_, S_):
    p = _problem(bsm, ctor, T_)
    A = _build(bsm, ctor, p, storage=S_)
    orc_p = _oracle_problem(ctor, _rounded(p, S_))
    rng = np.random.default_rng(2)
    n = p["size"][0]
    x = rand_vec(rng, n, T_)
    ynan = np.full(n, np.nan, dtype=T_)
    cplx = np.dtype(T_).kind == "c"
    alpha = 0.5 - 0.25j if cplx else -0.75
    for op in OPS:
        got = _gpu(torch_cuda, bsm, A, op, x, ynan, alpha, 0, True)  # strong zero: the NaN must not propagate
        assert np.all(np.isfinite(got))
        assert relerr(got, oracle_mul(oracle, orc_p, op, x, ynan, alpha, 0, True)) <= 1e-13
        got = _gpu(torch_cuda, bsm, A, op, x, ynan, alpha, 0.0, False)  # numeric zero multiplies: NaN stays
        assert np.all(np.isnan(got))
        y0 = rand_vec(rng, n, T_)
        beta = 1.5 + 0.5j if cplx else 1.5
        got = _gpu(torch_cuda, bsm, A, op, x, y0, alpha, beta, False)
        assert relerr(got, oracle_mul(oracle, orc_p, op, x, y0, alpha, beta, False)) <= 1e-13


def _device_blocks(torch, p):
    q = dict(p)
    for k in ("blocks", "diagonals", "offdiagonals"):
        if k in p:  # column-major CUDA tensors
            q[k] = [torch.from_numpy(np.ascontiguousarray(b.T)).cuda().t() for b in p[k]]
    return q


@pytest.mark.parametrize("T_, S_", PAIRS)
@pytest.mark.parametrize("ctor", CTORS)
def test_mixed_rowcolvals_host_and_device_blocks(torch_cuda, bsm, ctor, T_, S_):
    p = _problem(bsm, ctor, T_)
    if np.dtype(T_) == np.float64:  # subnormal, overflowing and tie-breaking entries round alike on both packers
        key = "blocks" if "blocks" in p else "offdiagonals"
        b = p[key][0].copy(order="F")
        b.flat[:6] = [1e-40, -3e-42, 1e39, 1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24, 2.0 ** -149]
        p[key] = [b] + list(p[key][1:])
    Ah = _build(bsm, ctor, p, storage=S_)
    Ad = _build(bsm, ctor, _device_blocks(torch_cuda, p), storage=S_)
    rh, ch, vh = (t.cpu().numpy() for t in bsm.rowcolvals_device(Ah))
    rd, cd, vd = (t.cpu().numpy() for t in bsm.rowcolvals_device(Ad))
    assert vh.dtype == np.dtype(T_)
    assert np.array_equal(rh, rd) and np.array_equal(ch, cd) and vh.tobytes() == vd.tobytes()
    # exactly astype(S).astype(T) of the pure single-precision handle's values
    with np.errstate(over="ignore"):
        As = _build(bsm, ctor, _cast(p, S_))
    rs, cs, vs = (t.cpu().numpy() for t in bsm.rowcolvals_device(As))
    assert np.array_equal(rh, rs) and np.array_equal(ch, cs)
    assert vh.tobytes() == vs.astype(T_).tobytes()


@pytest.mark.parametrize("T_, S_", PAIRS)
@pytest.mark.parametrize("ctor", ["vbcrs", "symmetric", "blocksparse"])
def test_mixed_mul_multi_is_column_by_column(torch_cuda, bsm, ctor, T_, S_):
    torch = torch_cuda
    p = _problem(bsm, ctor, T_)
    A = _build(bsm, ctor, p, storage=S_, accumulate="colored")
    n, k = p["size"][0], 5
    rng = np.random.default_rng(4)
    X = np.stack([rand_vec(rng, n, T_) for _ in range(k)], axis=1)
    for op in OPS:
        Xd = torch.from_numpy(np.ascontiguousarray(X.T)).cuda().t()
        Yd = torch.zeros((k, n), dtype=Xd.dtype, device="cuda").t()
        bsm.mul(Yd, _wrap(bsm, A, op), Xd)
        torch.cuda.synchronize()
        Y = Yd.cpu().numpy()
        for j in range(k):
            col = _gpu(torch, bsm, A, op, X[:, j].copy(), np.zeros(n, T_))
            assert Y[:, j].tobytes() == col.tobytes(), (op, j)


@pytest.mark.parametrize("T_, S_", PAIRS)
def test_mixed_graph_replay(torch_cuda, bsm, T_, S_):
    torch = torch_cuda
    p = _problem(bsm, "symmetric", T_)
    A = _build(bsm, "symmetric", p, storage=S_, accumulate="colored")
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
    p = _problem(bsm, ctor, np.float64, big=True)
    A = _build(bsm, ctor, _device_blocks(torch_cuda, p), storage=np.float32)
    st = A.stats()
    assert st["alg_bytes"] < st["stored_entries"] * 8  # the value stream is counted in float32
    orc_p = _rounded(p, np.float32)
    x = p["x"] if "x" in p else rand_vec(np.random.default_rng(6), p["size"][1], np.float64)
    y0 = np.full(p["size"][0], np.nan)
    got = _gpu(torch_cuda, bsm, A, N, x, y0)
    assert relerr(got, oracle_mul(oracle, orc_p, N, x, y0)) <= 1e-13
    y1 = rand_vec(np.random.default_rng(7), p["size"][1], np.float64)
    got = _gpu(torch_cuda, bsm, A, T, x[:p["size"][0]], y1, 0.5, 2.0, False)
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
