"""Device helpers shared by the GPU suites: the `torch_cuda` and `env` fixtures (imported by name into a test module),
the tolerance table, column-major device copies (`dev_copy`, `dev_vec`, `dev_mat` with NaN padding, `outside_bytes`),
`scatter` for partitioned vectors, the two product drivers `gpu_mul` (one column) and `gpu_mul_multi` (several), and the
byte and pass-count checks of the handle suites (`same_products`, `passes_of_one_product`, `same_bytes`).
`torch` is an argument wherever a helper needs it, so that this module imports without it.  Test code only."""
import numpy as np
import pytest

from _common import wrap

# max|got - ref| / max|ref| of a product against the CPU oracle, by vector type
TOL = {np.dtype(np.float64): 1e-12, np.dtype(np.complex128): 1e-12, np.dtype(np.float32): 1e-5, np.dtype(np.complex64): 1e-5}


def _torch_with_library():
    import torch
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    from bsm_amd import _lib as L
    L.lib()  # fails loudly if the HIP extension is missing
    return torch


@pytest.fixture(scope="module")
def torch_cuda():
    return _torch_with_library()


@pytest.fixture(scope="module")
def env():
    """(torch, bsm, oracle)"""
    torch = _torch_with_library()
    import bsm_amd as bsm
    from oracle import load_oracle
    return torch, bsm, load_oracle()


def torch_dtype(torch, dt):
    return torch.from_numpy(np.zeros(1, dtype=dt)).dtype


def dev_copy(torch, b):
    """column-major CUDA copy of a matrix"""
    return torch.from_numpy(np.ascontiguousarray(b.T)).cuda().t()


def scatter(torch, v, ranges):
    """v cut by 1-based inclusive ranges into CUDA tensors (None for an empty range)"""
    return [torch.from_numpy(np.ascontiguousarray(v[lo - 1:hi])).cuda() if hi >= lo else None for lo, hi in ranges]


def dev_vec(torch, v, off=0, guard=0):
    """v as a contiguous view `off` elements into a NaN-filled device buffer with `guard` elements behind -> (buffer, view)"""
    buf = torch.full((off + len(v) + guard,), float("nan"), dtype=torch_dtype(torch, v.dtype), device="cuda")
    buf[off:off + len(v)] = torch.from_numpy(np.ascontiguousarray(v)).cuda()
    return buf, buf[off:off + len(v)]


def dev_mat(torch, M, pad=0, off=0, guard=0):
    """M as a column-major view with leading dimension rows + pad, `off` elements into a NaN-filled device buffer with
    `guard` elements behind -> (buffer, view)"""
    n, k = M.shape
    ld = n + pad
    buf = torch.full((off + k * ld + guard,), float("nan"), dtype=torch_dtype(torch, M.dtype), device="cuda")
    body = buf[off:off + k * ld].view(k, ld)
    body[:, :n] = torch.from_numpy(np.ascontiguousarray(M.T)).cuda()
    return buf, body[:, :n].t()


def outside_bytes(buf, n, ld, k, off=0):
    """the bytes of a dev_vec / dev_mat buffer outside the n x k matrix (leading dimension ld) that starts `off` elements
    into it: pad rows and guard elements"""
    a = buf.cpu().numpy()
    keep = np.ones(len(a), dtype=bool)
    for j in range(k):
        keep[off + j * ld:off + j * ld + n] = False
    return a[keep].tobytes()


def gpu_mul(torch, bsm, A, op, x, y0, alpha=1, beta=0, strong=True, host=False):
    """y = alpha op(A) x + beta y0 (strong: beta is the strong zero) through bsm.mul on copies of x and y0 -- uploaded to
    the GPU (x may be a non-contiguous view), or as host vectors, which the library stages itself"""
    Aop = wrap(bsm, A, op)
    if host:
        y = np.array(y0, copy=True)
        if strong:
            return bsm.mul(y, Aop, x) if alpha == 1 else bsm.mul(y, Aop, x, alpha, False)
        return bsm.mul(y, Aop, x, alpha, beta)
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    yd = torch.from_numpy(np.array(y0, copy=True)).cuda()
    bsm.mul(yd, Aop, xd, alpha, False if strong else beta)
    torch.cuda.synchronize()
    return yd.cpu().numpy()


def gpu_mul_multi(torch, bsm, A, op, X, Y0, alpha=1, beta=0, strong=True, pad=0):
    """Y = alpha op(A) X + beta Y0 through ONE bsm.mul on column-major device copies with leading dimension rows + pad;
    the padding of X and Y must come back bit-identical"""
    xb, xv = dev_mat(torch, X, pad)
    yb, yv = dev_mat(torch, Y0, pad)
    (xl, k), yl = X.shape, Y0.shape[0]
    before = (outside_bytes(xb, xl, xl + pad, k), outside_bytes(yb, yl, yl + pad, k))
    bsm.mul(yv, wrap(bsm, A, op), xv, alpha, False if strong else beta)
    torch.cuda.synchronize()
    assert (outside_bytes(xb, xl, xl + pad, k), outside_bytes(yb, yl, yl + pad, k)) == before, "padding of X / Y was written"
    return yv.cpu().numpy()


# ---- what the solver-on-every-handle suites (test_gpu_solver_handles.py, test_gpu_lsqr_handles.py) share ------------------
def result_like(torch, bsm, H, x):
    """an uninitialised device vector / column-major matrix for op(H) x: the rows of op(H) (those of x where it is square), the
    columns and the type of x"""
    rows = bsm.size(H)[0]
    return torch.empty((x.shape[1], rows), dtype=x.dtype, device="cuda").t() if x.dim() == 2 else torch.empty(rows, dtype=x.dtype, device="cuda")


def same_products(torch, bsm, Bd, *ops):
    """two products of every handle give the same bytes (as test_freezing_holds asserts before it compares solves)"""
    x = Bd[:, 0] if Bd.shape[1] == 1 else Bd
    for H in ops:
        y1, y2 = (result_like(torch, bsm, H, x) for _ in range(2))
        bsm.mul(y1, H, x)
        bsm.mul(y2, H, x)
        torch.cuda.synchronize()
        assert y1.cpu().numpy().tobytes() == y2.cpu().numpy().tobytes(), "the products of this handle are not reproducible"


def passes_of_one_product(torch, bsm, H, Hop, Bd):
    """what one plain product of op(H) (Hop: H or its wrapper) of Bd's width adds to H.value_passes()"""
    x = Bd[:, 0] if Bd.shape[1] == 1 else Bd
    y = result_like(torch, bsm, Hop, x)
    before = H.value_passes()
    bsm.mul(y, Hop, x)
    torch.cuda.synchronize()
    return H.value_passes() - before


def same_bytes(a, b, what):
    (xa, ia), (xb, ib) = a, b
    assert xa.cpu().numpy().tobytes() == xb.cpu().numpy().tobytes(), (what, "X differs")
    assert np.asarray(ia.history).tobytes() == np.asarray(ib.history).tobytes(), (what, "the history differs")
