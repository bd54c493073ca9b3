"""GPU suite of block_jacobi: the preconditioner M = sum_s E_s inv(A[I_s, I_s]) E_s^T built on the device (extraction,
batched inverse and construction from device tensors) on the operators of tests/_jacobi.py, its blocks against the dense
ground truth by rho <= 4, its products against the dense product of its own blocks, refresh after new values of A, and
ten steps of the preconditioned Richardson iteration against the same recurrence in numpy."""
import numpy as np
import pytest

from _common import Cc, N, T, rand_vec, relerr
from _ctors import ctor_build
from _gpu import TOL, gpu_mul, gpu_mul_multi, torch_cuda  # noqa: F401
from _jacobi import CODE, KINDS, NOP, RHO_MAX, dense_of, jacobi_problem, rho, set_blocks
from _submat import Truth
from _values import src_list

pytestmark = pytest.mark.gpu

TYPES = [(np.float32, None), (np.float64, None), (np.complex64, None), (np.complex128, None), (np.float64, np.float32)]
TYPE_IDS = [np.dtype(d).name + ("" if s is None else "_as_" + np.dtype(s).name) for d, s in TYPES]
OPS = (N, T, Cc)
LEFT_OUT = 2  # the 7-set is given to no set of M: its rows are zero rows of the preconditioner


def host_blocks(M):
    return [b.cpu().numpy() for b in M.blocks]


def applied(D, op, x, y0, alpha, beta, strong):
    Dop = D if op == N else (D.T if op == T else D.conj().T)
    r = alpha * (Dop @ x)
    return r.astype(y0.dtype) if strong else (r + beta * y0).astype(y0.dtype)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype,storage", TYPES, ids=TYPE_IDS)
def test_blocks_and_products(torch_cuda, bsm, kind, dtype, storage):
    torch = torch_cuda
    rng = np.random.default_rng(2000 + 10 * KINDS.index(kind) + CODE[np.dtype(dtype)])
    p, sets = jacobi_problem(rng, kind, dtype)
    used = sets[:LEFT_OUT] + sets[LEFT_OUT + 1:]
    A, tr = bsm.synthetic.build(p), Truth(p)
    M = bsm.block_jacobi(A, used, **({} if storage is None else {"storage": storage}))
    assert M.device == A.device and M.source is A and all(b.is_cuda for b in M.blocks)
    assert all(np.array_equal(a, b) for a, b in zip(M.sets, used))
    blocks = host_blocks(M)
    worst = 0.0
    for s, (got, want) in enumerate(zip(blocks, set_blocks(tr.D, used))):
        assert got.dtype == np.dtype(dtype) and got.shape == want.shape
        r = rho(got, want)
        worst = max(worst, r)
        assert r <= RHO_MAX, (kind, s, r)
    print(f"INVSTAT block_jacobi device {kind} {TYPE_IDS[TYPES.index((dtype, storage))]} worst rho {worst:.3f}")
    # products against the dense product of M's own blocks (rounded once where M stores them in single precision)
    own = blocks if storage is None else [b.astype(storage).astype(dtype) for b in blocks]
    D = dense_of(own, used, NOP)
    free = sets[LEFT_OUT] - 1
    x, y0 = rand_vec(rng, NOP, dtype), rand_vec(rng, NOP, dtype)
    X, Y0 = np.asfortranarray(np.stack([rand_vec(rng, NOP, dtype) for _ in range(5)], axis=1)), \
        np.asfortranarray(np.stack([rand_vec(rng, NOP, dtype) for _ in range(5)], axis=1))
    for op in OPS:
        for alpha, beta, strong in ((1, 0, True), (-0.5, 1.25, False)):
            ynan = y0.copy()
            if strong:
                ynan[free] = np.nan  # a strong zero: NaN in the rows M does not touch must not survive
            got = gpu_mul(torch, bsm, M, op, x, ynan, alpha, beta, strong)
            want = applied(D, op, x, y0, alpha, beta, strong)
            e = relerr(got, want)
            print(f"  {kind} op {op} alpha {alpha} beta {beta}: {e:.3e}")
            assert e < TOL[np.dtype(dtype)], (kind, op, e)
            assert got[free].tobytes() == (np.zeros(len(free), dtype) if strong else (dtype(beta) * y0[free]).astype(dtype)).tobytes()
            gotm = gpu_mul_multi(torch, bsm, M, op, X, Y0, alpha, beta, strong, pad=3)
            wantm = applied(D, op, X, Y0, alpha, beta, strong)
            em = relerr(gotm.ravel(), wantm.ravel())
            assert em < TOL[np.dtype(dtype)], (kind, op, "multi", em)
            assert gotm[free].tobytes() == (np.zeros((len(free), 5), dtype) if strong else (dtype(beta) * Y0[free]).astype(dtype)).tobytes()
    # transpose(A) gives the transposed inverse blocks
    Mt = bsm.block_jacobi(bsm.transpose(A), used)
    for s, (got, want) in enumerate(zip(host_blocks(Mt), set_blocks(tr.D.T, used))):
        assert rho(got, want) <= RHO_MAX, (kind, s, "transpose")


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_a_real_preconditioner_under_complex_vectors(torch_cuda, bsm, dtype):
    torch = torch_cuda
    rng = np.random.default_rng(2100)
    p, sets = jacobi_problem(rng, "blocksparse", dtype)
    M = bsm.block_jacobi(bsm.synthetic.build(p), sets)
    D = dense_of(host_blocks(M), sets, NOP)
    cdt = np.result_type(dtype, np.complex64)
    x = rand_vec(rng, NOP, cdt)
    for op in OPS:
        got = gpu_mul(torch, bsm, M, op, x, np.zeros(NOP, cdt))
        assert relerr(got, applied(D, op, x, np.zeros(NOP, cdt), 1, 0, True)) < TOL[np.dtype(cdt)], op


@pytest.mark.parametrize("kind", KINDS)
def test_refresh_after_update_blocks(torch_cuda, bsm, kind):
    torch = torch_cuda
    seed = 2200 + KINDS.index(kind)
    p, sets = jacobi_problem(np.random.default_rng(seed), kind, np.float64)
    q, _ = jacobi_problem(np.random.default_rng(seed), kind, np.float64, scale=-0.5)  # the same layout, new values
    first = [b.copy(order="F") for b in src_list(p)]  # (the handle's mirror keeps the caller's arrays: update_blocks edits them)
    A = bsm.synthetic.build(p)
    M = bsm.block_jacobi(A, sets)
    ptrs, nbytes = [b.data_ptr() for b in M.blocks], M.stats()["device_bytes"]
    old = host_blocks(M)
    bsm.update_blocks(A, src_list(q))
    M.refresh()
    assert [b.data_ptr() for b in M.blocks] == ptrs and M.stats()["device_bytes"] == nbytes
    new = host_blocks(M)
    for s, want in enumerate(set_blocks(Truth(q).D, sets)):
        assert rho(new[s], want) <= RHO_MAX, (kind, s)
    assert any(a.tobytes() != b.tobytes() for a, b in zip(old, new))
    # the image follows: a product of M is the product of the new blocks
    x = rand_vec(np.random.default_rng(seed), NOP, np.float64)
    got = gpu_mul(torch, bsm, M, N, x, np.zeros(NOP))
    assert relerr(got, dense_of(new, sets, NOP) @ x) < TOL[np.dtype(np.float64)]
    # back to the first values, on a side stream
    bsm.update_blocks(A, first)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    M.refresh(stream=side)
    side.synchronize()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(old, host_blocks(M)))  # the kernel is deterministic
    # another source of the same size may be named; a storage= M refuses the refill as update_blocks does
    B = bsm.synthetic.build(q)
    M.refresh(B)
    assert M.source is B and all(a.tobytes() == b.tobytes() for a, b in zip(new, host_blocks(M)))
    Ms = bsm.block_jacobi(A, sets, storage=np.float32)
    with pytest.raises(NotImplementedError):
        Ms.refresh()


@pytest.mark.parametrize("kind", KINDS)
def test_a_multi_device_source(torch_cuda, bsm, kind):
    """the blocks of a handle over two (virtual) devices arrive on its first device and M is a single-device handle
    there.  At most two stored values meet anywhere in these operators and a + b = b + a, so the extracted blocks are
    the single-device ones bit for bit (the bound of _submat.accept for such entries) -- and so are their inverses"""
    p, sets = jacobi_problem(np.random.default_rng(2300 + KINDS.index(kind)), kind, np.float64)
    assert Truth(p).Cnt.max() == 2
    one = bsm.block_jacobi(bsm.synthetic.build(p), sets)
    A2 = ctor_build(bsm, kind, p, devices=[0, 0])
    assert len(A2.parts()) == 2
    two = bsm.block_jacobi(A2, sets)
    assert two.devices is None and two.device == 0
    assert all(a.tobytes() == b.tobytes() for a, b in zip(host_blocks(one), host_blocks(two)))


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_ten_preconditioned_richardson_steps(torch_cuda, bsm, dtype):
    """x += M (b - A x) on a symmetric operator whose diagonal blocks dominate (couplings scaled by 1e-3), all on the GPU,
    against the same recurrence in numpy on the dense truth in the same type.  The GPU residual may be twice numpy's plus
    10 n eps |b|, the floor of the recurrence itself"""
    torch = torch_cuda
    rng = np.random.default_rng(2400)
    p, sets = jacobi_problem(rng, "symmetric", dtype)
    p["offdiagonals"] = p["offdiagonals"][:1] + [np.asfortranarray(b * dtype(1e-3)) for b in p["offdiagonals"][1:]]
    D = Truth(p).D
    b = rand_vec(rng, NOP, dtype)
    Minv = dense_of([np.linalg.inv(blk).astype(dtype) for blk in set_blocks(D, sets)], sets, NOP)
    x = np.zeros(NOP, dtype)
    for _ in range(10):
        x = (x + Minv @ (b - D @ x).astype(dtype)).astype(dtype)
    wide = D.astype(np.float64)
    r_np = float(np.max(np.abs(b.astype(np.float64) - wide @ x.astype(np.float64))))
    assert r_np < 1e-3 * float(np.max(np.abs(b)))  # the recurrence converges on this operator
    A = bsm.synthetic.build(p)
    M = bsm.block_jacobi(A)  # the operator's own diagonalindices
    bd = torch.from_numpy(b).cuda()
    xd, rd = torch.zeros_like(bd), torch.empty_like(bd)
    for _ in range(10):
        rd.copy_(bd)
        bsm.mul(rd, A, xd, -1, 1)   # r = b - A x
        bsm.mul(xd, M, rd, 1, 1)    # x += M r
    torch.cuda.synchronize()
    r_gpu = float(np.max(np.abs(b.astype(np.float64) - wide @ xd.cpu().numpy().astype(np.float64))))
    bound = 2 * r_np + 10 * NOP * float(np.finfo(dtype).eps) * float(np.max(np.abs(b)))
    print(f"INVSTAT richardson {np.dtype(dtype).name}: gpu {r_gpu:.3e} numpy {r_np:.3e} bound {bound:.3e}")
    assert r_gpu <= bound, (r_gpu, r_np, bound)
