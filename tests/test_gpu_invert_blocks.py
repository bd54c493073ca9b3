"""GPU suite of bsm_invert_blocks with BSM_MEM_DEVICE: invert_kernel (csrc/bsm_invert.hip) in both of its regimes -- blocks
eliminated in LDS and blocks eliminated in place -- and at the seam between them, in NaN-padded buffers, against the
accuracy bound of tests/_jacobi.py (rho <= 4); run-to-run bit-identity, the info convention, the size limit and streams."""
import numpy as np
import pytest

from _gpu import dev_mat, outside_bytes, torch_cuda  # noqa: F401
from _jacobi import CODE, DTYPES, RHO_MAX, SIZES, good_block, raw_invert, rho

pytestmark = pytest.mark.gpu

IDS = [np.dtype(d).name for d in DTYPES]
PAD, OFF, GUARD = 3, 2, 4


def seam(bsm, dtype):
    """largest order whose n * n * sizeof(T) fits BSM_INVERT_LDS_BYTES: eliminated in LDS, seam + 1 in place"""
    n = int(np.sqrt(bsm._lib.BSM_INVERT_LDS_BYTES // np.dtype(dtype).itemsize))
    assert n * n * np.dtype(dtype).itemsize <= bsm._lib.BSM_INVERT_LDS_BYTES < (n + 1) ** 2 * np.dtype(dtype).itemsize
    return n


def device_run(torch, bsm, dtype, blocks, stream=None):
    """one bsm_invert_blocks call on NaN-padded device copies of the blocks -> (info, results); every byte outside the
    n x n windows must come back unchanged"""
    arrs = [dev_mat(torch, b, PAD, OFF, GUARD) for b in blocks]
    before = [outside_bytes(buf, b.shape[0], b.shape[0] + PAD, b.shape[0], OFF) for (buf, _), b in zip(arrs, blocks)]
    ptrs = [v.data_ptr() if v.numel() else None for _, v in arrs]
    ns = [b.shape[0] for b in blocks]
    st = torch.cuda.current_stream().cuda_stream if stream is None else stream
    rc, info = raw_invert(CODE[np.dtype(dtype)], ptrs, ns, [n + PAD for n in ns], memspace=1, stream=st)
    assert rc == 0, bsm._lib.lib().bsm_last_error()
    after = [outside_bytes(buf, b.shape[0], b.shape[0] + PAD, b.shape[0], OFF) for (buf, _), b in zip(arrs, blocks)]
    assert after == before, "a byte outside a window was written"
    return info, [v.cpu().numpy() for _, v in arrs]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_both_regimes_and_their_seam_in_padded_buffers(torch_cuda, bsm, dtype):
    torch = torch_cuda
    rng = np.random.default_rng(1900 + CODE[np.dtype(dtype)])
    s = seam(bsm, dtype)
    sizes = (0,) + SIZES + (s - 1, s, s + 1)
    assert min(n for n in sizes if n) ** 2 * np.dtype(dtype).itemsize < bsm._lib.BSM_INVERT_LDS_BYTES < max(sizes) ** 2 * np.dtype(dtype).itemsize
    B = [good_block(rng, n, dtype) for n in sizes]
    info, X = device_run(torch, bsm, dtype, B)
    assert not info.any(), info
    worst = 0.0
    for x, b in zip(X, B):
        r = rho(x, b)
        print(f"  device {np.dtype(dtype).name} n {b.shape[0]}: rho {r:.3f}")
        worst = max(worst, r)
        assert r <= RHO_MAX, (b.shape[0], r)
    print(f"INVSTAT device {np.dtype(dtype).name} worst rho {worst:.3f}")
    # a second run on fresh copies: a fixed pivot rule and a fixed update order leave no room for another bit
    info2, X2 = device_run(torch, bsm, dtype, B)
    assert not info2.any() and all(a.tobytes() == b.tobytes() for a, b in zip(X, X2))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_info_names_the_step_and_spares_the_neighbours(torch_cuda, bsm, dtype):
    torch = torch_cuda
    rng = np.random.default_rng(1920)
    n, big = 9, seam(bsm, dtype) + 1
    good = [good_block(rng, k, dtype) for k in (7, n, 65, big)]
    zero = np.zeros((n, n), dtype=dtype, order="F")
    dup = good_block(rng, n, dtype)
    dup[5] = dup[2]
    nan = good_block(rng, n, dtype)
    nan[3, 4] = np.nan
    bigdup = good_block(rng, big, dtype)  # the same in the in-place regime
    bigdup[big - 3] = bigdup[11]
    batch = [good[0], zero, good[1], dup, nan, good[2], bigdup, good[3]]
    info, X = device_run(torch, bsm, dtype, batch)
    assert info[1] == 1, info
    assert 1 <= info[3] <= n, info
    assert info[4] != 0, info
    assert 1 <= info[6] <= big, info
    for k in (0, 2, 5, 7):
        assert info[k] == 0 and rho(X[k], batch[k]) <= RHO_MAX, (k, info)


def test_the_largest_order_and_the_first_refused_one(torch_cuda, bsm):
    torch = torch_cuda
    rng = np.random.default_rng(1930)
    b = good_block(rng, 1024, np.float32)
    info, (x,) = device_run(torch, bsm, np.float32, [b])
    r = rho(x, b)
    print(f"INVSTAT device float32 n 1024: rho {r:.3f}")
    assert info[0] == 0 and r <= RHO_MAX, (info, r)
    buf = torch.full((1025 * 1025,), float("nan"), dtype=torch.float32, device="cuda")
    small = torch.eye(3, dtype=torch.float32, device="cuda") * 2
    rc, info = raw_invert(0, [small.data_ptr(), buf.data_ptr()], [3, 1025], [3, 1025], memspace=1, stream=None)
    torch.cuda.synchronize()
    assert rc == -2 and np.all(info == -77)  # BSM_ERR_UNSUPPORTED, nothing written
    assert bool(torch.isnan(buf).all()) and small.cpu().numpy().tobytes() == (np.eye(3, dtype=np.float32) * 2).tobytes()


@pytest.mark.parametrize("dtype", [np.float64, np.complex64], ids=["float64", "complex64"])
def test_the_python_entry_on_tensors_and_a_side_stream(torch_cuda, bsm, dtype):
    torch = torch_cuda
    rng = np.random.default_rng(1940)
    B = [good_block(rng, n, dtype) for n in (0, 1, 33, 64, 150)]
    ref = [torch.from_numpy(np.ascontiguousarray(b.T)).cuda().t() for b in B]
    assert bsm.invert_blocks(ref).tolist() == [0] * len(B)  # torch's current (default) stream
    side = torch.cuda.Stream()
    T1 = [torch.from_numpy(np.ascontiguousarray(b.T)).cuda().t() for b in B]
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        assert not bsm.invert_blocks(T1).any()      # torch's current stream is the side stream
    info, raw = device_run(torch, bsm, dtype, B, stream=side.cuda_stream)
    assert not info.any()
    for a, b, d, src in zip(ref, T1, raw, B):
        assert rho(a.cpu().numpy(), src) <= RHO_MAX
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() == np.ascontiguousarray(d).tobytes()
    with pytest.raises(TypeError):
        bsm.invert_blocks([torch.zeros(3, 3, dtype=torch.float64, device="cuda"), torch.zeros(2, 2, dtype=torch.float32, device="cuda").t()])
