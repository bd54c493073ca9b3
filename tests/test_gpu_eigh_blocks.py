"""GPU suite of bsm_eigh_blocks / bsm_spectral_blocks with BSM_MEM_DEVICE: eigh_kernel (csrc/bsm_eigh.hip) in both of its
regimes -- A and V resident in LDS, and rotated in device memory -- and at the seam between them in ONE launch per type, in
NaN-padded buffers, against the figures of tests/_eigh.py (rho <= 4, the twin <= 1 on the same inputs: test_eigh_blocks_cpu.py);
run-to-run bit-identity, the sweep counts, the info convention, the size limit, streams; spectral_kernel against the fma bound."""
import numpy as np
import pytest

from _eigh import (CODE, DTYPES, FUNC, RHO_MAX, batch, check_spectral, eigh_seam, f_of, figures, matrix, raw_eigh, raw_spectral, real_of,
                   spectral_seam, wide_of)
from _gpu import dev_copy, dev_mat, dev_vec, outside_bytes, torch_cuda  # noqa: F401
from _jacobi import uniform

pytestmark = pytest.mark.gpu

IDS = [np.dtype(d).name for d in DTYPES]
PAD, OFF, GUARD = 3, 2, 4


def device_run(torch, bsm, dtype, blocks, vectors=1, stream=None):
    """one bsm_eigh_blocks call on NaN-padded device copies of the blocks, w in NaN-guarded device vectors -> (info, sweeps, w,
    blocks afterwards); every byte outside the n x n windows and the n entries of w must come back unchanged"""
    real = real_of(dtype)
    arrs = [dev_mat(torch, b, PAD, OFF, GUARD) for b in blocks]
    ws = [dev_vec(torch, np.zeros(b.shape[0], real), 1, 2) for b in blocks]
    before = [outside_bytes(buf, b.shape[0], b.shape[0] + PAD, b.shape[0], OFF) for (buf, _), b in zip(arrs, blocks)]
    wbefore = [outside_bytes(buf, b.shape[0], b.shape[0], 1, 1) for (buf, _), b in zip(ws, blocks)]
    ns = [b.shape[0] for b in blocks]
    st = torch.cuda.current_stream().cuda_stream if stream is None else stream
    rc, info, sweeps = raw_eigh(CODE[np.dtype(dtype)], [v.data_ptr() if v.numel() else None for _, v in arrs], ns, [n + PAD for n in ns],
                                [v.data_ptr() if v.numel() else None for _, v in ws], vectors=vectors, memspace=1, stream=st)
    assert rc == 0, bsm._lib.lib().bsm_last_error()
    assert [outside_bytes(buf, b.shape[0], b.shape[0] + PAD, b.shape[0], OFF) for (buf, _), b in zip(arrs, blocks)] == before, \
        "a byte outside a window was written"
    assert [outside_bytes(buf, b.shape[0], b.shape[0], 1, 1) for (buf, _), b in zip(ws, blocks)] == wbefore, "a byte outside w was written"
    return info, sweeps, [v.cpu().numpy() for _, v in ws], [v.cpu().numpy() for _, v in arrs]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_both_regimes_and_their_seam_in_one_launch(torch_cuda, bsm, dtype):
    torch = torch_cuda
    blocks = [b for _, b in batch(dtype)]
    s = eigh_seam(dtype)
    assert [b.shape[0] for b in blocks[-2:]] == [s, s + 1] and s == {4: 128, 8: 90, 16: 64}[np.dtype(dtype).itemsize]
    info, sweeps, W, X = device_run(torch, bsm, dtype, blocks)
    assert not info.any(), info
    worst = [0.0, 0.0, 0.0]
    for (cls, b), w, x, sw in zip(batch(dtype), W, X, sweeps):
        f = figures(b, w, x)
        print(f"  device {np.dtype(dtype).name} {cls} n {b.shape[0]}: {sw} sweeps, rho_w {f[0]:.3f} rho_r {f[1]:.3f} rho_o {f[2]:.3f}")
        assert max(f) <= RHO_MAX, (cls, b.shape[0], f)
        assert np.all(np.diff(w) >= 0) and 0 <= sw <= 20, (cls, b.shape[0], sw)
        worst = [max(a, c) for a, c in zip(worst, f)]
    print(f"EIGHSTAT device {np.dtype(dtype).name} worst rho_w {worst[0]:.3f} rho_r {worst[1]:.3f} rho_o {worst[2]:.3f}, most sweeps {sweeps.max()}")
    # a second run on fresh copies: a fixed order of rotations and one writer per entry leave no room for another bit
    info2, sweeps2, W2, X2 = device_run(torch, bsm, dtype, blocks)
    assert not info2.any() and sweeps2.tolist() == sweeps.tolist()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(W, W2)) and all(a.tobytes() == b.tobytes() for a, b in zip(X, X2))
    # vectors = 0: the same eigenvalues to the bit
    info3, sweeps3, W3, _ = device_run(torch, bsm, dtype, blocks, vectors=0)
    assert not info3.any() and sweeps3.tolist() == sweeps.tolist() and all(a.tobytes() == b.tobytes() for a, b in zip(W, W3))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_info_1_spares_the_neighbours(torch_cuda, bsm, dtype):
    torch = torch_cuda
    rng = np.random.default_rng(3900)
    big = eigh_seam(dtype) + 1
    good = [matrix(rng, "uniform", n, dtype) for n in (7, 9, 65, big)]
    nan = matrix(rng, "uniform", 9, dtype)
    nan[3, 4] = np.nan
    bignan = matrix(rng, "uniform", big, dtype)  # the same in the device-memory regime
    bignan[big - 3, 11] = np.inf
    given = [good[0], nan, good[1], bignan, good[2], good[3]]
    info, sweeps, W, X = device_run(torch, bsm, dtype, given)
    assert info.tolist() == [0, 1, 0, 1, 0, 0], info
    for k in (1, 3):
        assert X[k].tobytes() == np.ascontiguousarray(given[k]).tobytes() or np.array_equal(X[k], given[k], equal_nan=True)
        assert np.all(np.isnan(W[k])) and sweeps[k] == 0
    for k in (0, 2, 4, 5):
        assert max(figures(given[k], W[k], X[k])) <= RHO_MAX, k


def test_the_largest_order_and_the_first_refused_one(torch_cuda, bsm):
    torch = torch_cuda
    b = matrix(np.random.default_rng(3910), "uniform", 512, np.float32)
    info, sweeps, (w,), (x,) = device_run(torch, bsm, np.float32, [b])
    f = figures(b, w, x)
    print(f"EIGHSTAT device float32 n 512: {sweeps[0]} sweeps, rho_w {f[0]:.3f} rho_r {f[1]:.3f} rho_o {f[2]:.3f}")
    assert info[0] == 0 and max(f) <= RHO_MAX and sweeps[0] <= 20, (info, f, sweeps)
    buf = torch.full((513 * 513,), float("nan"), dtype=torch.float32, device="cuda")
    small = torch.eye(3, dtype=torch.float32, device="cuda") * 2
    wb = torch.full((513 + 3,), 5.0, dtype=torch.float32, device="cuda")
    rc, info, sweeps = raw_eigh(0, [small.data_ptr(), buf.data_ptr()], [3, 513], [3, 513], [wb.data_ptr(), wb.data_ptr() + 12], memspace=1)
    torch.cuda.synchronize()
    assert rc == -2 and np.all(info == -77) and np.all(sweeps == -77)  # BSM_ERR_UNSUPPORTED, nothing written
    assert bool(torch.isnan(buf).all()) and bool((wb == 5.0).all())
    assert small.cpu().numpy().tobytes() == (np.eye(3, dtype=np.float32) * 2).tobytes()


@pytest.mark.parametrize("dtype", [np.float64, np.complex64], ids=["float64", "complex64"])
def test_the_python_entries_on_tensors_and_a_side_stream(torch_cuda, bsm, dtype):
    torch = torch_cuda
    rng = np.random.default_rng(3920)
    B = [matrix(rng, "uniform", n, dtype) for n in (0, 1, 33, 64, 100)]
    ref = [dev_copy(torch, b) for b in B]
    w, info = bsm.eigh_blocks(ref)  # torch's current (default) stream
    assert info.tolist() == [0] * len(B) and all(x.is_cuda and x.dim() == 1 and len(x) == b.shape[0] for x, b in zip(w, B))
    assert w[0].dtype == torch.float64 if dtype == np.float64 else w[0].dtype == torch.float32
    side = torch.cuda.Stream()
    T1 = [dev_copy(torch, b) for b in B]
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        w1, info1, sweeps1 = bsm.eigh_blocks(T1, sweeps=True)  # torch's current stream is the side stream
        out1, sinfo1 = bsm.spectral_blocks(T1, w1, func="absinv")
    assert not info1.any() and not sinfo1.any() and sweeps1.max() <= 20
    info2, _, W2, X2 = device_run(torch, bsm, dtype, B, stream=side.cuda_stream)
    assert not info2.any()
    for a, b, c, d, x, y, src, o in zip(ref, T1, X2, W2, w, w1, B, out1):
        assert max(figures(src, x.cpu().numpy(), a.cpu().numpy())) <= RHO_MAX
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() == np.ascontiguousarray(c).tobytes()
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes() == d.tobytes()
        check_spectral(o.cpu().numpy(), b.cpu().numpy(), f_of(y.cpu().numpy(), "absinv", 0.0).astype(real_of(dtype)), "absinv")
    with pytest.raises(TypeError):
        bsm.eigh_blocks([torch.zeros(3, 3, dtype=torch.float64, device="cuda"), torch.zeros(2, 2, dtype=torch.float32, device="cuda").t()])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_spectral_blocks_at_both_sides_of_its_seam(torch_cuda, bsm, dtype):
    torch = torch_cuda
    rng = np.random.default_rng(3930 + CODE[np.dtype(dtype)])
    real, code = real_of(dtype), CODE[np.dtype(dtype)]
    s = spectral_seam(dtype)
    ns = (0, 1, 3, 17, s, s + 1)
    st = torch.cuda.current_stream().cuda_stream

    def run(V, w, func, rcond):
        outs = [dev_mat(torch, np.zeros((n, n), dtype), PAD, OFF, GUARD) for n in ns]
        before = [outside_bytes(buf, n, n + PAD, n, OFF) for (buf, _), n in zip(outs, ns)]
        dV, dw = [dev_mat(torch, v, 1, 1, 1) for v in V], [dev_vec(torch, x, 1, 1) for x in w]
        rc, info = raw_spectral(code, [v.data_ptr() if v.numel() else None for _, v in dV], ns, [n + 1 for n in ns],
                                [x.data_ptr() if x.numel() else None for _, x in dw], FUNC[func], rcond,
                                [o.data_ptr() if o.numel() else None for _, o in outs], [n + PAD for n in ns], memspace=1, stream=st)
        assert rc == 0 and not info.any(), (bsm._lib.lib().bsm_last_error(), info)
        assert [outside_bytes(buf, n, n + PAD, n, OFF) for (buf, _), n in zip(outs, ns)] == before, "a byte outside a window was written"
        return [o.cpu().numpy() for _, o in outs]

    # exact on integer data
    V = [np.asfortranarray(rng.integers(-3, 4, (n, n)).astype(dtype)) for n in ns]
    if np.dtype(dtype).kind == "c":
        V = [np.asfortranarray(v + 1j * rng.integers(-3, 4, v.shape)).astype(dtype) for v in V]
    w = [rng.integers(-4, 5, n).astype(real) for n in ns]
    for v, x, o in zip(V, w, run(V, w, "values", 0.0)):
        want = (v.astype(wide_of(dtype)) * x[None, :].astype(np.float64)) @ v.astype(wide_of(dtype)).conj().T
        assert np.array_equal(o.astype(want.dtype), want), v.shape
    # random data: the fma bound, Hermitian to the bit, the same bytes from run to run
    V = [np.asfortranarray(uniform(rng, (n, n), dtype)) for n in ns]
    w = [rng.uniform(-2, 2, n).astype(real) for n in ns]
    for func in ("inv", "absinv", "pinv"):
        got, again = run(V, w, func, 0.25), run(V, w, func, 0.25)
        for v, x, o, o2, n in zip(V, w, got, again, ns):
            worst = check_spectral(o, v, f_of(x, func, 0.25).astype(real), (func, n))
            assert o.tobytes() == o2.tobytes()
            print(f"  spectral device {np.dtype(dtype).name} {func} n {n}: worst error / bound {worst:.3f}")
    # info names the first bad eigenvalue and spares the neighbours (one block per regime)
    bad = [x.copy() for x in w]
    bad[3][5] = 0
    bad[5][7] = np.nan
    bad[5][9] = 0
    outs = [dev_mat(torch, np.full((n, n), 7, dtype), 0, 0, 0) for n in ns]
    dV, dw = [dev_copy(torch, v) for v in V], [dev_vec(torch, x)[1] for x in bad]
    rc, info = raw_spectral(code, [v.data_ptr() if v.numel() else None for v in dV], ns, [max(n, 1) for n in ns],
                            [x.data_ptr() if x.numel() else None for x in dw], FUNC["inv"], 0.0,
                            [o.data_ptr() if o.numel() else None for _, o in outs], [max(n, 1) for n in ns], memspace=1, stream=st)
    assert rc == 0 and info.tolist() == [0, 0, 0, 6, 0, 8], info
    assert bool((outs[3][1] == 7).all()) and bool((outs[5][1] == 7).all())
    check_spectral(outs[4][1].cpu().numpy(), V[4], f_of(w[4], "inv", 0.0).astype(real), "neighbour")
