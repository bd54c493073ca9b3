"""GPU suite of bsm_krylov_orth, one classical Gram-Schmidt pass  h = V^H w,  w -= V h,  hsum += h,  nrm = ||w||  at the
smallest shapes where the kernels can go wrong: n around the wave (64) and the workgroup (256), one that is no multiple of
anything (1000) and one that spans many workgroups and the second reduction stage (70 001); k around the column batch
and the bound; leading dimensions and start addresses that take the 16-byte path, its head and tail, and the
element-by-element path.

Bounds (none of them measured):
  h    per column |h - h_wide| <= c n eps(T) (|V|^H |w|), c = 1 real, 2 complex: the bound of a dot product of n terms
       in ANY summation order (each complex product is four real ones);
  w'   per entry |w' - (w - V h)| <= c (k + 2) eps(T) (|w| + |V| |h|) with the RETURNED h on the right-hand side (so no
       error of h propagates): k FMAs into one accumulator;
  nrm  within max(n, 1) eps(T) relative of ||w'|| of the returned w';
everything evaluated in float64 / complex128.  Untouched memory is compared byte for byte."""
import numpy as np
import pytest

from _gpu import dev_mat, dev_vec, outside_bytes, torch_cuda, torch_dtype  # noqa: F401
from _jacobi import CODE, uniform
from _krylov import MAX_RESTART, raw_orth, raw_orth_work, real_of, wide_of

pytestmark = pytest.mark.gpu

NS = (0, 1, 63, 64, 65, 255, 256, 257, 1000, 70_001)
KS = (0, 1, 2, 7, 8, 9, 31, 32, 33, MAX_RESTART)
GUARD = 5
# (name, pad of the leading dimension -- "p16": the smallest pad >= 1 that makes ldv * sizeof(T) a multiple of 16 --,
#  elements V and w start past a 16-byte boundary)
VARIANTS = (("ld_n_plus_3", 3, 0), ("ld_n_plus_3_off_1", 3, 1), ("ld_16_bytes_off_1", "p16", 1))
worst = {}


def pad_of(n, pad, dtype):
    if pad != "p16":
        return pad
    es = np.dtype(dtype).itemsize
    return next(p for p in range(1, 17) if ((n + p) * es) % 16 == 0)


class Case:
    """V (n x MAX_RESTART) and w on the device inside NaN-padded, guarded buffers, and their host copies"""

    def __init__(self, torch, rng, n, dtype, pad, off):
        self.torch, self.n, self.dtype, self.off = torch, n, np.dtype(dtype), off
        self.ld = n + pad_of(n, pad, dtype)
        self.V = np.asfortranarray(uniform(rng, (n, MAX_RESTART), dtype))
        self.w = uniform(rng, n, dtype)
        # the 256-byte aligned allocation + `off` elements: one element past a 16-byte boundary for off = 1
        self.vbuf, self.vd = dev_mat(torch, self.V, self.ld - n, off, GUARD)
        self.v_before = self.vbuf.cpu().numpy().tobytes()

    def run(self, k, w=None, hsum0=None, raw=False):
        """one pass over a fresh copy of w (or `w`) -> (w', hsum, nrm) on the host; checks every guard"""
        torch, n, dt = self.torch, self.n, self.dtype
        w = self.w if w is None else w
        wbuf, wd = dev_vec(torch, w, self.off, GUARD)
        hbuf, hd = dev_vec(torch, np.zeros(k, dt) if hsum0 is None else hsum0, 0, GUARD)
        nbuf, nd = dev_vec(torch, np.full(1, 7.0, real_of(dt)), 0, GUARD)
        need = raw_orth_work(CODE[dt], n, k)
        work = torch.full((need + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        before = [outside_bytes(wbuf, n, n, 1, self.off), outside_bytes(hbuf, k, k, 1), outside_bytes(nbuf, 1, 1, 1)]
        if raw:
            st = torch.cuda.current_stream().cuda_stream
            assert raw_orth(CODE[dt], n, k, self.vd.data_ptr(), self.ld, wd.data_ptr(), hd.data_ptr(), nd.data_ptr(), work.data_ptr(), st) == 0
        else:
            import bsm_amd as bsm
            bsm.krylov_orth(self.vd, wd, k, hd, nd, work=work)
        torch.cuda.synchronize()
        after = [outside_bytes(wbuf, n, n, 1, self.off), outside_bytes(hbuf, k, k, 1), outside_bytes(nbuf, 1, 1, 1)]
        assert before == after, "a guard element of w, hsum or nrm was written"
        assert bytes(work[need:].cpu().numpy()) == b"\xa5" * 64, "bytes behind the work array were written"
        assert self.vbuf.cpu().numpy().tobytes() == self.v_before, "V, its padding or its guard was written"
        return wd.cpu().numpy(), hd.cpu().numpy(), nd.cpu().numpy()[0]

    def check(self, k, tag):
        n, dt = self.n, self.dtype
        eps, wide, c = float(np.finfo(dt).eps), wide_of(dt), 2 if dt.kind == "c" else 1
        w1, h, nrm = self.run(k)
        Vw, ww = self.V[:, :k].astype(wide), self.w.astype(wide)
        # h
        err = np.abs(h.astype(wide) - Vw.conj().T @ ww)
        bound = c * n * eps * (np.abs(Vw).T @ np.abs(ww))
        assert np.all(err <= bound), (tag, "h", float(np.max(err - bound)))
        # w' with the returned h
        hw = h.astype(wide)
        err_w = np.abs(w1.astype(wide) - (ww - Vw @ hw))
        bound_w = c * (k + 2) * eps * (np.abs(ww) + np.abs(Vw) @ np.abs(hw))
        assert np.all(err_w <= bound_w), (tag, "w'", float(np.max(err_w - bound_w)))
        # the norm of the returned w'
        true = float(np.linalg.norm(w1.astype(wide)))
        assert abs(float(nrm) - true) <= max(n, 1) * eps * true, (tag, "nrm", float(nrm), true)
        if n == 0:
            assert nrm == 0 and np.all(h == 0)
        key = dt.name
        with np.errstate(divide="ignore", invalid="ignore"):
            rh = np.nanmax(np.where(bound > 0, err / bound, 0)) if k and n else 0.0
            rw = np.nanmax(np.where(bound_w > 0, err_w / bound_w, 0)) if n else 0.0
        worst[key] = (max(worst.get(key, (0, 0))[0], float(rh)), max(worst.get(key, (0, 0))[1], float(rw)))
        return w1, h, nrm


def check_accumulation_and_determinism(case, k, tag):
    """hsum accumulates, and equal inputs give equal bytes (the raw C entry on one of the two runs)"""
    w1, h1, n1 = case.run(k)
    w1b, h1b, n1b = case.run(k, raw=True)
    assert (w1.tobytes(), h1.tobytes(), n1.tobytes()) == (w1b.tobytes(), h1b.tobytes(), n1b.tobytes()), (tag, "not deterministic")
    # a second pass on w' with hsum = h1: the second pass's h is added -- bit for bit fl(h1 + h2), h2 from a fresh pass
    _, h2, _ = case.run(k, w=w1)
    _, hs, _ = case.run(k, w=w1, hsum0=h1)
    assert hs.tobytes() == (h1 + h2).astype(case.dtype).tobytes(), (tag, "hsum does not accumulate")


@pytest.mark.parametrize("variant", VARIANTS, ids=[v[0] for v in VARIANTS])
@pytest.mark.parametrize("n", NS)
def test_float64_full_cross_product(torch_cuda, n, variant):
    name, pad, off = variant
    case = Case(torch_cuda, np.random.default_rng(5000 + n), n, np.float64, pad, off)
    for k in KS:
        case.check(k, (n, k, name))
    check_accumulation_and_determinism(case, 9, (n, 9, name))
    print(f"KRYSTAT orth float64 n {n} {name}: worst h ratio {worst['float64'][0]:.3f}, worst w' ratio {worst['float64'][1]:.3f}")


@pytest.mark.parametrize("variant", VARIANTS, ids=[v[0] for v in VARIANTS])
@pytest.mark.parametrize("dtype", [np.float32, np.complex64, np.complex128], ids=["float32", "complex64", "complex128"])
def test_other_types_on_the_diagonals(torch_cuda, dtype, variant):
    """(n_i, k_i) and (n_i, k_{9 - i}): every n and every k twice, large n with small and with large k"""
    name, pad, off = variant
    for i, n in enumerate(NS):
        case = Case(torch_cuda, np.random.default_rng(5100 + n), n, dtype, pad, off)
        for k in sorted({KS[i], KS[len(KS) - 1 - i]}):
            case.check(k, (np.dtype(dtype).name, n, k, name))
        if n in (65, 1000):
            check_accumulation_and_determinism(case, KS[i], (np.dtype(dtype).name, n, name))
    key = np.dtype(dtype).name
    print(f"KRYSTAT orth {key} {name}: worst h ratio {worst[key][0]:.3f}, worst w' ratio {worst[key][1]:.3f}")


@pytest.mark.parametrize("dtype", [np.float64, np.complex64], ids=["float64", "complex64"])
def test_captured_into_a_graph_and_replayed(torch_cuda, bsm, dtype):
    """one pass captured (a linear graph: three launches in a row, no branches) gives on replay the bytes of the eager call"""
    torch = torch_cuda
    n, k = 1000, 9
    case = Case(torch, np.random.default_rng(5200), n, dtype, "p16", 0)
    w_eager, h_eager, n_eager = case.run(k)
    wd = torch.from_numpy(case.w).cuda()
    hd = torch.zeros(k, dtype=wd.dtype, device="cuda")
    nd = torch.zeros(1, dtype=torch_dtype(torch, real_of(dtype)), device="cuda")
    work = torch.empty(bsm.krylov_orth_work(dtype, n, k), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        bsm.krylov_orth(case.vd, wd, k, hd, nd, work=work)
    wd.copy_(torch.from_numpy(case.w).cuda())  # (capture does not run anything; be sure of the inputs anyway)
    hd.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert wd.cpu().numpy().tobytes() == w_eager.tobytes()
    assert hd.cpu().numpy().tobytes() == h_eager.tobytes() and nd.cpu().numpy()[0].tobytes() == n_eager.tobytes()


def test_python_wrapper_checks(torch_cuda, bsm):
    torch = torch_cuda
    V = torch.zeros(4, 10, dtype=torch.float64, device="cuda").t()  # 10 x 4, column-major
    w, h, nrm = (torch.zeros(m, dtype=torch.float64, device="cuda") for m in (10, 4, 1))
    with pytest.raises(TypeError):
        bsm.krylov_orth(V, w.float(), 2, h, nrm)
    with pytest.raises(TypeError):
        bsm.krylov_orth(V, w, 2, h, nrm.float())
    with pytest.raises(TypeError):
        bsm.krylov_orth(V.t().contiguous().t().t(), w[:4], 2, h, nrm)  # row-major
    with pytest.raises(ValueError):
        bsm.krylov_orth(V, w[:9], 2, h, nrm)
    with pytest.raises(ValueError):
        bsm.krylov_orth(V, w, 5, h, nrm)
    with pytest.raises(ValueError):
        bsm.krylov_orth(V, w, 2, h, nrm, work=torch.zeros(8, dtype=torch.uint8, device="cuda"))
    with pytest.raises(TypeError):
        bsm.krylov_orth(V.cpu(), w, 2, h, nrm)
