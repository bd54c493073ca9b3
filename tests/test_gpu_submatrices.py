"""GPU suite of bsm_submatrices / bsm_diag: the legs of test_submatrices_cpu.py on device handles, in both memspaces,
against the dense ground truth of tests/_submat.py AND against the host loop of an analysis-only handle (the same wave
records, decoded in plain C++): bit-identical where at most one stored value lands, within the derived bound elsewhere."""
import numpy as np
import pytest

from _common import NODEV, Cc, N, T, rand_vec, wrap
from _ctors import ctor_build
from _fuzz import restrict_rows, seed_of
from _gpu import TOL, dev_mat, outside_bytes, torch_cuda  # noqa: F401
from _submat import Truth, accept, bits, check_sets, disjoint_rounds, partition_sets, raw_submatrices
from _values import on_device, value_operators

pytestmark = pytest.mark.gpu

KINDS = ["blocksparse", "vbcrs", "symmetric"]
TYPES = [(np.float32, None), (np.float64, None), (np.complex64, None), (np.complex128, None),
         (np.float64, np.float32), (np.complex128, np.complex64)]
TYPE_IDS = [np.dtype(d).name + ("" if s is None else "_as_" + np.dtype(s).name) for d, s in TYPES]
OPS = (N, T, Cc)
NOPER = 4  # operators per (kind, types): the first of the value fuzz


def kw_of(storage):
    return {} if storage is None else {"storage": storage}


def one_based(n):
    return np.arange(1, n + 1, dtype=np.int64)


def device_call(torch, bsm, A, op, I, J, dtype):
    """bsm_submatrices into NaN-filled device arrays with ldo = ni + 3, two elements into their buffers and four in front
    of their ends, on torch's current stream -> the windows; every byte outside them must come back unchanged"""
    arrs = [dev_mat(torch, np.full((len(i), len(j)), np.nan, dtype=dtype), pad=3, off=2, guard=4) for i, j in zip(I, J)]
    before = [outside_bytes(b, len(i), len(i) + 3, len(j), 2) for (b, _), i, j in zip(arrs, I, J)]
    ptrs = [v.data_ptr() if v.numel() else None for _, v in arrs]
    rc = raw_submatrices(A, op, I, J, ptrs, [len(i) + 3 for i in I], 1, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, bsm._lib.lib().bsm_last_error()
    after = [outside_bytes(b, len(i), len(i) + 3, len(j), 2) for (b, _), i, j in zip(arrs, I, J)]
    assert after == before, "a byte outside a window was written"
    return [v.cpu().numpy() for _, v in arrs]


def same_as_host(dev, host, truth, op, I, J, what):
    """device result against the analysis-only handle's host loop"""
    _, Ab, Cn = truth.of(op)
    for s, (d, h, i, j) in enumerate(zip(dev, host, I, J)):
        if d.size == 0:
            continue
        sel = np.ix_(np.asarray(i) - 1, np.asarray(j) - 1)
        one = Cn[sel] <= 1
        same = (bits(d).reshape(d.shape + (-1,)) == bits(h).reshape(h.shape + (-1,))).all(axis=-1)
        assert np.all(same[one]), (what, s, "kernel and host loop differ where one stored value lands")
        bound = Cn[sel] * np.finfo(d.dtype).eps * Ab[sel]
        assert np.all(np.abs(d - h)[~one] <= bound[~one]), (what, s)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype,storage", TYPES, ids=TYPE_IDS)
def test_selections_in_both_memspaces_and_against_the_host_loop(torch_cuda, bsm, kind, dtype, storage):
    torch = torch_cuda
    rng = np.random.default_rng(seed_of(kind, dtype) + 9400)
    for case, p in enumerate(value_operators(kind, dtype)[:NOPER]):
        A = bsm.synthetic.build(p, **kw_of(storage))
        H = bsm.synthetic.build(p, device=NODEV, **kw_of(storage))
        tr = Truth(p, storage)
        for op in OPS:
            Aop, Hop = wrap(bsm, A, op), wrap(bsm, H, op)
            m, n = bsm.size(Aop)
            legs = [("full", [one_based(m)], [one_based(n)]),
                    ("halves", [rng.permutation(m)[:m // 2] + 1], [rng.permutation(n)[:n // 2] + 1]),
                    ("partition",) + partition_sets(rng, (m, n))]
            if kind == "symmetric":
                own = [bsm.diagonalindices(Aop, d) for d in bsm.eachdiagonalindex(Aop)]
                legs.append(("own sets", own, own))
                rl = [bsm.rowindices(Aop, b) for b in bsm.eachoffdiagonalindex(Aop)]
                cl = [bsm.colindices(Aop, b) for b in bsm.eachoffdiagonalindex(Aop)]
                for ids in disjoint_rounds(rl, cl)[:2]:
                    legs.append(("pairs", [rl[b] for b in ids], [cl[b] for b in ids]))
                    legs.append(("swapped pairs", [cl[b] for b in ids], [rl[b] for b in ids]))
            for name, I, J in legs:
                tag = (kind, case, op, name)
                host = bsm.submatrices(Hop, I, J)
                staged = bsm.submatrices(Aop, I, J)  # BSM_MEM_HOST on the device handle
                direct = device_call(torch, bsm, A, op, I, J, dtype)
                mirror = [t.cpu().numpy() for t in bsm.submatrices(Aop, I, J, device=True)]
                for got in (staged, direct, mirror):
                    check_sets(tr, op, got, I, J, tag)
                    same_as_host(got, host, tr, op, I, J, tag)
        # diag(A), both memspaces
        k = np.arange(min(p["size"]))
        dh = bsm.diag(H)
        for d in (bsm.diag(A), bsm.diag(A, device=True).cpu().numpy()):
            accept(d, tr.D[k, k], tr.Abs[k, k], tr.Cnt[k, k], (kind, case, "diag"))
            same_as_host([d[:, None]], [dh[:, None]], _DiagTruth(tr, k), N, [k + 1], [[1]], (kind, case))
        dadj = bsm.diag(bsm.adjoint(A), device=True).cpu().numpy()  # (two device runs may add overlapping entries in another order)
        same_as_host([dadj[:, None]], [dh.conj()[:, None]], _DiagTruth(tr, k), N, [k + 1], [[1]], (kind, case, "adjoint"))
        buf, view = dev_mat(torch, np.full((len(k), 1), np.nan, dtype=dtype), pad=2, off=3, guard=5)
        before = outside_bytes(buf, len(k), len(k) + 2, 1, 3)
        assert bsm._lib.lib().bsm_diag(A._h.ptr, view.data_ptr(), 1, torch.cuda.current_stream().cuda_stream) == 0
        assert outside_bytes(buf, len(k), len(k) + 2, 1, 3) == before
        same_as_host([view.cpu().numpy()], [dh[:, None]], _DiagTruth(tr, k), N, [k + 1], [[1]], (kind, case, "padded"))


class _DiagTruth:
    """the diagonal of a Truth as a one-column operator, for same_as_host"""

    def __init__(self, tr, k):
        self.Abs, self.Cnt = tr.Abs[k, k][:, None], tr.Cnt[k, k][:, None]

    def of(self, op):
        return None, self.Abs, self.Cnt


@pytest.mark.parametrize("kind", KINDS)
def test_three_virtual_devices(torch_cuda, bsm, kind):
    """every stored entry lives in exactly one part: the parts' staging buffers add up to the operator"""
    torch = torch_cuda
    rng = np.random.default_rng(seed_of(kind, np.float64) + 9500)
    p = value_operators(kind, np.float64)[0]
    A, tr = ctor_build(bsm, kind, p, devices=[0, 0, 0]), Truth(p)
    assert len(A.parts()) == 3
    for op in OPS:
        Aop = wrap(bsm, A, op)
        m, n = bsm.size(Aop)
        I, J = partition_sets(rng, (m, n))
        check_sets(tr, op, bsm.submatrices(Aop, I, J), I, J, (kind, op, "parts, host"))
        check_sets(tr, op, device_call(torch, bsm, A, op, I, J, np.float64), I, J, (kind, op, "parts, device"))
    k = np.arange(min(p["size"]))
    for d in (bsm.diag(A), bsm.diag(A, device=True).cpu().numpy()):
        accept(d, tr.D[k, k], tr.Abs[k, k], tr.Cnt[k, k], (kind, "parts", "diag"))


def test_device_resident_blocks_and_an_own_slice(torch_cuda, bsm):
    torch = torch_cuda
    rng = np.random.default_rng(seed_of("symmetric", np.complex128) + 9600)
    p = value_operators("symmetric", np.complex128)[1]
    A, tr = bsm.synthetic.build(on_device(torch, p)), Truth(p)
    own = [bsm.diagonalindices(A, d) for d in bsm.eachdiagonalindex(A)]
    check_sets(tr, N, bsm.submatrices(A, own), own, own, "device blocks, own sets")
    I, J = partition_sets(rng, p["size"])
    check_sets(tr, Cc, device_call(torch, bsm, A, Cc, I, J, np.complex128), I, J, "device blocks, adjoint")
    # a VBCRS that holds the blocks of a row slice: the entries of those blocks
    v = value_operators("vbcrs", np.float32)[0]
    nr = v["size"][0]
    lo, hi = nr // 4, 3 * nr // 4
    q = restrict_rows(v, lo, hi)
    assert 0 < len(q["blocks"]) < len(v["blocks"])
    B, tq = bsm.synthetic.build(q, own=(lo, hi)), Truth(q)
    I, J = partition_sets(rng, q["size"])
    check_sets(tq, N, bsm.submatrices(B, I, J), I, J, "own slice")
    k = np.arange(min(q["size"]))
    accept(bsm.diag(B), tq.D[k, k], tq.Abs[k, k], tq.Cnt[k, k], "own slice, diag")


@pytest.mark.parametrize("kind", KINDS)
def test_a_call_on_the_default_stream_leaves_the_image_alone(torch_cuda, bsm, kind):
    torch = torch_cuda
    p = value_operators(kind, np.float64)[3]
    A = bsm.synthetic.build(p, accumulate="gather")  # bitwise reproducible products
    m, n = p["size"]
    x = torch.from_numpy(rand_vec(np.random.default_rng(3), n, np.float64)).cuda()
    y0, y1 = torch.empty(m, dtype=torch.float64, device="cuda"), torch.empty(m, dtype=torch.float64, device="cuda")
    bsm.mul(y0, A, x)
    out = torch.full((m * n,), float("nan"), dtype=torch.float64, device="cuda")
    assert raw_submatrices(A, N, [one_based(m)], [one_based(n)], [out.data_ptr()], [m], 1, None) == 0  # stream 0
    bsm.mul(y1, A, x)
    torch.cuda.synchronize()
    assert y1.cpu().numpy().tobytes() == y0.cpu().numpy().tobytes()
    accept(out.cpu().numpy().reshape(n, m).T, *Truth(p).of(N), (kind, "default stream"))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", [np.float32, np.complex128], ids=lambda d: np.dtype(d).name)
def test_getitem_against_the_product_route(torch_cuda, bsm, kind, dtype):
    """A[:, :] is the reference's own test of the product (unit vectors through bsm_mul_multi); it rounds differently, so
    the tolerance is that of a product against the oracle (TOL)"""
    rng = np.random.default_rng(seed_of(kind, dtype) + 9700)
    p = min(value_operators(kind, dtype), key=lambda q: q["size"][0] * q["size"][1])
    A = bsm.synthetic.build(p)
    for op in OPS:
        Aop = wrap(bsm, A, op)
        full = Aop[:, :]
        m, n = full.shape
        I, J = rng.integers(0, m, 40), rng.integers(0, n, 50)
        for got, want in ((Aop[I, J], full[np.ix_(I, J)]), (Aop[:, 7], full[:, 7]), (Aop[-1, ::-2], full[-1, ::-2])):
            err = float(np.max(np.abs(got - want)) / max(float(np.max(np.abs(full))), 1e-30))
            print(f"  getitem {kind} {np.dtype(dtype).name} op {op}: {err:.3e}")
            assert got.shape == want.shape and err < TOL[np.dtype(dtype)], (kind, op, err)
