"""GPU suite (-m gpu): several right-hand sides on mixed-precision handles (BSM_F64_F32, BSM_C128_C64) -- the
single-precision image streamed ONCE per batch of double-precision columns (the interleaved pass, csrc/bsm_il.hip:
panel_kernel_il<ILMixed<S>, ...>), observed through bsm_value_passes.

    mixed Y  vs a pure double-precision handle of the ROUNDED blocks, column by column : <= 1e-13
    mixed Y  vs the oracle on the ORIGINAL blocks                                      : <= 1e-5
(the tolerances of tests/test_gpu_mixed_storage.py: a sum or an operand kept in single precision misses the first by
six orders of magnitude)
"""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if __name__ == "__main__":  # the child process of test_one_pass_observed
    sys.path[:0] = [ROOT, HERE]

from _common import Cc, N, T, fixture_problem, lens, oracle_mul, rand_vec, relerr, wrap  # noqa: E402
from _ctors import complexify, ctor_build, ctor_oracle_problem, ctor_problem  # noqa: E402
from _fuzz import rounded  # noqa: E402
from _gpu import dev_mat, gpu_mul, gpu_mul_multi, torch_cuda  # noqa: E402, F401
from _values import on_device  # noqa: E402

pytestmark = pytest.mark.gpu
OPS = [N, T, Cc]
PAIRS = [(np.float64, np.float32), (np.complex128, np.complex64)]
KS = (2, 3, 4, 5, 8, 9, 16, 17)
TOL_ROUNDED, TOL_ORACLE = 1e-13, 1e-5
# the generators' keywords per constructor route (those of tests/test_gpu_mixed_storage.py); FULL: C2 and C3 at full size
SIZES = {"blocksparse": dict(n=600, nblocks=60, bs=16), "vbcrs": dict(n=4000, nblocks=200, lo=4, hi=48),
         "symmetric": dict(nseg=16, bs=24, halfband=2), "vbcrs_from_symmetric": dict(nseg=16, bs=24, halfband=2)}
FULL = {"vbcrs": {}, "symmetric": {}}


def _cols(rng, n, k, dt):
    return np.asfortranarray(np.stack([rand_vec(rng, n, dt) for _ in range(k)], axis=1))


def _scalars(T_):
    """the two (alpha, beta, strong zero) cases of every comparison"""
    return ((1, 0, True), ((0.5 - 0.25j) if np.dtype(T_).kind == "c" else 0.5, 2.0, False))


# ---- 1. the product matrix ------------------------------------------------------------------------------------------
CTORS = ["blocksparse", "vbcrs", "symmetric", "vbcrs_from_symmetric"]
CTOR_TIMAGE = [(c, t) for c in CTORS for t in (0, 1) if t == 0 or c in ("blocksparse", "vbcrs")]


@pytest.mark.parametrize("acc", ["auto", "atomic", "direct", "gather"])
@pytest.mark.parametrize("T_, S_", PAIRS)
@pytest.mark.parametrize("ctor, timage", CTOR_TIMAGE)
def test_mixed_multi_product_matrix(torch_cuda, bsm, oracle, ctor, timage, T_, S_, acc):
    torch = torch_cuda
    p = ctor_problem(bsm, ctor, T_, SIZES)
    A = ctor_build(bsm, ctor, p, storage=S_, accumulate=acc, transpose_image=timage)
    R = ctor_build(bsm, ctor, rounded(p, S_), accumulate=acc, transpose_image=timage)  # pure T, rounded blocks
    rng = np.random.default_rng(11)
    kmax = max(KS)
    worst = 0.0
    for op in OPS:
        xl, yl = lens(p, op)
        X, Y0 = _cols(rng, xl, kmax, T_), _cols(rng, yl, kmax, T_)
        cases = _scalars(T_)
        # every column through the rounded pure handle's ONE-column product, and (beta = 0) the oracle on the original blocks
        refs = [np.stack([gpu_mul(torch, bsm, R, op, X[:, j], Y0[:, j], a, b, s) for j in range(kmax)], axis=1)
                for a, b, s in cases]
        orc = np.stack([oracle_mul(oracle, ctor_oracle_problem(ctor, p), op, X[:, j].copy(), Y0[:, j].copy())
                        for j in range(kmax)], axis=1)
        for k in KS:
            for (a, b, s), ref in zip(cases, refs):
                got = gpu_mul_multi(torch, bsm, A, op, X[:, :k], Y0[:, :k], a, b, s, pad=7)
                for j in range(k):
                    e = relerr(got[:, j], ref[:, j])
                    worst = max(worst, e)
                    assert e <= TOL_ROUNDED, (op, k, j, a, b, e)
                    if s:
                        assert relerr(got[:, j], orc[:, j]) <= TOL_ORACLE, (op, k, j)
    print(f"mixed multi {ctor} timage={timage} {np.dtype(S_)} {acc}: worst column error vs rounded pure {worst:.2e}")


# ---- 2. strong zero and NaN through the pass ---------------------------------------------------------------------------
@pytest.mark.parametrize("T_, S_", PAIRS)
@pytest.mark.parametrize("ctor", ["vbcrs", "symmetric"])
def test_mixed_multi_strong_zero_and_nan(torch_cuda, bsm, ctor, T_, S_):
    torch = torch_cuda
    p = ctor_problem(bsm, ctor, T_, SIZES)
    A = ctor_build(bsm, ctor, p, storage=S_)
    n = p["size"][0]
    X = _cols(np.random.default_rng(12), n, 8, T_)
    Ynan = np.full((n, 8), np.nan, dtype=T_, order="F")
    for op in OPS:
        before = A.value_passes()
        got = gpu_mul_multi(torch, bsm, A, op, X, Ynan, 0.5, 0, True, pad=3)   # strong zero: the NaN must not propagate
        assert A.value_passes() - before == 1, "K = 8 did not take the pass"
        assert np.all(np.isfinite(got)), op
        got = gpu_mul_multi(torch, bsm, A, op, X, Ynan, 0.5, 0.0, False, pad=3)  # a numeric zero multiplies: NaN stays
        assert np.all(np.isnan(got)), op


# ---- 3. state of the work arrays, the claim, owned rows ---------------------------------------------------------------
@pytest.mark.parametrize("T_, S_", PAIRS)
def test_mixed_multi_state_claim_and_ownership(torch_cuda, bsm, oracle, T_, S_):
    """What tests/test_gpu_parity.py::test_multi_rhs_interleaved_pass_state_and_ownership checks for the same-type pairs:
    alternating ops, widths and component counts on ONE rectangular handle (the accumulator W must be zero again after
    every pass -- a stale W shows at O(1)), two streams on one handle without synchronisation (the loser of the claim
    runs column by column), a handle that owns a row range.  Oracle on the ROUNDED blocks: <= 1e-13.  A MulPlan product
    (one column) runs between the passes."""
    torch = torch_cuda
    cplx = np.dtype(T_).kind == "c"
    rng = np.random.default_rng(31)
    nr, nc, nb = 700, 1100, 60
    blocks, ri, ci = [], [], []
    for b in range(nb):
        m_, n_ = int(rng.integers(3, 30)), int(rng.integers(2, 70))
        blk = rng.standard_normal((m_, n_)) + (1j * rng.standard_normal((m_, n_)) if cplx else 0)
        blocks.append(np.asfortranarray(blk.astype(T_)))
        ri.append(np.sort(rng.choice(nr, m_, replace=False)) + 1)
        ci.append(rng.choice(nc, n_, replace=False) + 1)
    p = dict(kind="blocksparse", blocks=blocks, rowindices=ri, colindices=ci, size=(nr, nc))
    pr = rounded(p, S_)
    A = bsm.synthetic.build(p, storage=S_)
    al, be = ((0.5 - 1j), 2j) if cplx else (0.75, -1.5)
    for op, k in ((N, 8), (T, 3), (Cc, 8), (N, 2), (T, 13), (N, 4), (Cc, 5), (N, 8)):
        xl, yl = lens(p, op)
        X, Y0 = _cols(rng, xl, k, T_), _cols(rng, yl, k, T_)
        got = gpu_mul_multi(torch, bsm, A, op, X, Y0, al, be, False, pad=1)
        ref = np.stack([oracle_mul(oracle, pr, op, X[:, j].copy(), Y0[:, j].copy(), al, be, False) for j in range(k)], axis=1)
        for j in range(k):
            assert relerr(got[:, j], ref[:, j]) <= TOL_ROUNDED, (op, k, j)
        if op == N and k == 4:  # a MulPlan product between two passes
            xd, yd = torch.from_numpy(X[:, 0].copy()).cuda(), torch.from_numpy(Y0[:, 0].copy()).cuda()
            before = A.value_passes()
            bsm.matrices.MulPlan(yd, A, xd, al, be)()
            torch.cuda.synchronize()
            assert A.value_passes() - before == 1
            assert relerr(yd.cpu().numpy(), ref[:, 0]) <= TOL_ROUNDED
    # two streams, one handle, no synchronisation in between
    f = fixture_problem("cuboid") if cplx else fixture_problem("cuboid", np.float64, "real")
    fr = rounded(f, S_)
    F = bsm.synthetic.build(f, storage=S_)
    n = f["size"][0]
    Xs = [_cols(rng, n, 8, T_) for _ in range(2)]
    Xd = [dev_mat(torch, x)[1] for x in Xs]
    Yd = [dev_mat(torch, np.full((n, 8), np.nan, dtype=T_, order="F"))[1] for _ in range(2)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    before = F.value_passes()
    for rep in range(6):
        for q in range(2):
            with torch.cuda.stream(streams[q]):
                bsm.mul(Yd[q], F, Xd[q])
    torch.cuda.synchronize()
    extra = F.value_passes() - before - 12  # a product that got the claim: 1 pass, one that lost it: 8
    assert 0 <= extra <= 12 * 7 and extra % 7 == 0, extra
    print(f"two streams ({np.dtype(S_)}): {extra // 7} of 12 products lost the claim and ran column by column")
    for q in range(2):
        ref = np.stack([oracle_mul(oracle, fr, N, Xs[q][:, j].copy(), np.zeros(n, T_)) for j in range(8)], axis=1)
        got = Yd[q].cpu().numpy()
        for j in range(8):
            assert relerr(got[:, j], ref[:, j]) <= TOL_ROUNDED, (q, j)
    # a handle that owns the middle rows only: beta on the owned rows, sums on top of what was there outside them
    s_ = bsm.synthetic.config5(n=9000, lo=8, hi=40, halfband=3)
    if cplx:
        for i, key in enumerate(("diagonals", "offdiagonals")):
            s_[key] = complexify(s_[key], 40 + i)
    sr = rounded(s_, S_)
    n = s_["size"][0]
    own = (3001, 6000)
    Sm = bsm.synthetic.build(s_, own=own, storage=S_)
    for k in (8, 16, 5):
        X, Y0 = _cols(rng, n, k, T_), _cols(rng, n, k, T_)
        got = gpu_mul_multi(torch, bsm, Sm, N, X, Y0, al, be, False)
        for j in range(k):  # the single product through the same handle defines the semantics outside the owned range
            assert relerr(got[:, j], gpu_mul(torch, bsm, Sm, N, X[:, j], Y0[:, j], al, be, False)) <= TOL_ROUNDED, (k, j)
        ref = oracle_mul(oracle, sr, N, X[:, 0].copy(), Y0[:, 0].copy(), al, be, False)
        assert relerr(got[own[0] - 1:own[1], 0], ref[own[0] - 1:own[1]]) <= TOL_ROUNDED


# ---- 4. graph capture -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T_, S_", PAIRS)
def test_mixed_multi_graph_capture(torch_cuda, bsm, T_, S_):
    """a captured K = 8 product never gets the work arrays: it is eight one-column products, counted at capture"""
    torch = torch_cuda
    p = ctor_problem(bsm, "symmetric", T_, SIZES)
    A = ctor_build(bsm, "symmetric", p, storage=S_)
    n = p["size"][0]
    X = dev_mat(torch, _cols(np.random.default_rng(14), n, 8, T_))[1]
    Y = dev_mat(torch, np.zeros((n, 8), dtype=T_, order="F"))[1]
    eager = dev_mat(torch, np.zeros((n, 8), dtype=T_, order="F"))[1]
    before = A.value_passes()
    bsm.mul(eager, A, X)
    torch.cuda.synchronize()
    assert A.value_passes() - before == 1
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        bsm.mul(Y, A, X)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    before = A.value_passes()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        bsm.mul(Y, A, X)
    assert A.value_passes() - before == 8
    ref = eager.cpu().numpy()
    for _ in range(2):
        Y.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        got = Y.cpu().numpy()
        for j in range(8):
            assert relerr(got[:, j], ref[:, j]) <= TOL_ROUNDED, j
    assert A.value_passes() - before == 8  # a replay enqueues nothing through the library


# ---- 5. host vectors ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T_, S_", PAIRS)
@pytest.mark.parametrize("ctor", ["vbcrs", "symmetric"])
def test_mixed_multi_host_vectors(torch_cuda, bsm, oracle, ctor, T_, S_):
    p = ctor_problem(bsm, ctor, T_, SIZES)
    A = ctor_build(bsm, ctor, p, storage=S_)
    n = p["size"][0]
    rng = np.random.default_rng(15)
    al, be = _scalars(T_)[1][:2]
    for op in (N, T):
        X, Y0 = _cols(rng, n, 8, T_), _cols(rng, n, 8, T_)
        Y = Y0.copy(order="F")
        before = A.value_passes()
        bsm.mul(Y, wrap(bsm, A, op), X, al, be)
        assert A.value_passes() - before == 1
        Z = np.full((n, 8), np.nan, dtype=T_, order="F")
        bsm.mul(Z, wrap(bsm, A, op), X)
        for j in range(8):
            ref = oracle_mul(oracle, ctor_oracle_problem(ctor, rounded(p, S_)), op, X[:, j].copy(), Y0[:, j].copy(), al, be, False)
            assert relerr(Y[:, j], ref) <= TOL_ROUNDED, (op, j)
            assert relerr(Z[:, j], oracle_mul(oracle, ctor_oracle_problem(ctor, p), op, X[:, j].copy(), Y0[:, j].copy())) <= TOL_ORACLE


# ---- 6. one pass, observed ---------------------------------------------------------------------------------------------
def _observed_handles(bsm, T_, S_):
    """name -> (handle, problem): an atomic, an exclusive-forward and a fused symmetric mixed handle, a coloured one, and
    a gather one whose column products are deterministic in every op (one producer per y entry: VBCRS with its second,
    transposed ordering -- bsm_mul_multi never takes the gather workspace, its columns accumulate with atomics)"""
    pb, pv, ps = (ctor_problem(bsm, c, T_, SIZES) for c in ("blocksparse", "vbcrs", "symmetric"))
    out = dict(atomic=(ctor_build(bsm, "blocksparse", pb, storage=S_, accumulate="atomic"), pb),
               exclusive=(ctor_build(bsm, "vbcrs", pv, storage=S_), pv),
               fused=(ctor_build(bsm, "symmetric", ps, storage=S_), ps),
               colored=(ctor_build(bsm, "symmetric", ps, storage=S_, accumulate="colored"), ps),
               gather=(ctor_build(bsm, "vbcrs", pv, storage=S_, accumulate="gather", transpose_image=1), pv))
    assert out["exclusive"][0].stats()["exclusive"] == 1
    return out


def _delta(torch, bsm, A, p, k, op=N):
    T_ = A.dtype
    xl, yl = lens(p, op)
    rng = np.random.default_rng(100 + k)
    X = _cols(rng, xl, k, T_)
    before = A.value_passes()
    if k == 1:
        Y = gpu_mul(torch, bsm, A, op, X[:, 0], np.zeros(yl, T_))[:, None]
    else:
        Y = gpu_mul_multi(torch, bsm, A, op, X, np.zeros((yl, k), dtype=T_, order="F"))
    return A.value_passes() - before, X, Y


@pytest.mark.parametrize("T_, S_", PAIRS)
def test_one_pass_observed(torch_cuda, bsm, T_, S_):
    torch = torch_cuda
    cplx = np.dtype(T_).kind == "c"
    want = {8: 1, 16: 2, 17: 3, 1: 1} if cplx else {8: 1, 16: 1, 24: 2, 17: 2, 1: 1}
    H = _observed_handles(bsm, T_, S_)
    for name in ("atomic", "exclusive", "fused"):
        A, p = H[name]
        for k, passes in want.items():
            assert _delta(torch, bsm, A, p, k)[0] == passes, (name, k)
    assert _delta(torch, bsm, *H["colored"], 8)[0] == 8   # coloured images keep their bitwise reproducible columns
    ps = ctor_problem(bsm, "symmetric", T_, SIZES)
    assert _delta(torch, bsm, ctor_build(bsm, "symmetric", ps), ps, 8)[0] == 1  # the counter on the existing paths
    # BSM_MULTI_IL=0: today's contract, still reachable (the library reads the switch once per process)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), np.dtype(T_).name, np.dtype(S_).name],
                       env=dict(os.environ, BSM_MULTI_IL="0"), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    out = r.stdout.decode()
    assert r.returncode == 0 and out.strip().endswith("CHILD OK"), out[-3000:] + r.stderr.decode()[-3000:]


def _child_no_il(T_, S_):
    """BSM_MULTI_IL=0: K = 8 is eight one-column products on every mixed handle, bitwise equal to eight bsm_mul calls
    where those are deterministic (op N of the exclusive-forward handle, every op of the gather one)"""
    import torch
    import bsm_amd as bsm
    assert os.environ.get("BSM_MULTI_IL") == "0"
    H = _observed_handles(bsm, T_, S_)
    for name, (A, p) in H.items():
        for op in OPS:
            d, X, Y = _delta(torch, bsm, A, p, 8, op)
            assert d == 8, (name, op, d)
            if (name == "exclusive" and op == N) or name == "gather":
                for j in range(8):
                    col = gpu_mul(torch, bsm, A, op, X[:, j], np.zeros(Y.shape[0], A.dtype))
                    assert Y[:, j].tobytes() == col.tobytes(), (name, op, j)
    ps = ctor_problem(bsm, "symmetric", T_, SIZES)
    assert _delta(torch, bsm, ctor_build(bsm, "symmetric", ps), ps, 8)[0] == 1  # pure handle: the multi-RHS kernels
    print("CHILD OK")


# ---- 7. full size ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def c3_pair(torch_cuda, bsm):
    """full-size C3: (problem, mixed handle, pure double handle of the rounded blocks), built once for tests 7 and 8"""
    p = ctor_problem(bsm, "symmetric", np.float64, FULL)
    A = ctor_build(bsm, "symmetric", on_device(torch_cuda, p), storage=np.float32)
    pr = rounded(p, np.float32)
    R = ctor_build(bsm, "symmetric", on_device(torch_cuda, pr))
    return p, pr, A, R


def _full_size(torch, bsm, oracle, p, pr, A, R):
    rng = np.random.default_rng(16)
    for op in (N, T):
        xl, yl = lens(p, op)
        X, Y0 = _cols(rng, xl, 8, np.float64), _cols(rng, yl, 8, np.float64)
        before = A.value_passes()
        got = gpu_mul_multi(torch, bsm, A, op, X, Y0, 0.5, 2.0, False, pad=64)
        assert A.value_passes() - before == 1
        for j in range(8):
            ref = gpu_mul(torch, bsm, R, op, X[:, j], Y0[:, j], 0.5, 2.0, False)
            assert relerr(got[:, j], ref) <= TOL_ROUNDED, (op, j)
        got = gpu_mul_multi(torch, bsm, A, op, X, np.full_like(Y0, np.nan))
        for j in (0, 7):
            assert relerr(got[:, j], oracle_mul(oracle, pr, op, X[:, j].copy(), Y0[:, j].copy())) <= TOL_ROUNDED, (op, j)
            assert relerr(got[:, j], oracle_mul(oracle, p, op, X[:, j].copy(), Y0[:, j].copy())) <= TOL_ORACLE, (op, j)


def test_mixed_multi_full_size_c3(torch_cuda, bsm, oracle, c3_pair):
    _full_size(torch_cuda, bsm, oracle, *c3_pair)


def test_mixed_multi_full_size_c2(torch_cuda, bsm, oracle):
    p = ctor_problem(bsm, "vbcrs", np.float64, FULL)
    pr = rounded(p, np.float32)
    A = ctor_build(bsm, "vbcrs", on_device(torch_cuda, p), storage=np.float32)
    R = ctor_build(bsm, "vbcrs", on_device(torch_cuda, pr))
    _full_size(torch_cuda, bsm, oracle, p, pr, A, R)


# ---- 8. it pays -----------------------------------------------------------------------------------------------------
def test_mixed_multi_pays_on_c3(torch_cuda, bsm, c3_pair):
    """Full-size C3, mixed handle: (a) one K = 8 mul(Y, A, X) against (b) eight one-column mul calls on the same handle --
    what a K = 8 product was before the pass, on kernels the pass does not touch.  Median over 7 alternations, each timed
    with device events around 50 repetitions after a warm-up.  Required: (a) <= 0.75 x (b); the measured ratio is in
    docs/experiments_r09.md."""
    torch = torch_cuda
    p, _, A, _ = c3_pair
    n = p["size"][0]
    rng = np.random.default_rng(17)
    X = dev_mat(torch, _cols(rng, n, 8, np.float64))[1]
    Y = dev_mat(torch, np.zeros((n, 8), order="F"))[1]
    xs = [X[:, j].contiguous() for j in range(8)]
    ys = [torch.zeros(n, dtype=torch.float64, device="cuda") for _ in range(8)]

    def batch():
        bsm.mul(Y, A, X)

    def columns():
        for j in range(8):
            bsm.mul(ys[j], A, xs[j])

    def timed(f, reps=50):
        for _ in range(5):
            f()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            f()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) * 1e3 / reps  # us

    before = A.value_passes()
    batch()
    assert A.value_passes() - before == 1
    ta, tb = [], []
    for _ in range(7):
        ta.append(timed(batch))
        tb.append(timed(columns))
    a, b = float(np.median(ta)), float(np.median(tb))
    print(f"C3 mixed x 8: one product {a:.1f} us, eight one-column products {b:.1f} us, ratio {a / b:.3f}")
    assert a <= 0.75 * b, (a, b)


if __name__ == "__main__":
    _child_no_il(np.dtype(sys.argv[1]).type, np.dtype(sys.argv[2]).type)
