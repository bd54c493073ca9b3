"""GPU suite (-m gpu): the cross-type (vector type, stored type) pairs on the layout-edge operators of tests/_fuzz.py --
mixed storage (float32 under float64, complex64 under complex128) and real operators under complex vectors (float64 under
complex128, float32 under complex64) -- HIP path through bsm.mul against the CPU oracle: one column, several columns (the
interleaved pass on both sides of the thresholds of csrc/bsm_plan.cpp, observed through bsm_value_passes), the plan's
switches in child processes, vectors that do not start on a 16-byte boundary (all eight pairs), owned row ranges.

The oracle runs on the ROUNDED blocks for the mixed pairs and on the blocks promoted to complex128, with complex128
vectors, for real operators under complex vectors.  Norm and bounds are those of tests/test_gpu_fuzz.py:
    max|got - ref| / max|ref|  <  1e-12 (float64 / complex128 vectors),  1e-5 (complex64 vectors)
Coloured cases follow _fuzz.build_fuzz; every test asserts that at least half of its coloured cases ran.  Every test
prints one PAIRSTAT line (worst error, products and columns checked): docs/experiments_r11.md quotes them."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if __name__ == "__main__":  # the child process of test_several_columns_under_the_plan_switches
    sys.path[:0] = [ROOT, HERE]

from _common import BLOCK_KEYS, Cc, N, T, acc_modes, lens, oracle_mul, rand_vec, wrap  # noqa: E402
from _fuzz import CROSS_PAIRS, GEN, Stat, build_fuzz, cast_blocks, restrict_rows, rounded, scalar_sets, seed_of  # noqa: E402
from _gpu import TOL, dev_mat, dev_vec, env, gpu_mul, outside_bytes  # noqa: E402, F401

pytestmark = pytest.mark.gpu
KINDS = ["blocksparse", "vbcrs", "symmetric"]
SAME_PAIRS = [(t, t, None) for t in (np.float32, np.float64, np.complex64, np.complex128)]
KS = (2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 24, 35)


def _pid(pair):
    return "{}_on_{}".format(np.dtype(pair[1]).name, np.dtype(pair[2] if pair[2] is not None else pair[0]).name)


def _seed(kind, pair, offset):
    """seed_of plus a fixed offset per test and pair (two cross pairs share a block type)"""
    return seed_of(kind, pair[0]) + offset + 100 * (CROSS_PAIRS + SAME_PAIRS).index(pair)


def _storage_kw(pair):
    return {} if pair[2] is None else {"storage": pair[2]}


def _oracle_problem(p, pair):
    B, V, S = pair
    if S is not None:
        return rounded(p, S)
    return cast_blocks(p, np.complex128) if np.dtype(V) != np.dtype(B) else p


def _ref(oracle, q, pair, op, x, y0, alpha, beta, strong):
    B, V, _ = pair
    if np.dtype(V) != np.dtype(B):  # a real operator under complex vectors: complex128 throughout, and C is T
        x, y0 = np.asarray(x, np.complex128), np.asarray(y0, np.complex128)
        op = T if op == Cc else op
    return oracle_mul(oracle, q, op, np.ascontiguousarray(x), np.ascontiguousarray(y0), alpha, beta, strong)


def _has_off(p):
    """whether the image has off-diagonal pieces of a symmetric operator (every product of it runs both halves)"""
    return p["kind"] == "symmetric" and any(b.size for b in p["offdiagonals"])


def _passes(K, pair, has_off, colored):
    """value streams of a K-column product of a cross pair (csrc/bsm_plan.cpp: next_batch): one per batch of the
    interleaved pass -- 16 real / 8 complex columns while at least `least` are left -- and one per column left; coloured
    handles and BSM_MULTI_IL=0 have no such batch"""
    if K == 1:
        return 1
    if colored or int(os.environ.get("BSM_MULTI_IL", "1")) == 0:
        return K
    if pair[2] is None:
        least = 2
    elif "BSM_IL_MIXED_MIN_COLS" in os.environ:
        least = min(max(int(os.environ["BSM_IL_MIXED_MIN_COLS"]), 2), 8)
    else:
        least = 2 if has_off else 3
    KK = 8 if np.dtype(pair[1]).kind == "c" else 16
    n, left = 0, K
    while left >= least:
        left -= min(KK, left)
        n += 1
    return n + left


def _pairstat(st):
    st.done("PAIRSTAT", f"products {st.products} columns {st.columns}")


def _cases(bsm, st, rng, kind, pair, count, modes=None):
    """`count` operators of GEN[kind], modes cycled, transpose_image every third case -> (case, acc, problem, handle)"""
    modes = modes or acc_modes(kind)
    for case in range(count):
        acc = modes[case % len(modes)]
        kw = _storage_kw(pair)
        if kind != "symmetric" and case % 3 == 0:
            kw["transpose_image"] = True
        p, A = build_fuzz(bsm, rng, kind, np.dtype(pair[0]), acc, **kw)
        st.coloured += acc == "colored"
        if A is None:
            continue
        st.ran += acc == "colored"
        yield case, acc, p, A


# ---- 1. one column ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("pair", CROSS_PAIRS, ids=_pid)
def test_one_column(env, kind, pair):
    torch, bsm, oracle = env
    V = np.dtype(pair[1])
    tol = TOL[V]
    st = Stat("one", kind, _pid(pair))
    rng = np.random.default_rng(_seed(kind, pair, 1000))
    for case, acc, p, A in _cases(bsm, st, rng, kind, pair, 24):
        q = _oracle_problem(p, pair)
        for op in (N, T, Cc):
            xl, yl = lens(p, op)
            x, y0 = rand_vec(rng, xl, V), rand_vec(rng, yl, V)
            ynan = y0.copy()
            ynan[::7] = np.nan
            for alpha, beta, strong in scalar_sets(V):
                # strong zero: the NaN of the incoming y must vanish
                got = gpu_mul(torch, bsm, A, op, x, ynan if strong else y0, alpha, beta, strong)
                st.products += 1
                if strong:
                    assert np.all(np.isfinite(got)), (st.tag, case, acc, op, "strong zero left a NaN")
                ref = _ref(oracle, q, pair, op, x, y0, alpha, beta, strong)
                st.check(got, ref, tol, (case, acc, op, alpha, beta))
            # a numeric zero multiplies: the NaN stays, every other entry is alpha * op(A) * x
            got = gpu_mul(torch, bsm, A, op, x, ynan, -0.5, 0.0, False)
            st.products += 1
            assert np.all(np.isnan(got[::7])), (st.tag, case, acc, op, "numeric beta = 0 dropped a NaN")
            ref = _ref(oracle, q, pair, op, x, y0, -0.5, 0, True)
            keep = np.ones(yl, dtype=bool)
            keep[::7] = False
            st.check(np.where(keep, got, 0), np.where(keep, ref, 0), tol, (case, acc, op, "beta = 0.0"))
    _pairstat(st)


# ---- 2. several columns ------------------------------------------------------------------------------------------------
def _several_columns(torch, bsm, oracle, st, kind, pair, count, offset):
    """The core loop of test_several_columns and of its child processes: K of KS columns per product, column-major X and
    Y with an odd pad of NaN rows, complex scalars for complex vectors, the value streams counted"""
    V = np.dtype(pair[1])
    tol = TOL[V]
    rng = np.random.default_rng(_seed(kind, pair, offset))
    am, bm = (-0.5 + 0.75j, 1.25 - 0.5j) if V.kind == "c" else (-0.5, 1.25)
    for case, acc, p, A in _cases(bsm, st, rng, kind, pair, count):
        q = _oracle_problem(p, pair)
        has_off = _has_off(p)
        for op in (N, T, Cc):
            xl, yl = lens(p, op)
            k = int(rng.choice(KS))
            strong = bool(rng.integers(0, 2))
            padx, pady = 2 * int(rng.integers(0, 5)) + 1, 2 * int(rng.integers(0, 5)) + 1
            X = np.asfortranarray(np.stack([rand_vec(rng, xl, V) for _ in range(k)], axis=1))
            Y0 = np.asfortranarray(np.stack([rand_vec(rng, yl, V) for _ in range(k)], axis=1))
            xb, Xd = dev_mat(torch, X, padx)
            yb, Yd = dev_mat(torch, Y0, pady)
            before = (outside_bytes(xb, xl, xl + padx, k), outside_bytes(yb, yl, yl + pady, k), xb.cpu().numpy().tobytes())
            passes = A.value_passes()
            bsm.mul(Yd, wrap(bsm, A, op), Xd, am, False if strong else bm)
            torch.cuda.synchronize()
            st.products += 1
            what = (case, acc, op, k, "strong" if strong else "beta")
            assert A.value_passes() - passes == _passes(k, pair, has_off, acc == "colored"), (st.tag, what, "value streams")
            pads = outside_bytes(yb, yl, yl + pady, k)
            assert pads == before[1] and np.all(np.isnan(np.frombuffer(pads, dtype=V))), (st.tag, what, "pad rows of Y written")
            assert xb.cpu().numpy().tobytes() == before[2], (st.tag, what, "X written")
            assert np.all(np.isnan(np.frombuffer(before[0], dtype=V)))
            got = Yd.cpu().numpy()
            for j in range(k):
                ref = _ref(oracle, q, pair, op, X[:, j], Y0[:, j], am, bm, strong)
                st.check(got[:, j], ref, tol, what + (j,))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("pair", CROSS_PAIRS, ids=_pid)
def test_several_columns(env, kind, pair):
    torch, bsm, oracle = env
    st = Stat("multi", kind, _pid(pair))
    _several_columns(torch, bsm, oracle, st, kind, pair, 24, 2000)
    _pairstat(st)


# ---- 3. the plan's switches, read once per process --------------------------------------------------------------------
@pytest.mark.parametrize("env_extra", [{"BSM_MULTI_IL": "0"}, {"BSM_MULTI_IL": "2", "BSM_IL_XCD": "5"},
                                       {"BSM_IL_MIXED_MIN_COLS": "8"}], ids=lambda e: ",".join(f"{k}={v}" for k, v in e.items()))
def test_several_columns_under_the_plan_switches(env_extra):
    """test_several_columns' loop in a child process per setting: the interleaved pass switched off (every column a
    one-column product), its workgroups dealt to the XCDs in runs of 5, and mixed storage taking it from 8 columns on"""
    r = subprocess.run(["timeout", "-k", "10", "900", sys.executable, os.path.abspath(__file__), "6"],
                       env=dict(os.environ, **env_extra), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    out = r.stdout.decode()
    print("\n".join(ln for ln in out.splitlines() if ln.startswith(("PAIRSTAT", "CHILD"))))
    assert r.returncode == 0, out[-3000:] + r.stderr.decode()[-3000:]
    last = out.strip().splitlines()[-1]
    assert last.startswith("CHILD OK") and int(last.split()[2]) > 1000, last


def _child_switches(count):
    import torch
    import bsm_amd as bsm
    from oracle import load_oracle
    oracle = load_oracle()
    columns = 0
    for kind in KINDS:
        for pair in CROSS_PAIRS:
            st = Stat("child", kind, _pid(pair))
            _several_columns(torch, bsm, oracle, st, kind, pair, count, 3000)
            _pairstat(st)
            columns += st.columns
    print(f"CHILD OK {columns} columns checked")


# ---- 4. vectors off a 16-byte boundary, all eight pairs ---------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("pair", SAME_PAIRS + CROSS_PAIRS, ids=_pid)
def test_unaligned_vectors(env, kind, pair):
    """x and y start 1, 2 and 3 elements into NaN-filled device buffers, with guard elements behind: the product is
    that of the oracle and no element outside y (guards and pad rows) changes a bit; x is not written at all"""
    torch, bsm, oracle = env
    V = np.dtype(pair[1])
    tol = TOL[V]
    st = Stat("unaligned", kind, _pid(pair))
    rng = np.random.default_rng(_seed(kind, pair, 4000))
    am, bm = (-0.5 + 0.75j, 1.25 - 0.5j) if V.kind == "c" else (-0.5, 1.25)
    for case, acc, p, A in _cases(bsm, st, rng, kind, pair, 6, modes=["atomic", "gather"]):
        q = _oracle_problem(p, pair)
        offx, offy = case % 3 + 1, (case + 1) % 3 + 1
        for op in (N, T, Cc):
            xl, yl = lens(p, op)
            for k in (1, 5):
                X = np.asfortranarray(np.stack([rand_vec(rng, xl, V) for _ in range(k)], axis=1))
                Y0 = np.asfortranarray(np.stack([rand_vec(rng, yl, V) for _ in range(k)], axis=1))
                for strong in (True, False):
                    if k == 1:
                        xb, xv = dev_vec(torch, X[:, 0], offx, 5)
                        yb, yv = dev_vec(torch, Y0[:, 0], offy, 5)
                        padx = pady = 0
                    else:
                        padx, pady = 3, 1
                        xb, xv = dev_mat(torch, X, padx, offx, 5)
                        yb, yv = dev_mat(torch, Y0, pady, offy, 5)
                    assert xv.data_ptr() % 16 == (offx * V.itemsize) % 16 and yv.data_ptr() % 16 == (offy * V.itemsize) % 16
                    before = (xb.cpu().numpy().tobytes(), outside_bytes(yb, yl, yl + pady, k, offy))
                    bsm.mul(yv, wrap(bsm, A, op), xv, am, False if strong else bm)
                    torch.cuda.synchronize()
                    st.products += 1
                    what = (case, acc, op, k, "strong" if strong else "beta", offx, offy)
                    assert xb.cpu().numpy().tobytes() == before[0], (st.tag, what, "x written")
                    assert outside_bytes(yb, yl, yl + pady, k, offy) == before[1], (st.tag, what, "a guard element of y changed")
                    got = yv.cpu().numpy().reshape(yl, k)
                    for j in range(k):
                        ref = _ref(oracle, q, pair, op, X[:, j], Y0[:, j], am, bm, strong)
                        st.check(got[:, j], ref, tol, what + (j,))
    _pairstat(st)


@pytest.mark.parametrize("pair", [SAME_PAIRS[3], CROSS_PAIRS[1], CROSS_PAIRS[2]], ids=_pid)
def test_complex128_y_on_an_8_byte_boundary_through_the_c_abi(env, pair):
    """No tensor view puts a complex128 vector on an 8-byte boundary; a C caller can.  bsm_mul / bsm_mul_cvec with y at
    data_ptr() + 8, on atomic-mode handles and beta != 1 (numeric and strong zero): y .*= beta runs element by element
    (csrc/bsm_one.hip: scale_kernel, the branch for a gap that is no multiple of the element size)"""
    torch, bsm, oracle = env
    from bsm_amd import _lib as L
    V = np.dtype(np.complex128)
    st = Stat("abi8", "all", _pid(pair))
    fn = L.lib().bsm_mul_cvec if np.dtype(pair[0]).kind != "c" else L.lib().bsm_mul
    alpha, beta = np.array([-0.5 + 0.75j]), np.array([1.25 - 0.5j])
    for kind in KINDS:
        rng = np.random.default_rng(_seed(kind, pair, 5000))
        for case, acc, p, A in _cases(bsm, st, rng, kind, pair, 4, modes=["atomic"]):
            q = _oracle_problem(p, pair)
            for op in (N, T, Cc):
                xl, yl = lens(p, op)
                x, y0 = rand_vec(rng, xl, V), rand_vec(rng, yl, V)
                xd = torch.from_numpy(x).cuda()
                for strong in (1, 0):
                    flat = np.full(2 * yl + 4, np.nan)  # doubles: one in front of y, three behind
                    flat[1:1 + 2 * yl] = y0.view(np.float64)
                    yb = torch.from_numpy(flat).cuda()
                    assert (yb.data_ptr() + 8) % 16 == 8
                    L.check(fn(A._h.ptr, op, xd.data_ptr(), yb.data_ptr() + 8, alpha.ctypes.data, beta.ctypes.data, strong,
                               L.BSM_MEM_DEVICE, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
                    torch.cuda.synchronize()
                    st.products += 1
                    out = yb.cpu().numpy()
                    what = (kind, case, op, "strong" if strong else "beta")
                    assert out[:1].tobytes() + out[1 + 2 * yl:].tobytes() == flat[:1].tobytes() + flat[1 + 2 * yl:].tobytes(), what
                    ref = _ref(oracle, q, pair, op, x, y0, alpha[0], beta[0], bool(strong))
                    st.check(out[1:1 + 2 * yl].copy().view(np.complex128), ref, TOL[V], what)
    _pairstat(st)


def _entries(p):
    return sum(b.size for k in BLOCK_KEYS for b in p.get(k, []))


def _first_hull(p):
    """(lowest, highest) row of the first block that has entries"""
    if p["kind"] == "vbcrs":
        b = next(i for i, blk in enumerate(p["blocks"]) if blk.size)
        return int(p["rowstart"][b]), int(p["rowstart"][b]) + p["blocks"][b].shape[0] - 1
    if p["kind"] == "blocksparse":
        r = next(r for r, blk in zip(p["rowindices"], p["blocks"]) if blk.size)
    elif p["diagonals"]:
        r = p["diagonalindices"][0]
    else:
        r = np.concatenate([p["rowindices"][0], p["colindices"][0]])
    return int(np.min(r)), int(np.max(r))


# ---- 5. owned row ranges ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("pair", CROSS_PAIRS, ids=_pid)
def test_owned_rows(env, kind, pair):
    """own=(lo, hi) on the blocks of a random operator whose rows all lie in the range (_fuzz.restrict_rows), op N, one
    column and eight, host and device vectors: rows outside the range come back bit for bit, rows inside are the
    oracle's product of the restricted operator.  Under the strong zero the incoming owned rows hold NaN."""
    torch, bsm, oracle = env
    B, V = np.dtype(pair[0]), np.dtype(pair[1])
    tol = TOL[V]
    st = Stat("own", kind, _pid(pair))
    rng = np.random.default_rng(_seed(kind, pair, 6000))
    am, bm = (-0.5 + 0.75j, 1.25 - 0.5j) if V.kind == "c" else (-0.5, 1.25)
    modes = ["auto", "atomic", "gather"]
    for case in range(6):
        full = GEN[kind](rng, B)
        nr, nc = full["size"]
        lo, hi = nr // 4 + 1 + int(rng.integers(0, 9)), 3 * nr // 4 - int(rng.integers(0, 9))
        p = restrict_rows(full, lo, hi)
        if not _entries(p):  # (scattered row sets: none inside the middle half) -- the row hull of the first block instead
            lo, hi = _first_hull(full)
            p = restrict_rows(full, lo, hi)
        assert _entries(p)
        A = bsm.synthetic.build(p, own=(lo, hi), accumulate=modes[case % 3], **_storage_kw(pair))
        q = _oracle_problem(p, pair)
        inside = np.zeros(nr, dtype=bool)
        inside[lo - 1:hi] = True
        for k in (1, 8):
            X = np.asfortranarray(np.stack([rand_vec(rng, nc, V) for _ in range(k)], axis=1))
            Y0 = np.asfortranarray(np.stack([rand_vec(rng, nr, V) for _ in range(k)], axis=1))
            for strong in (True, False):
                Yin = Y0.copy(order="F")
                if strong:
                    Yin[lo - 1:hi:7] = np.nan
                for where in ("host", "device"):
                    if where == "host":
                        xh, yh = (X[:, 0].copy(), Yin[:, 0].copy()) if k == 1 else (X, Yin.copy(order="F"))
                        bsm.mul(yh, A, xh, am, False if strong else bm)
                        got = yh.reshape(nr, k)
                    else:
                        xb, xv = dev_vec(torch, X[:, 0]) if k == 1 else dev_mat(torch, X, 1)
                        yb, yv = dev_vec(torch, Yin[:, 0]) if k == 1 else dev_mat(torch, Yin, 3)
                        bsm.mul(yv, A, xv, am, False if strong else bm)
                        torch.cuda.synchronize()
                        got = yv.cpu().numpy().reshape(nr, k)
                    st.products += 1
                    what = (case, modes[case % 3], k, "strong" if strong else "beta", where, lo, hi)
                    assert got[~inside].tobytes() == Yin[~inside].tobytes(), (st.tag, what, "a row outside the owned range changed")
                    assert np.all(np.isfinite(got[inside])), (st.tag, what)
                    for j in range(k):
                        ref = _ref(oracle, q, pair, N, X[:, j], Y0[:, j], am, bm, strong)
                        st.check(got[inside, j], ref[inside], tol, what + (j,))
    _pairstat(st)


if __name__ == "__main__":
    _child_switches(int(sys.argv[1]))
