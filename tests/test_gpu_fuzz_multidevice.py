"""GPU suite (-m gpu): ONE handle spread over the devices of a bsm_ctx_t (csrc/bsm_dist.cpp) on the layout-edge operators
of tests/_fuzz.py: block rows that start anywhere and reach into the next part's rows, scattered / unsorted / strided
index lists, empty blocks, parts without blocks, rectangular sizes (the column partition is then equal chunks).

Virtual devices (`devices=[0] * P`, P cycling through 2, 3, 5 -- five parts get the per-device issuing threads), the
operators exactly as the generator draws them (150 - 900 rows), seeds from _fuzz.seed_of (BSM_FUZZ_OFFSET explores other
streams), every product against the CPU oracle on the WHOLE operator:
    max|got - ref| / max|ref|  <  1e-12 (float64 / complex128),  1e-5 (float32 / complex64)
Accumulation modes: auto / atomic / gather, and coloured under the rule of _fuzz.build_fuzz.  Every test prints one
DISTDEV line (worst error, products, parts without blocks): docs/experiments_r14.md quotes them."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

from _common import Cc, N, T, acc_modes, lens, nblocks, oracle_mul, rand_vec, wrap  # noqa: E402
from _fuzz import Stat, build_fuzz, scalar_sets, seed_of, squared  # noqa: E402
from _gpu import TOL, dev_mat, env, gpu_mul, outside_bytes, scatter  # noqa: E402, F401

pytestmark = pytest.mark.gpu
KINDS = ["blocksparse", "vbcrs", "symmetric"]
DTYPES = [np.float64, np.complex128, np.float32, np.complex64]
PS = (2, 3, 5)
KS = (3, 8, 11, 17, 20)  # the 8-column batches, a remainder, more than the copy path's 16
OPS = (N, T, Cc)


def _did(dt):
    return np.dtype(dt).name


def _distdev(st, need_empty=False):
    st.done("DISTDEV", f"products {st.products} operators {st.cases} parts_without_blocks {st.empty_parts}")
    if need_empty:
        assert st.empty_parts > 0, (st.tag, "no part without blocks in the whole run")


def _device_cases(bsm, st, kind, dt, count, offset, modes=None, square_every=0):
    """`count` operators of GEN[kind] over P = 2, 3, 5 virtual devices, modes cycled -> (case, acc, P, problem, handle);
    square_every = k: every k-th operator widened to square (_fuzz.squared) before the handle is built"""
    modes = modes or acc_modes(kind)
    rng = np.random.default_rng(seed_of(kind, dt) + offset)
    for case in range(count):
        acc, P = modes[case % len(modes)], PS[case % len(PS)]
        p, A = build_fuzz(bsm, rng, kind, np.dtype(dt), acc, devices=[0] * P)
        if square_every and case % square_every == 0 and A is not None and p["size"][0] != p["size"][1]:
            p = squared(p)
            A = bsm.synthetic.build(p, accumulate=acc, devices=[0] * P)
        st.coloured += acc == "colored"
        if A is None:
            continue
        st.ran += acc == "colored"
        st.cases += 1
        st.empty_parts += sum(q["nblocks"] == 0 for q in A.parts())
        yield case, acc, P, p, A, rng


def _check_parts(p, A, P):
    """own ranges tile the rows and `cols` the columns, in order; rows == cols on square operators; touched contains own;
    every block in one part"""
    parts = A.parts()
    nr, nc = p["size"]
    assert len(parts) == P
    for key, n in (("own", nr), ("cols", nc)):
        nxt = 1
        for q in parts:
            lo, hi = q[key]
            assert hi >= lo - 1, (key, q)
            if hi >= lo:
                assert lo == nxt, (key, [r[key] for r in parts])
                nxt = hi + 1
        assert nxt == n + 1, (key, [r[key] for r in parts])
    if nr == nc:
        assert [q["own"] for q in parts] == [q["cols"] for q in parts]
    for q in parts:
        if q["own"][1] >= q["own"][0] and q["touched"][1] >= q["touched"][0]:
            assert q["touched"][0] <= q["own"][0] and q["touched"][1] >= q["own"][1], q
    assert sum(q["nblocks"] for q in parts) == nblocks(p)
    return parts


def _one(torch, bsm, oracle, st, p, A, op, x, yin, y0, alpha, beta, strong, where, tol, what):
    """one bsm.mul on host or device vectors against the oracle; yin: the incoming y (NaN under the strong zero)"""
    ref = oracle_mul(oracle, p, op, x, y0, alpha, beta, strong)
    if where == "host":
        got = np.array(yin, copy=True)
        bsm.mul(got, wrap(bsm, A, op), x, alpha, False if strong else beta)
    else:
        got = gpu_mul(torch, bsm, A, op, x, yin, alpha, beta, strong)
    st.products += 1
    if strong:
        assert np.all(np.isfinite(got)), (st.tag, what, where, "the strong zero left a NaN")
    st.check(got, ref, tol, what + (where,))


# ---- 1. parts and one-column products ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dt", DTYPES, ids=_did)
def test_parts_and_products(env, kind, dt):
    torch, bsm, oracle = env
    dt = np.dtype(dt)
    st = Stat("mul", kind, _did(dt))
    for case, acc, P, p, A, rng in _device_cases(bsm, st, kind, dt, 10, 1000):
        _check_parts(p, A, P)
        for op in OPS:
            xl, yl = lens(p, op)
            x, y0 = rand_vec(rng, xl, dt), rand_vec(rng, yl, dt)
            ynan = y0.copy()
            ynan[::7] = np.nan
            for alpha, beta, strong in scalar_sets(dt):
                for where in ("host", "device"):
                    _one(torch, bsm, oracle, st, p, A, op, x, ynan if strong else y0, y0, alpha, beta, strong, where, TOL[dt],
                         (case, acc, P, op, alpha, beta))
    _distdev(st, need_empty=True)


# ---- 2. several right-hand sides ----------------------------------------------------------------------------------------
def _several(torch, bsm, oracle, st, case, acc, P, p, A, rng, dt, ops=OPS):
    from bsm_amd import _lib as L
    tol = TOL[dt]
    am, bm = (-0.5 + 0.75j, 1.25 - 0.5j) if dt.kind == "c" else (-0.5, 1.25)
    for op in ops:
        xl, yl = lens(p, op)
        k = int(rng.choice(KS))
        strong = bool(rng.integers(0, 2))
        padx, pady = 2 * int(rng.integers(0, 5)) + 1, 2 * int(rng.integers(0, 5)) + 1
        X = np.asfortranarray(np.stack([rand_vec(rng, xl, dt) for _ in range(k)], axis=1))
        Y0 = np.asfortranarray(np.stack([rand_vec(rng, yl, dt) for _ in range(k)], axis=1))
        refs = [oracle_mul(oracle, p, op, np.ascontiguousarray(X[:, j]), np.ascontiguousarray(Y0[:, j]), am, bm, strong)
                for j in range(k)]
        what = (case, acc, P, op, k, "strong" if strong else "beta")
        # device memory, padded leading dimensions through bsm.mul
        xb, Xd = dev_mat(torch, X, padx)
        yb, Yd = dev_mat(torch, Y0, pady)
        pads = outside_bytes(yb, yl, yl + pady, k)
        bsm.mul(Yd, wrap(bsm, A, op), Xd, am, False if strong else bm)
        torch.cuda.synchronize()
        st.products += 1
        assert outside_bytes(yb, yl, yl + pady, k) == pads and np.all(np.isnan(np.frombuffer(pads, dtype=dt))), \
            (st.tag, what, "pad rows of Y written")
        assert bool(torch.equal(Xd.cpu(), torch.from_numpy(X))), (st.tag, what, "X written")
        got = Yd.cpu().numpy()
        for j in range(k):
            st.check(got[:, j], refs[j], tol, what + ("device", j))
        # host memory through the C ABI: ldx, ldy > n, NaN in the pad rows
        Xh = np.full((xl + padx, k), np.nan, dtype=dt, order="F")
        Yh = np.full((yl + pady, k), np.nan, dtype=dt, order="F")
        Xh[:xl], Yh[:yl] = X, Y0
        a, b = np.array([am], dtype=dt), np.array([bm], dtype=dt)
        L.check(L.lib().bsm_mul_multi(A._h.ptr, op, k, Xh.ctypes.data, xl + padx, Yh.ctypes.data, yl + pady, a.ctypes.data,
                                      b.ctypes.data, 1 if strong else 0, L.BSM_MEM_HOST, None))
        st.products += 1
        assert np.all(np.isnan(Yh[yl:])) and np.all(np.isnan(Xh[xl:])), (st.tag, what, "pad rows written")
        assert np.array_equal(Xh[:xl], X), (st.tag, what, "X written")
        for j in range(k):
            st.check(Yh[:yl, j], refs[j], tol, what + ("host, C ABI", j))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dt", DTYPES, ids=_did)
def test_several_columns(env, kind, dt):
    torch, bsm, oracle = env
    dt = np.dtype(dt)
    st = Stat("multi", kind, _did(dt))
    for case, acc, P, p, A, rng in _device_cases(bsm, st, kind, dt, 10, 2000):
        _several(torch, bsm, oracle, st, case, acc, P, p, A, rng, dt)
    _distdev(st)


# ---- 3. partitioned vectors: bsm.mul_parts ------------------------------------------------------------------------------
def _gathered(parts_t, ranges, n, dt):
    got = np.full(n, np.nan, dtype=dt)
    for (lo, hi), t in zip(ranges, parts_t):
        if hi >= lo:
            got[lo - 1:hi] = t.cpu().numpy()
    return got


def _parts_product(torch, bsm, oracle, st, p, A, op, x, yin, y0, alpha, beta, strong, tol, what):
    parts = A.parts()
    rows, cols = [q["own"] for q in parts], [q["cols"] for q in parts]
    xr, yr = (cols, rows) if op == N else (rows, cols)
    ref = oracle_mul(oracle, p, op, x, y0, alpha, beta, strong)
    xp, yp = scatter(torch, x, xr), scatter(torch, yin, yr)
    bsm.mul_parts(yp, wrap(bsm, A, op), xp, alpha, False if strong else beta)
    torch.cuda.synchronize()
    st.products += 1
    st.check(_gathered(yp, yr, len(y0), y0.dtype), ref, tol, what + ("parts",))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dt", DTYPES, ids=_did)
def test_partitioned_vectors(env, kind, dt):
    """x and y scattered by the parts' own / column ranges (None for an empty range), every op, twice (reused buffers),
    operators as drawn (rectangular: the column partition is equal chunks) and every third widened to square; on square
    real operators the y parts of one product are the x parts of the next"""
    torch, bsm, oracle = env
    dt = np.dtype(dt)
    st = Stat("parts", kind, _did(dt))
    rect = chained = 0
    for case, acc, P, p, A, rng in _device_cases(bsm, st, kind, dt, 10, 3000, square_every=3):
        parts = _check_parts(p, A, P)
        nr, nc = p["size"]
        rect += nr != nc
        for op in OPS:
            xl, yl = lens(p, op)
            x, y0 = rand_vec(rng, xl, dt), rand_vec(rng, yl, dt)
            ynan = y0.copy()
            ynan[::7] = np.nan
            for alpha, beta, strong in scalar_sets(dt):
                for rep in range(2):
                    _parts_product(torch, bsm, oracle, st, p, A, op, x, ynan if strong else y0, y0, alpha, beta, strong,
                                   TOL[dt], (case, acc, P, op, alpha, beta, rep))
        if nr == nc and dt.kind != "c":
            x = rand_vec(rng, nc, dt)
            xp = scatter(torch, x, [q["cols"] for q in parts])
            y1 = [torch.full_like(t, float("nan")) if t is not None else None for t in xp]
            y2 = [torch.full_like(t, float("nan")) if t is not None else None for t in xp]
            bsm.mul_parts(y1, A, xp)
            bsm.mul_parts(y2, A, y1)
            torch.cuda.synchronize()
            st.products += 2
            mid = _gathered(y1, [q["own"] for q in parts], nr, dt)
            st.check(mid, oracle_mul(oracle, p, N, x, np.zeros(nr, dtype=dt)), TOL[dt], (case, acc, P, "chain 1"))
            # the second product against the oracle on the FIRST product's own output: one product's rounding
            st.check(_gathered(y2, [q["own"] for q in parts], nr, dt), oracle_mul(oracle, p, N, mid, np.zeros(nr, dtype=dt)),
                     TOL[dt], (case, acc, P, "chain 2"))
            chained += 1
    _distdev(st)
    assert chained > 0 or dt.kind == "c"
    assert rect > 0 or kind == "symmetric"


# ---- 4. the copy path ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dt", DTYPES, ids=_did)
def test_copy_path(env, kind, dt, monkeypatch):
    """BSM_DIST_COPIES=1: devices without peer access (hipMemcpyPeerAsync + adds): one column and several, host and
    device vectors; the partitioned-vector entry has no copy path and says so"""
    torch, bsm, oracle = env
    monkeypatch.setenv("BSM_DIST_COPIES", "1")
    dt = np.dtype(dt)
    st = Stat("copies", kind, _did(dt))
    for case, acc, P, p, A, rng in _device_cases(bsm, st, kind, dt, 5, 4000):
        for op in OPS:
            xl, yl = lens(p, op)
            x, y0 = rand_vec(rng, xl, dt), rand_vec(rng, yl, dt)
            ynan = y0.copy()
            ynan[::7] = np.nan
            for alpha, beta, strong in scalar_sets(dt)[-2:]:
                for where in ("host", "device"):
                    _one(torch, bsm, oracle, st, p, A, op, x, ynan if strong else y0, y0, alpha, beta, strong, where, TOL[dt],
                         (case, acc, P, op, alpha, beta))
        _several(torch, bsm, oracle, st, case, acc, P, p, A, rng, dt, ops=(OPS[case % 3], OPS[(case + 1) % 3]))
        if case == 0:
            parts = A.parts()
            xp = scatter(torch, rand_vec(rng, p["size"][1], dt), [q["cols"] for q in parts])
            yp = scatter(torch, rand_vec(rng, p["size"][0], dt), [q["own"] for q in parts])
            with pytest.raises(RuntimeError, match="peer access"):
                bsm.mul_parts(yp, A, xp)
    _distdev(st)


# ---- 5. the switches of the fused path ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("switch", ["flags_off", "one_stream", "rezero_off"])
def test_fused_path_switches(env, kind, switch, monkeypatch):
    """ordering by events in place of flags, all parts on the caller's stream, work vectors cleared in front of every
    product in place of kept zero (tests/test_gpu_multidevice.py: test_flag_and_event_ordering_of_the_fan_out) -- each
    on three operators: products chained without synchronisation, partitioned vectors in between"""
    torch, bsm, oracle = env
    monkeypatch.setenv("BSM_DIST_FLAGS", "0" if switch == "flags_off" else "1")
    monkeypatch.setenv("BSM_DIST_ONE_STREAM", "1" if switch == "one_stream" else "0")
    monkeypatch.setenv("BSM_DIST_REZERO", "0" if switch == "rezero_off" else "1")
    for dt in (np.dtype(np.float64),):
        st = Stat(switch, kind, _did(dt))
        for case, acc, P, p, A, rng in _device_cases(bsm, st, kind, dt, 3, 5000, modes=["auto", "atomic", "gather"]):
            pending = []
            for op in (N, T, N, T):
                xl, yl = lens(p, op)
                x, y0 = rand_vec(rng, xl, dt), rand_vec(rng, yl, dt)
                y0[::5] = np.nan
                yd = torch.from_numpy(y0.copy()).cuda()
                bsm.mul(yd, wrap(bsm, A, op), torch.from_numpy(x).cuda())  # no synchronisation in between
                pending.append((op, x, y0, yd))
            x = rand_vec(rng, p["size"][1], dt)
            y0 = rand_vec(rng, p["size"][0], dt)
            _parts_product(torch, bsm, oracle, st, p, A, N, x, y0, y0, 0.75, -1.5, False, TOL[dt], (case, acc, P, switch))
            _one(torch, bsm, oracle, st, p, A, T, pending[1][1], pending[1][2], np.nan_to_num(pending[1][2]), 1, 0, True,
                 "host", TOL[dt], (case, acc, P, switch))
            _several(torch, bsm, oracle, st, case, acc, P, p, A, rng, dt, ops=(N,))
            torch.cuda.synchronize()
            for i, (op, x, y0, yd) in enumerate(pending):
                st.products += 1
                st.check(yd.cpu().numpy(), oracle_mul(oracle, p, op, x, y0, 1, 0, True), TOL[dt], (case, acc, P, switch, i))
        _distdev(st)


# ---- 6. stale state on one handle ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dt", DTYPES, ids=_did)
def test_products_in_random_order_on_one_handle(env, kind, dt):
    """12 products per operator in a seeded random order over (op, 1 / 5 / 11 columns, host or device vectors, mul or
    mul_parts) on ONE handle, every result checked: a work vector left non-zero, a receive buffer sized for the other
    direction or for fewer columns shows in the product after it"""
    torch, bsm, oracle = env
    dt = np.dtype(dt)
    tol = TOL[dt]
    st = Stat("order", kind, _did(dt))
    am, bm = (-0.5 + 0.75j, 1.25 - 0.5j) if dt.kind == "c" else (-0.5, 1.25)
    for case, acc, P, p, A, rng in _device_cases(bsm, st, kind, dt, 6, 6000):
        for step in range(12):
            op = OPS[int(rng.integers(0, 3))]
            k = int(rng.choice((1, 5, 11)))
            where = ("host", "device", "parts")[int(rng.integers(0, 3))]
            strong = bool(rng.integers(0, 2))
            xl, yl = lens(p, op)
            what = (case, acc, P, step, op, k, where, "strong" if strong else "beta")
            if where == "parts" or k == 1:
                x, y0 = rand_vec(rng, xl, dt), rand_vec(rng, yl, dt)
                yin = y0.copy()
                if strong:
                    yin[::7] = np.nan
                if where == "parts":
                    _parts_product(torch, bsm, oracle, st, p, A, op, x, yin, y0, am, bm, strong, tol, what)
                else:
                    _one(torch, bsm, oracle, st, p, A, op, x, yin, y0, am, bm, strong, where, tol, what)
                continue
            X = np.asfortranarray(np.stack([rand_vec(rng, xl, dt) for _ in range(k)], axis=1))
            Y0 = np.asfortranarray(np.stack([rand_vec(rng, yl, dt) for _ in range(k)], axis=1))
            if where == "host":
                got = Y0.copy(order="F")
                bsm.mul(got, wrap(bsm, A, op), X, am, False if strong else bm)
            else:
                yb, Yd = dev_mat(torch, Y0, 3)
                bsm.mul(Yd, wrap(bsm, A, op), dev_mat(torch, X, 1)[1], am, False if strong else bm)
                got = Yd.cpu().numpy()
            st.products += 1
            for j in range(k):
                ref = oracle_mul(oracle, p, op, np.ascontiguousarray(X[:, j]), np.ascontiguousarray(Y0[:, j]), am, bm, strong)
                st.check(got[:, j], ref, tol, what + (j,))
    _distdev(st)
