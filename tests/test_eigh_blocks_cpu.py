"""CPU suite of bsm_eigh_blocks (batched Hermitian Jacobi eigensolver), bsm_spectral_blocks (V f(w) V^H) and
block_jacobi(kind="abs" | "pinv") on analysis-only handles: the BSM_MEM_HOST route runs the rotations the device kernel runs,
serially in plain C++, so the method, the info convention, the refusals and the Python composition are checked here without
a GPU.  The twin, the matrices and the figures are derived in tests/_eigh.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from _common import NODEV
from _cg import NB, NCG
from _eigh import (ABS_COUNTS, BATCH_CLASSES, CODE, DTYPES, FUNC, RHO_MAX, abs_minv, batch, check_spectral, check_spectral_jacobi,
                   eigh_twin, f_of, figures, matrix, rank_deficient, raw_eigh, raw_spectral, real_of, wide_of)
from _jacobi import KINDS, dense_of, jacobi_problem, outside, padded, uniform
from _krylov import rtol_of
from _minres import cut_operator, minres_problem, minres_twin
from _values import src_list

IDS = [np.dtype(d).name for d in DTYPES]
CASES = [(k, dt) for k in KINDS for dt in DTYPES if not (k == "symmetric" and np.dtype(dt).kind == "c")]
CASE_IDS = [f"{k}-{np.dtype(dt).name}" for k, dt in CASES]
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_the_twin_stays_below_one_on_the_inputs_of_the_gpu_suite(dtype):
    worst = [0.0, 0.0, 0.0]
    most = 0
    for cls, B in batch(dtype):
        w, V, sweeps, info = eigh_twin(B)
        f = figures(B, w, V)
        print(f"  twin {np.dtype(dtype).name} {cls} n {B.shape[0]}: {sweeps} sweeps, rho_w {f[0]:.3f} rho_r {f[1]:.3f} rho_o {f[2]:.3f}")
        assert info == 0 and max(f) <= 1.0, (cls, B.shape[0], f)
        worst, most = [max(a, b) for a, b in zip(worst, f)], max(most, sweeps)
    print(f"EIGHSTAT twin {np.dtype(dtype).name} worst rho_w {worst[0]:.3f} rho_r {worst[1]:.3f} rho_o {worst[2]:.3f}, most sweeps {most}")
    assert most <= 13


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_host_route_on_padded_blocks(bsm, dtype):
    """the whole batch in one call, ld = n + 3 with NaN padding that must come back bit-identical, the n = 0 block with a NULL
    pointer; vectors = 0 gives the same w"""
    real = real_of(dtype)
    blocks = batch(dtype)
    bufs = [padded(B, 3) for _, B in blocks]
    ns = [B.shape[0] for _, B in blocks]
    before = [outside(buf, n, n + 3) for (buf, _), n in zip(bufs, ns)]
    ws = [np.full(n + 2, -5.0, real) for n in ns]  # two guard entries behind every w
    rc, info, sweeps = raw_eigh(CODE[np.dtype(dtype)], [buf if n else None for (buf, _), n in zip(bufs, ns)], ns, [n + 3 for n in ns],
                                [w if n else None for w, n in zip(ws, ns)])
    assert rc == 0 and not info.any(), (rc, info)
    worst = [0.0, 0.0, 0.0]
    for (buf, view), (cls, B), w, n, was, sw in zip(bufs, blocks, ws, ns, before, sweeps):
        assert outside(buf, n, n + 3) == was, "a byte outside a window was written"
        assert np.all(w[n:] == -5.0) and np.all(np.diff(w[:n]) >= 0)
        f = figures(B, w[:n], view)
        print(f"  host {np.dtype(dtype).name} {cls} n {n}: {sw} sweeps, rho_w {f[0]:.3f} rho_r {f[1]:.3f} rho_o {f[2]:.3f}")
        assert max(f) <= RHO_MAX and 0 <= sw <= 20, (cls, n, f, sw)
        worst = [max(a, b) for a, b in zip(worst, f)]
    print(f"EIGHSTAT host {np.dtype(dtype).name} worst rho_w {worst[0]:.3f} rho_r {worst[1]:.3f} rho_o {worst[2]:.3f}, most sweeps {sweeps.max()}")
    X = [B.copy(order="F") for _, B in blocks]
    w0 = [np.empty(n, real) for n in ns]
    rc, info, _ = raw_eigh(CODE[np.dtype(dtype)], [x if x.size else None for x in X], ns, [max(n, 1) for n in ns],
                           [w if n else None for w, n in zip(w0, ns)], vectors=0, sweeps=False)
    assert rc == 0 and not info.any()
    assert all(a.tobytes() == b[:n].tobytes() for a, b, n in zip(w0, ws, ns))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_info_1_spares_the_neighbours(bsm, dtype):
    rng = np.random.default_rng(3810)
    good = [matrix(rng, "uniform", n, dtype) for n in (7, 9, 17)]
    nan = matrix(rng, "uniform", 9, dtype)
    nan[3, 4] = np.nan
    inf = matrix(rng, "uniform", 5, dtype)
    inf[4, 4] = np.inf
    given = [good[0], nan, good[1], inf, good[2]]
    X = [b.copy(order="F") for b in given]
    ws = [np.zeros(b.shape[0], real_of(dtype)) for b in given]
    rc, info, sweeps = raw_eigh(CODE[np.dtype(dtype)], X, [b.shape[0] for b in X], [b.shape[0] for b in X], ws)
    assert rc == 0 and info.tolist() == [0, 1, 0, 1, 0], info
    for k in (1, 3):
        assert X[k].tobytes() == given[k].tobytes() and np.all(np.isnan(ws[k])) and sweeps[k] == 0
    for k in (0, 2, 4):
        assert max(figures(given[k], ws[k], X[k])) <= RHO_MAX
    # info == NULL and sweeps == NULL are allowed
    Y = [b.copy(order="F") for b in given]
    rc, _, _ = raw_eigh(CODE[np.dtype(dtype)], Y, [b.shape[0] for b in Y], [b.shape[0] for b in Y], ws, info=False, sweeps=False)
    assert rc == 0 and all(Y[k].tobytes() == X[k].tobytes() for k in range(5))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_ties_small_cases_and_asymmetry(bsm, dtype):
    real = real_of(dtype)
    # a diagonal block with repeated entries: the eigenvectors are the unit vectors in the stable order of the diagonal
    d = np.array([2, -1, 2, 0, -1, 2, 0, 5, -1], dtype=np.float64)
    w, info = bsm.eigh_blocks([X := np.asfortranarray(np.diag(d).astype(dtype))])
    order = np.argsort(d, kind="stable")
    assert info.tolist() == [0] and w[0].dtype == real and np.array_equal(w[0], d[order])
    assert np.array_equal(X, np.eye(9, dtype=dtype)[:, order])
    # [[0, 1], [1, 0]] -> -1, 1
    w, info, sweeps = bsm.eigh_blocks([X := np.asfortranarray(np.array([[0, 1], [1, 0]], dtype=dtype))], sweeps=True)
    assert info.tolist() == [0] and sweeps.tolist() == [1] and np.allclose(w[0], [-1, 1], rtol=0, atol=4 * np.finfo(real).eps)
    assert max(figures(np.array([[0, 1], [1, 0]], dtype=dtype), w[0], X)) <= RHO_MAX
    # rounding-level asymmetry (and a complex diagonal): what is decomposed is the symmetrised block
    rng = np.random.default_rng(3820)
    H = matrix(rng, "uniform", 17, dtype)
    B = (H * (1 + 8 * np.finfo(real).eps * uniform(rng, (17, 17), np.float64))).astype(dtype)
    if np.dtype(dtype).kind == "c":
        B[np.arange(17), np.arange(17)] += 1j * uniform(rng, 17, np.float64).astype(real)
    assert not np.array_equal(B, B.conj().T)
    w, info = bsm.eigh_blocks([X := B.copy(order="F")])
    tw, tV, _, _ = eigh_twin(B)
    assert info.tolist() == [0] and max(figures(B, w[0], X)) <= RHO_MAX and max(figures(B, tw, tV)) <= 1.0
    # the Python entry: views of one flat array, empty input, the operand rules of invert_blocks
    Xs = [matrix(rng, "uniform", n, dtype) for n in (0, 1, 9)]
    w, info = bsm.eigh_blocks(Xs)
    assert [len(x) for x in w] == [0, 1, 9] and w[2].base is w[1].base and info.dtype == np.int64 and info.tolist() == [0, 0, 0]
    w, info = bsm.eigh_blocks([])
    assert w == [] and info.shape == (0,)
    with pytest.raises(ValueError):
        bsm.eigh_blocks([np.zeros((2, 3), dtype=dtype, order="F")])
    with pytest.raises(TypeError):
        bsm.eigh_blocks([np.zeros((3, 3), dtype=dtype)[::-1].T[:, :2][:2]])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_spectral_blocks_host_route(bsm, dtype):
    rng = np.random.default_rng(3830 + CODE[np.dtype(dtype)])
    real, code = real_of(dtype), CODE[np.dtype(dtype)]
    # exact on integer data: V integer-valued (not orthogonal), small integer w, func = values
    ns = (0, 1, 3, 17, 64)
    V = [np.asfortranarray(rng.integers(-3, 4, (n, n)).astype(dtype)) for n in ns]
    if np.dtype(dtype).kind == "c":
        V = [np.asfortranarray(v + 1j * rng.integers(-3, 4, v.shape)).astype(dtype) for v in V]
    w = [rng.integers(-4, 5, n).astype(real) for n in ns]
    out, info = bsm.spectral_blocks(V, w, func="values")
    assert not info.any()
    for v, x, o in zip(V, w, out):
        want = (v.astype(wide_of(dtype)) * x[None, :].astype(np.float64)) @ v.astype(wide_of(dtype)).conj().T
        assert o.dtype == np.dtype(dtype) and o.flags.f_contiguous and np.array_equal(o.astype(want.dtype), want)
    # random data in NaN-guarded padded buffers: the fma bound, bit-Hermitian output, nothing outside the windows
    ns = (1, 3, 17, 65)
    V = [np.asfortranarray(uniform(rng, (n, n), dtype)) for n in ns]
    w = [rng.uniform(-2, 2, n).astype(real) for n in ns]
    for func in ("values", "inv", "absinv", "pinv"):
        bufs = [padded(np.zeros((n, n), dtype), 2) for n in ns]
        before = [outside(buf, n, n + 2) for (buf, _), n in zip(bufs, ns)]
        rc, info = raw_spectral(code, V, ns, ns, w, FUNC[func], 0.25, [b for b, _ in bufs], [n + 2 for n in ns])
        assert rc == 0 and not info.any()
        for (buf, view), v, x, n, was in zip(bufs, V, w, ns, before):
            assert outside(buf, n, n + 2) == was
            worst = check_spectral(view, v, f_of(x, func, 0.25).astype(real), (func, n))
            print(f"  spectral host {np.dtype(dtype).name} {func} n {n}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_func_and_rcond_on_a_hand_made_spectrum(bsm, dtype):
    """{0, 0, 0} U +-[1, 2]: an explicit rcond (the default of pinv would sit inside the rounding of computed zeros)"""
    real, code = real_of(dtype), CODE[np.dtype(dtype)]
    rcond = 1e-3 if real == np.float32 else 1e-8
    w = np.array([-2, -1.5, -1, 0, 0, 0, 1, 1.25, 2], dtype=real)
    n = len(w)
    Q = np.asfortranarray(np.linalg.qr(uniform(np.random.default_rng(3840), (n, n), wide_of(dtype)))[0].astype(dtype))

    def run(func, x=w, rc_=rcond):
        out = np.full((n, n), 7, dtype=dtype, order="F")
        rc, info = raw_spectral(code, [Q], [n], [n], [x], FUNC[func], rc_, [out], [n])
        assert rc == 0
        return out, int(info[0])
    out, info = run("pinv")
    assert info == 0
    check_spectral(out, Q, np.array([-0.5, -1 / 1.5, -1, 0, 0, 0, 1, 0.8, 0.5], real), "pinv")
    out, info = run("absinv")
    assert info == 0 and np.all(np.linalg.eigvalsh(out.astype(wide_of(dtype))) > 0)
    check_spectral(out, Q, (1 / np.maximum(np.abs(w.astype(np.float64)), rcond * 2)).astype(real), "absinv")
    out, info = run("absinv", rc_=0.0)
    assert info == 4 and np.all(out == 7)  # the first zero eigenvalue, 1-based; out not written
    out, info = run("inv")
    assert info == 4 and np.all(out == 7)
    out, info = run("pinv", rc_=0.0)  # |0| > 0 is false: dropped without a bound
    assert info == 0
    check_spectral(out, Q, np.array([-0.5, -1 / 1.5, -1, 0, 0, 0, 1, 0.8, 0.5], real), "pinv rcond 0")
    out, info = run("pinv", rc_=0.6)  # bound 1.2: the three eigenvalues of magnitude 1 go too
    check_spectral(out, Q, np.array([-0.5, -1 / 1.5, 0, 0, 0, 0, 0, 0.8, 0.5], real), "pinv rcond 0.6")
    bad = w.copy()
    bad[6] = np.nan
    for func in ("inv", "absinv", "pinv"):
        assert run(func, bad, 0.5)[1] == (4 if func == "inv" else 7), func
    assert run("values", bad)[1] == 0
    # the neighbours of a bad block are done
    good = np.array([1, 2, 3, 4, 5, 6, 7, 8, 9], real)
    outs = [np.full((n, n), 7, dtype=dtype, order="F") for _ in range(3)]
    rc, info = raw_spectral(code, [Q, Q, Q], [n] * 3, [n] * 3, [good, w, good], FUNC["inv"], 0.0, outs, [n] * 3)
    assert rc == 0 and info.tolist() == [0, 4, 0] and np.all(outs[1] == 7) and outs[0].tobytes() == outs[2].tobytes()
    check_spectral(outs[0], Q, 1 / good, "neighbour")


def test_refusals_leave_the_buffers_untouched(bsm):
    from bsm_amd import _lib as L
    rng = np.random.default_rng(3850)
    a, b = matrix(rng, "uniform", 3, np.float64), matrix(rng, "uniform", 5, np.float64)

    def refused(blocks, n, ld, want=-1, code=1, w=None, **kw):
        bufs = [x.copy(order="F") if isinstance(x, np.ndarray) else x for x in blocks]
        ws = [np.full(max(k, 1), 3.0) for k in n] if w is None else w
        rc, info, sweeps = raw_eigh(code, bufs, n, ld, ws, **kw)
        assert rc == want, (rc, want)
        assert L.lib().bsm_last_error()
        assert np.all(info == -77) and np.all(sweeps == -77), "info was written by a refused call"
        assert all(x is None or np.all(x == 3.0) for x in ws)
        for x, y in zip(bufs, blocks):
            if isinstance(x, np.ndarray):
                assert x.tobytes() == y.tobytes()

    assert raw_eigh(1, [a.copy(order="F"), b.copy(order="F")], [3, 5], [3, 5], [np.zeros(3), np.zeros(5)])[0] == 0
    for name in ("blocks", "n", "ld", "w"):
        refused([a, b], [3, 5], [3, 5], null=(name,))
    refused([a, b], [3, 5], [3, 5], nblocks=-1)
    refused([a, b], [3, -5], [3, 5])
    refused([a, b], [3, 5], [3, 4])
    refused([a, None], [3, 0], [3, 0])
    refused([a, None], [3, 5], [3, 5])
    refused([a, b], [3, 5], [3, 5], w=[np.full(3, 3.0), None])  # a NULL w with n > 0
    for code in (4, 5, -1, 6):
        refused([a, b], [3, 5], [3, 5], code=code)
    refused([a, b], [3, 5], [3, 5], memspace=2)
    big = np.zeros((513, 513), order="F")
    refused([a, big], [3, 513], [3, 513], want=-2)  # BSM_ERR_UNSUPPORTED, and block 1 is not decomposed first
    assert raw_eigh(1, [], [], [], [], null=("blocks", "n", "ld", "w"))[0] == 0
    rc, info, _ = raw_eigh(1, [None, a.copy(order="F")], [0, 3], [1, 3], [None, np.zeros(3)])
    assert rc == 0 and info.tolist() == [0, 0]

    # bsm_spectral_blocks
    wa, wb = np.ones(3), np.ones(5)

    def srefused(V, n, ldv, w, out_ld, want=-1, code=1, func=1, rcond=0.0, **kw):
        outs = [np.full((max(k, 1), max(k, 1)), 7.0, order="F") for k in n]
        rc, info = raw_spectral(code, V, n, ldv, w, func, rcond, outs, out_ld, **kw)
        assert rc == want, (rc, want)
        assert L.lib().bsm_last_error()
        assert np.all(info == -77) and all(np.all(o == 7.0) for o in outs)

    outs = [np.zeros((3, 3), order="F"), np.zeros((5, 5), order="F")]
    assert raw_spectral(1, [a, b], [3, 5], [3, 5], [wa, wb], 1, 0.0, outs, [3, 5])[0] == 0
    for name in ("V", "n", "ldv", "w", "out", "ldo"):
        srefused([a, b], [3, 5], [3, 5], [wa, wb], [3, 5], null=(name,))
    srefused([a, b], [3, 5], [3, 5], [wa, wb], [3, 5], rcond=-1e-3)
    srefused([a, b], [3, 5], [3, 5], [wa, wb], [3, 5], rcond=float("nan"))
    srefused([a, b], [3, 5], [3, 5], [wa, wb], [3, 5], func=4)
    srefused([a, b], [3, 5], [3, 5], [wa, wb], [3, 5], func=-1)
    srefused([a, b], [3, 5], [3, 5], [wa, wb], [3, 4])   # ldo < n
    srefused([a, b], [3, 5], [2, 5], [wa, wb], [3, 5])   # ldv < n
    srefused([a, b], [3, 5], [3, 5], [wa, None], [3, 5])
    srefused([a, b], [3, 5], [3, 5], [wa, wb], [3, 5], code=4)
    srefused([a, b], [3, 5], [3, 5], [wa, wb], [3, 5], memspace=-1)
    srefused([a, big], [3, 513], [3, 513], [wa, np.ones(513)], [3, 513], want=-2)
    with pytest.raises(ValueError):
        bsm.spectral_blocks([a], [wa], func="sqrt")
    with pytest.raises(TypeError):
        bsm.spectral_blocks([a], [wa.astype(np.float32)])


@pytest.mark.parametrize("kind, dtype", CASES, ids=CASE_IDS)
def test_abs_block_jacobi_of_an_analysis_only_handle(bsm, kind, dtype):
    p, _, sets, D, _, _ = minres_problem(kind, dtype)
    A = bsm.synthetic.build(p, device=NODEV)
    M = bsm.block_jacobi(A, sets, kind="abs")
    assert isinstance(M, bsm.BlockJacobi) and M.device is None and M.kind == "abs" and M.rcond == 0.0 and M.source is A
    check_spectral_jacobi(bsm, M, D, sets, "absinv", 0.0, f"abs {kind} {np.dtype(dtype).name}")
    # the eigenvalues tell the inertia: D = W (S + s J) W with J = +-1 by set
    assert len(M.eigenvalues) == len(sets)
    for k, w in enumerate(M.eigenvalues):
        assert len(w) == len(sets[k]) and np.all(np.asarray(w) > 0 if k % 2 == 0 else np.asarray(w) < 0), k
    # positive definite, whatever the signs of the blocks
    Md = dense_of([np.asarray(bsm.block(M, s + 1)) for s in range(len(sets))], sets, NCG)
    assert np.all(np.linalg.eigvalsh(Md.astype(wide_of(dtype))) > 0)
    with pytest.raises(ValueError):
        bsm.block_jacobi(A, sets, kind="inverse", rcond=0.1)
    with pytest.raises(ValueError):
        bsm.block_jacobi(A, sets, kind="sqrt")
    with pytest.raises(ValueError):
        bsm.block_jacobi(A, sets, kind="abs", rcond=-1.0)


@pytest.mark.parametrize("kind", KINDS)
def test_kind_inverse_is_the_route_of_invert_blocks(bsm, kind):
    p, sets = jacobi_problem(np.random.default_rng(3860), kind, np.float64)
    A = bsm.synthetic.build(p, device=NODEV)
    M = bsm.block_jacobi(A, sets, kind="inverse")
    assert M.kind == "inverse" and M.rcond is None and M.eigenvalues is None
    blocks = bsm.submatrices(A, sets)
    assert not bsm.invert_blocks(blocks).any()
    assert all(np.ascontiguousarray(bsm.block(M, s + 1)).tobytes() == np.ascontiguousarray(b).tobytes() for s, b in enumerate(blocks))
    assert all(np.ascontiguousarray(bsm.block(bsm.block_jacobi(A, sets), s + 1)).tobytes() == np.ascontiguousarray(b).tobytes()
               for s, b in enumerate(blocks))


@pytest.mark.parametrize("kind, dtype", CASES, ids=CASE_IDS)
def test_pinv_takes_the_rank_deficient_block_abs_refuses(bsm, kind, dtype):
    p, sets, D, k = rank_deficient(kind, dtype)
    A = bsm.synthetic.build(p, device=NODEV)
    M = bsm.block_jacobi(A, sets, kind="pinv")
    rcond = float(np.sqrt(np.finfo(real_of(dtype)).eps))
    assert M.kind == "pinv" and M.rcond == rcond
    check_spectral_jacobi(bsm, M, D, sets, "pinv", rcond, f"pinv {kind} {np.dtype(dtype).name}")
    assert np.linalg.matrix_rank(np.asarray(bsm.block(M, k + 1)).astype(wide_of(dtype)), tol=1e-3) == 5
    # kind="abs" cannot tell three of the eigenvalues from zero and says so, naming the set; a clamp takes them
    with pytest.raises(np.linalg.LinAlgError, match=rf"set {k + 1} "):
        bsm.block_jacobi(A, sets, kind="abs")
    Mc = bsm.block_jacobi(A, sets, kind="abs", rcond=1e-3)
    assert Mc.kind == "abs" and Mc.rcond == 1e-3
    assert np.all(np.linalg.eigvalsh(np.asarray(bsm.block(Mc, k + 1)).astype(wide_of(dtype))) > 0)
    # an all-zero block: its first eigenvalue is named; the pseudo-inverse of zero is zero
    z = D.copy()
    z[np.ix_(sets[k] - 1, sets[k] - 1)] = 0
    Z = bsm.synthetic.build(cut_operator(kind, z, sets), device=NODEV)
    with pytest.raises(np.linalg.LinAlgError, match=rf"eigenvalue 1 .*set {k + 1} "):
        bsm.block_jacobi(Z, sets, kind="abs")
    assert not np.asarray(bsm.block(bsm.block_jacobi(Z, sets, kind="pinv"), k + 1)).any()


def test_refresh_keeps_the_kind_and_leaves_m_untouched_when_it_raises(bsm):
    kind, dtype = "blocksparse", np.float64
    _, _, sets, D, _, _ = minres_problem(kind, dtype)
    k = [i for i, s in enumerate(sets) if len(s) == 8][0]
    # (a cut of its own: update_blocks writes into the arrays a host handle was built from, and minres_problem's are shared)
    A = bsm.synthetic.build(cut_operator(kind, D, sets), device=NODEV)
    M = bsm.block_jacobi(A, sets, kind="abs")
    kept = [id(b) for b in M.blocks]
    was = [np.array(b, copy=True) for b in M.blocks]
    was_w = [np.array(w, copy=True) for w in M.eigenvalues]
    z = D.copy()
    z[np.ix_(sets[k] - 1, sets[k] - 1)] = 0
    bsm.update_blocks(A, src_list(cut_operator(kind, z, sets)))
    with pytest.raises(np.linalg.LinAlgError, match=rf"set {k + 1} "):
        M.refresh()
    assert M.kind == "abs" and all(a.tobytes() == np.asarray(b).tobytes() for a, b in zip(was, M.blocks))
    assert all(np.array_equal(a, b) for a, b in zip(was_w, M.eigenvalues))
    D2 = (-0.5 * D).astype(dtype)
    bsm.update_blocks(A, src_list(cut_operator(kind, D2, sets)))
    M.refresh()
    assert M.kind == "abs" and [id(b) for b in M.blocks] == kept
    check_spectral_jacobi(bsm, M, D2, sets, "absinv", 0.0, "abs after refresh")
    assert all(np.all(np.asarray(w) < 0 if s % 2 == 0 else np.asarray(w) > 0) for s, w in enumerate(M.eigenvalues))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_the_twin_converges_with_the_abs_preconditioner(dtype):
    """status 0 on every column where the block inverse of D itself breaks down at once (BROKEN_COUNTS of _minres.py)"""
    _, _, sets, D, _, B = minres_problem("vbcrs", dtype)
    Minv, _ = abs_minv(D, sets)
    runs = [minres_twin(D, B[:, c], Minv, rtol_of(dtype), 0.0, 200, dtype) for c in range(NB)]
    print(f"EIGHSTAT minres twin abs {np.dtype(dtype).name}: statuses {[r.status for r in runs]}, counts {[r.iterations for r in runs]}")
    assert [r.status for r in runs] == [0] * NB
    assert [r.iterations for r in runs] == ABS_COUNTS[np.dtype(dtype).name]


def test_the_prototypes_are_declared_and_bound():
    from bsm_amd import _lib as L
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    flat = re.sub(r"\s+", " ", open(os.path.join(root, "include", "bsm_rocm.h")).read())
    assert ("int bsm_eigh_blocks(int dtype, int64_t nblocks, void *const *blocks, const int64_t *n, const int64_t *ld, "
            "void *const *w, int32_t vectors, int64_t *info, int32_t *sweeps, int memspace, void *stream);") in flat
    assert ("int bsm_spectral_blocks(int dtype, int64_t nblocks, const void *const *V, const int64_t *n, const int64_t *ldv, "
            "const void *const *w, int32_t func, double rcond, void *const *out, const int64_t *ldo, int64_t *info, int memspace, "
            "void *stream);") in flat
    assert f"#define BSM_EIGH_LDS_BYTES {L.BSM_EIGH_LDS_BYTES} " in flat and f"#define BSM_EIGH_MAX_N {L.BSM_EIGH_MAX_N}" in flat
    assert f"#define BSM_EIGH_MAX_SWEEPS {L.BSM_EIGH_MAX_SWEEPS}" in flat
    assert "enum { BSM_SPEC_VALUES = 0, BSM_SPEC_INV = 1, BSM_SPEC_ABSINV = 2, BSM_SPEC_PINV = 3 };" in flat
    assert (L.BSM_SPEC_VALUES, L.BSM_SPEC_INV, L.BSM_SPEC_ABSINV, L.BSM_SPEC_PINV) == (0, 1, 2, 3)
    lib = L.lib()
    PP, IP = C.POINTER(C.c_void_p), C.POINTER(C.c_int64)
    assert {"bsm_eigh_blocks", "bsm_spectral_blocks"} <= set(L.EXPORTS)
    assert lib.bsm_eigh_blocks.restype is C.c_int and list(lib.bsm_eigh_blocks.argtypes) == [
        C.c_int, C.c_int64, PP, IP, IP, PP, C.c_int32, IP, C.POINTER(C.c_int32), C.c_int, C.c_void_p]
    assert lib.bsm_spectral_blocks.restype is C.c_int
    assert len(BATCH_CLASSES) == 12
