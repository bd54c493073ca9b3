"""GPU suite of bsm_lsqr_solve / Lsqr: LSQR on several right-hand sides in lockstep against the numpy twin of tests/_lsqr.py
(same recurrences, none of the code) on rectangular operators -- counts and the true stopping criteria on the order-600 x
400 problems, the iterate after four iterations on TWO grids at once (the vectors of B's and of X's length) to MARGIN times
what the twin moves under permuted sums, the decisions and the freezing of finished columns, guarded buffers, the operator /
vector pairings and surfaces, and the refusals.  The twin itself is tested in test_lsqr_cpu.py.  The figures are printed in
LSSTAT lines before they are asserted."""
import ctypes as C

import numpy as np
import pytest

from _bicgstab import bicgstab_problem
from _cg import ERR_DEVICE, ERR_INVALID, ERR_UNSUPPORTED, MAX_RHS, is_complex
from _ctors import ctor_build
from _gpu import dev_copy, dev_mat, outside_bytes, torch_cuda  # noqa: F401
from _jacobi import CODE, uniform
from _lockstep import COLUMNS, MARGIN, RANGE_BYTES, deviation, krylov_grid, reference_of, staggered6
from _lsqr import (LSQR_ITS, M600, N400, NB, check_columns, check_products, history_unit, lsqr_problem, lsqr_rtol, lsqr_spread, lsqr_twin, raw_lsqr_create,
                   raw_lsqr_destroy, raw_lsqr_solve, singular_symmetric, tall_case, true_criteria)
from _values import copied

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64, np.complex64, np.complex128]
_twins, _built, _refs, _spreads = {}, {}, {}, {}


def name(dtype):
    return np.dtype(dtype).name


# ---- 1. the order-600 x 400 problems ------------------------------------------------------------------------------------------
LEGS = ["consistent", "inconsistent", "adjoint", "transpose"]
CASES = [(k, dt, leg) for k in ("vbcrs", "blocksparse") for dt in DTYPES for leg in LEGS if not (leg == "transpose" and is_complex(dt))]


def leg_of(dtype, leg):
    """(dense operator of the system, B, rule the columns end by)"""
    _, A, _, Bc, Bi, Bu = lsqr_problem("vbcrs", dtype)
    return {"consistent": (A, Bc, 1), "inconsistent": (A, Bi, 2), "adjoint": (A.conj().T, Bu, 1), "transpose": (A.T, Bu, 1)}[leg]


def twins(dtype, leg, damp=0.0):
    """the twin's run per column: the dense operator does not depend on its cut, so the reference is computed once per type"""
    key = (name(dtype), "adjoint" if leg == "transpose" else leg, damp)  # (real types: A^T is A^H)
    if key not in _twins:
        A, B, _ = leg_of(dtype, leg)
        r = lsqr_rtol(dtype)
        _twins[key] = [lsqr_twin(A, B[:, c], r, 0.0, r, damp, 400, dtype) for c in range(NB)]
    return _twins[key]


def wrapped(bsm, H, leg):
    return {"adjoint": bsm.adjoint, "transpose": bsm.transpose}.get(leg, lambda a: a)(H)


@pytest.mark.parametrize("kind, dtype, leg", CASES, ids=[f"{k}-{name(dt)}-{leg}" for k, dt, leg in CASES])
def test_against_the_twin(torch_cuda, bsm, kind, dtype, leg):
    torch = torch_cuda
    A, B, rule = leg_of(dtype, leg)
    r = lsqr_rtol(dtype)
    H = bsm.synthetic.build(lsqr_problem(kind, dtype)[0])
    S = bsm.Lsqr(wrapped(bsm, H, leg), nrhs=NB)
    X, info = S.solve(dev_copy(torch, B), rtol=r, ntol=r, maxiter=400)
    xh = X.cpu().numpy()
    assert xh.shape == (A.shape[1], NB)
    runs = twins(dtype, leg)
    check_columns(info, runs, A, xh, B, r, r, f"{kind}-{name(dtype)}-{leg}", rule)
    assert info.history.shape == (info.iterations, NB)
    for c in range(NB):
        k = int(info.column_iterations[c])
        assert info.history[k - 1, c] == info.residual[c] and info.normal_residual[c] >= 0 and info.anorm[c] > 0
        assert abs(info.bnorm[c] - np.linalg.norm(B[:, c].astype(np.complex128))) <= M600 * np.finfo(dtype).eps * info.bnorm[c]
        assert abs(info.anorm[c] - runs[c].anorm) <= 0.05 * runs[c].anorm  # (one iteration more or less moves it by 1 / 75)
    if leg == "adjoint":  # the minimum-norm solution, within 4 x the twin's own distance to it
        ref = np.linalg.pinv(A.astype(np.complex128)) @ B.astype(np.complex128)
        for c in range(NB):
            own = np.linalg.norm(runs[c].x - ref[:, c])
            got = np.linalg.norm(xh[:, c] - ref[:, c])
            print(f"LSSTAT {kind}-{name(dtype)} column {c}: distance to the pseudo-inverse solution {got:.3e}, the twin's {own:.3e}")
            assert got <= 4 * own
    es = np.dtype(dtype).itemsize
    assert info.workspace != 0 and info.workspace_bytes >= (4 * A.shape[1] + 2 * A.shape[0]) * NB * es


# ---- 2. two grids at once: iterate and history after 4 iterations -----------------------------------------------------------
def r0_of(dtype):
    return RANGE_BYTES // np.dtype(dtype).itemsize


# (m in R0 and rows more, n in R0 and rows more (R0 = 0: the count itself), through adjoint, Gm, Gn of the SYSTEM, double types only)
SHAPES = [((1, 1), (0, 40), False, 2, 1, False), ((1, 1), (0, 40), True, 1, 2, False), ((2, 3), (1, 1), False, 3, 2, False),
          ((64, 1), (32, 0), False, 65, 32, False), ((256, 1), (1, 1), False, 256, 2, True)]


def grid_cases():
    out = []
    for dt in DTYPES:
        r0 = r0_of(dt)
        for (ma, mb), (na, nb), flip, gm, gn, wide_only in SHAPES:
            if wide_only and np.finfo(dt).eps > 1e-10:
                continue
            for k in COLUMNS:
                out.append((dt, ma * r0 + mb, na * r0 + nb, flip, gm, gn, k))
    return out


GRID = grid_cases()


def operator(bsm, m, n, dtype, zero_rows=0):
    key = (m, n, name(dtype), zero_rows)
    if key not in _built:
        _built[key] = bsm.synthetic.build(tall_case(m, n, dtype, zero_rows)[0])
    return _built[key]


def solve_in_guarded_buffers(torch, S, B, n, kmax, X0=None, **kw):
    """the solve with B (m rows) at ldb = m + 3 and X (n rows) one element past a 16-byte boundary (ldx = n + 1, kmax columns of
    room), both inside NaN-filled buffers: padding, guard elements, the columns beyond nrhs and B itself must keep their
    bytes.  X0: an initial guess, handed over IN that X buffer"""
    m, k = B.shape
    bbuf, bview = dev_mat(torch, B, pad=3, guard=5)
    xfill = np.full((n, kmax), np.nan, dtype=B.dtype)
    if X0 is not None:
        xfill[:, :k] = X0
    xbuf, xall = dev_mat(torch, xfill, pad=1, off=1, guard=5)
    xview = xall[:, :k]
    before = (outside_bytes(bbuf, m, m + 3, k), outside_bytes(xbuf, n, n + 1, k, off=1), bbuf.cpu().numpy().tobytes())
    X, info = S.solve(bview, X=xview, X0=None if X0 is None else xview, **kw)
    torch.cuda.synchronize()
    assert outside_bytes(bbuf, m, m + 3, k) == before[0], "the padding of B was written"
    assert outside_bytes(xbuf, n, n + 1, k, off=1) == before[1], "X was written outside its n x nrhs window"
    assert bbuf.cpu().numpy().tobytes() == before[2], "B was written"
    return X.cpu().numpy(), info


def check_iterates(tag, info, xh, op, B, dtype, k, X0=None, damp=0.0):
    """every column of a solve cut at LSQR_ITS iterations with rtol = ntol = 0: status 1, count LSQR_ITS, x and the history within
    MARGIN x spread of the reference's (the twin on the operator and right-hand side as rounded to dtype, evaluated in
    reference_of(dtype)); references and the spread (of column 0) are computed once per tag.  A history spread of exactly 0
    is replaced by one rounding unit (_lsqr.history_unit, which says why); every other spread is used as it is"""
    if tag not in _spreads:
        sx, sh = lsqr_spread(op, B[:, 0], LSQR_ITS, dtype, x0=None if X0 is None else X0[:, 0], damp=damp)
        _spreads[tag] = (sx, history_unit(sh))
    sx, sh = _spreads[tag]
    devs = []
    for c in range(k):
        if (tag, c) not in _refs:
            _refs[tag, c] = lsqr_twin(op, B[:, c], 0.0, 0.0, 0.0, damp, LSQR_ITS, reference_of(dtype), x0=None if X0 is None else X0[:, c])
        ref = _refs[tag, c]
        assert ref.status == 1 and ref.iterations == LSQR_ITS
        devs.append(deviation(xh[:, c], info.history[:, c], ref, LSQR_ITS, dtype))
    dx, dh = max(d[0] for d in devs), max(d[1] for d in devs)
    print(f"LSSTAT {tag} K={k}: iterate {dx:.2f} eps max|x|, spread {sx:.2f}, used {dx / (MARGIN * sx):.2f} of the bound; history {dh:.2e} "
          f"eps ||b||, spread {sh:.2e}, used {dh / (MARGIN * sh):.2f}")
    assert info.column_status.tolist() == [1] * k and info.column_iterations.tolist() == [LSQR_ITS] * k, (info.column_status, info.column_iterations)
    assert info.history.shape == (LSQR_ITS, k)
    assert dx <= MARGIN * sx, (tag, [d[0] for d in devs], sx)
    assert dh <= MARGIN * sh, (tag, [d[1] for d in devs], sh)


@pytest.mark.parametrize("dtype, m, n, flip, gm, gn, k", GRID,
                         ids=[f"{name(dt)}-{m}x{n}{'-adjoint' if f else ''}-G{gm}x{gn}-k{k}" for dt, m, n, f, gm, gn, k in GRID])
def test_iterate_and_history_after_four_iterations_on_two_grids(torch_cuda, bsm, dtype, m, n, flip, gm, gn, k):
    es = np.dtype(dtype).itemsize
    _, op, B16, Bt16 = tall_case(m, n, dtype)
    H = operator(bsm, m, n, dtype)
    op, B16, A = (op.H, Bt16, bsm.adjoint(H)) if flip else (op, B16, H)
    rows, cols = op.shape
    assert (krylov_grid(rows, es), krylov_grid(cols, es)) == (gm, gn)
    B = np.asfortranarray(B16[:, :k])
    S = bsm.Lsqr(A, nrhs=MAX_RHS)
    xh, info = solve_in_guarded_buffers(torch_cuda, S, B, cols, MAX_RHS, rtol=0.0, ntol=0.0, maxiter=LSQR_ITS)
    check_iterates(f"{name(dtype)} {rows}x{cols}", info, xh, op, B, dtype, k)
    check_products(info)


# ---- 3. the decisions in one solve ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.complex64], ids=name)
def test_decisions_in_one_solve(torch_cuda, bsm, dtype):
    """seven columns: four consistent ones that finish at different counts under one atol, a zero column, a column with a NaN in
    the last row of B (the last workgroup's range of the m-grid), a column orthogonal to the range of A (nonzero only in rows
    that no block covers: A^H b = 0 exactly).  The handle keeps a second ordering (transpose_image): the adjoint product of a
    block of 129 rows then adds its rows up in one fixed order like the forward one, and two runs of the solve agree to the
    bit; through the first ordering's transposed pass the shares of a column meet in an order that varies from run to run"""
    torch = torch_cuda
    m, n, z = r0_of(dtype) + 1, 40, 8
    p, op, _, _ = tall_case(m, n, dtype, z)
    H = bsm.synthetic.build(p, transpose_image=True)
    assert krylov_grid(m + z, np.dtype(dtype).itemsize) == 2
    rng = np.random.default_rng(77)
    Bc = np.stack([op.astype(dtype).times(uniform(rng, (n,), dtype)).astype(dtype) for _ in range(6)], axis=1)
    tau = 1e-3 if np.finfo(dtype).eps > 1e-10 else 1e-6
    B6, atol = staggered6(Bc, dtype, tau, 4.0 if np.finfo(dtype).eps > 1e-10 else 30.0)  # (twin: 7, 6, 4, 3 / 11, 8, 6, 4 iterations)
    orth = np.zeros((m + z, 1), dtype)
    orth[m:] = 1
    B = np.asfortranarray(np.concatenate([B6, orth], axis=1))
    runs = [lsqr_twin(op, B[:, c], 0.0, atol, 0.0, 0.0, 100, dtype) for c in range(4)]
    assert len({t.iterations for t in runs}) >= 3 and all(t.status == 0 for t in runs)
    S = bsm.Lsqr(H, nrhs=7)
    out = []
    for _ in range(2):
        X, info = S.solve(dev_copy(torch, B), rtol=0.0, atol=atol, ntol=0.0, maxiter=100)
        out.append((X.cpu().numpy(), info))
    (xh, info), (xh2, info2) = out
    print(f"LSSTAT decisions {name(dtype)}: statuses {info.column_status.tolist()}, iterations {info.column_iterations.tolist()}, twin "
          f"{[t.iterations for t in runs]}")
    assert xh.tobytes() == xh2.tobytes() and info.history.tobytes() == info2.history.tobytes()
    assert info.column_iterations.tolist() == info2.column_iterations.tolist()
    assert info.column_status.tolist() == [0, 0, 0, 0, 0, 2, 0]
    for c in range(4):
        assert abs(int(info.column_iterations[c]) - runs[c].iterations) <= 1
        assert true_criteria(op, xh[:, c], B[:, c], atol, 0.0, 0.0)[0] <= 2
    assert info.column_iterations[4] == 0 and not xh[:, 4].any() and info.residual[4] == 0
    assert info.column_iterations[5] == 0 and np.isnan(info.residual[5])
    assert info.column_iterations[6] == 0 and not xh[:, 6].any() and info.normal_residual[6] == 0 and info.residual[6] > 0
    assert info.iterations == max(info.column_iterations) and info.columns_converged == 6 and info.status == 2
    check_products(info)
    # a finished column repeats its last history value while the others run on, and its X keeps its bits: the same solve cut
    # right after the first column finished
    first = int(np.argmin(info.column_iterations[:4]))
    kf = int(info.column_iterations[first])
    assert kf < info.iterations and np.all(info.history[kf - 1:, first] == info.history[kf - 1, first])
    Xc, cut = S.solve(dev_copy(torch, B), rtol=0.0, atol=atol, ntol=0.0, maxiter=kf)
    assert cut.column_status[first] == 0 and Xc.cpu().numpy()[:, first].tobytes() == xh[:, first].tobytes()
    # maxiter cut: the columns still running report status 1 with maxiter iterations
    assert cut.status == 2 and all(cut.column_status[c] == 1 and cut.column_iterations[c] == kf for c in range(4) if info.column_iterations[c] > kf)
    check_products(cut)


# ---- 4. guarded buffers, with and without X0 -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("guess", [False, True], ids=["zero", "x0"])
def test_guarded_buffers(torch_cuda, bsm, dtype, guess):
    r0 = r0_of(dtype)
    m, n = 2 * r0 + 3, r0 + 1
    _, op, B16, _ = tall_case(m, n, dtype)
    B = np.asfortranarray(B16[:, :3])
    X0 = np.asfortranarray(uniform(np.random.default_rng(5), (n, 3), dtype)) if guess else None
    S = bsm.Lsqr(operator(bsm, m, n, dtype), nrhs=MAX_RHS)
    xh, info = solve_in_guarded_buffers(torch_cuda, S, B, n, MAX_RHS, X0=X0, rtol=0.0, ntol=0.0, maxiter=LSQR_ITS)
    check_iterates(f"{name(dtype)} {m}x{n} x0={guess}", info, xh, op, B, dtype, 3, X0=X0)
    check_products(info, guess)


# ---- 5. pairings and surfaces ------------------------------------------------------------------------------------------------------
def solve_600(torch, bsm, A, B, dtype, **kw):
    r = lsqr_rtol(dtype)
    S = bsm.Lsqr(A, nrhs=NB, dtype=dtype)
    X, info = S.solve(dev_copy(torch, B) if torch is not None else B, rtol=r, ntol=r, maxiter=400, **kw)
    return (X.cpu().numpy() if torch is not None else X), info


@pytest.mark.parametrize("rdtype, cdtype", [(np.float32, np.complex64), (np.float64, np.complex128)], ids=["single", "double"])
def test_real_operator_under_complex_vectors(torch_cuda, bsm, rdtype, cdtype):
    p, A, _, _, Bi, _ = lsqr_problem("vbcrs", rdtype)
    B = np.asfortranarray((Bi + 1j * Bi[:, ::-1]).astype(cdtype))
    r = lsqr_rtol(cdtype)
    runs = [lsqr_twin(A.astype(cdtype), B[:, c], r, 0.0, r, 0.0, 400, cdtype) for c in range(NB)]
    xh, info = solve_600(torch_cuda, bsm, bsm.synthetic.build(p), B, cdtype)
    check_columns(info, runs, A.astype(cdtype), xh, B, r, r, f"cvec-{name(cdtype)}", 2)


def test_mixed_storage_handle_solves_in_double(torch_cuda, bsm):
    p, A, _, Bc, _, _ = lsqr_problem("vbcrs", np.float64)
    A32 = A.astype(np.float32).astype(np.float64)  # the operator the handle holds
    r = 1e-8
    runs = [lsqr_twin(A32, Bc[:, c], r, 0.0, r, 0.0, 400, np.float64) for c in range(NB)]
    assert all(t.status == 0 for t in runs)  # (Bc is consistent with A, not with A32: the second rule ends the columns)
    xh, info = solve_600(torch_cuda, bsm, bsm.synthetic.build(p, storage=np.float32), Bc, np.float64)
    check_columns(info, runs, A32, xh, Bc, r, r, "storage-float32", 2)


@pytest.mark.parametrize("kw", [dict(transpose_image=True), dict(accumulate="gather")], ids=["transpose_image", "gather"])
@pytest.mark.parametrize("leg", ["inconsistent", "adjoint"])
def test_handle_options(torch_cuda, bsm, kw, leg):
    dtype = np.float64
    A, B, rule = leg_of(dtype, leg)
    H = bsm.synthetic.build(lsqr_problem("vbcrs", dtype)[0], **kw)
    xh, info = solve_600(torch_cuda, bsm, wrapped(bsm, H, leg), B, dtype)
    check_columns(info, twins(dtype, leg), A, xh, B, 1e-8, 1e-8, f"{list(kw)[0]}-{leg}", rule)


def test_singular_symmetric_operator(torch_cuda, bsm):
    """a real SymmetricBlockMatrix of order 40 and rank 30, Q diag(0 x 10, 1 .. 3) Q^T (_lsqr.singular_symmetric), consistent
    right-hand sides: the fused product serves op(A) and its adjoint.  (On V V^T with V 40 x 30 the twin needs 49 .. 51
    iterations, more than the order: orthogonality is lost and the counts move by 2.)"""
    D, B = singular_symmetric()
    sets = [np.arange(a, a + 10, dtype=np.int64) + 1 for a in range(0, 40, 10)]
    offs, ri, ci = [], [], []
    for a in range(4):
        for b in range(a):
            offs.append(np.asfortranarray(D[np.ix_(sets[a] - 1, sets[b] - 1)]))
            ri.append(sets[a])
            ci.append(sets[b])
    p = dict(kind="symmetric", diagonals=[np.asfortranarray(D[np.ix_(s - 1, s - 1)]) for s in sets], diagonalindices=sets, offdiagonals=offs,
             rowindices=ri, colindices=ci, size=(40, 40))
    r = 1e-8
    runs = [lsqr_twin(D, B[:, c], r, 0.0, r, 0.0, 100, np.float64) for c in range(3)]
    S = bsm.Lsqr(bsm.synthetic.build(p), nrhs=3)
    X, info = S.solve(dev_copy(torch_cuda, B), rtol=r, ntol=r)  # (maxiter defaults to min(m, n) = 40)
    check_columns(info, runs, D, X.cpu().numpy(), B, r, r, "singular symmetric", 1)


def test_square_nonsymmetric_problem(torch_cuda, bsm):
    """cond(D) = 8.3e3 and LSQR works on its square: at rtol = ntol = 1e-4 the twin's columns end by the second rule after 153 ..
    154 iterations (+-1 under permuted sums); to 1e-6 it needs 1357 .. 1367 and the counts move by up to 9"""
    p, _, D, B = bicgstab_problem("vbcrs", np.float64)
    r = 1e-4
    runs = [lsqr_twin(D, B[:, c], r, 0.0, r, 0.0, 400, np.float64) for c in range(B.shape[1])]
    S = bsm.Lsqr(bsm.synthetic.build(p), nrhs=B.shape[1])
    X, info = S.solve(dev_copy(torch_cuda, B), rtol=r, ntol=r)
    check_columns(info, runs, D, X.cpu().numpy(), B, r, r, "bicgstab problem", 2)


@pytest.mark.parametrize("dtype", [np.float64, np.complex64], ids=name)
def test_damped_against_the_closed_form(torch_cuda, bsm, dtype):
    p, A, _, _, Bi, _ = lsqr_problem("blocksparse", dtype)
    r, damp = lsqr_rtol(dtype), 2.0
    runs = twins(dtype, "inconsistent", damp)
    S = bsm.Lsqr(bsm.synthetic.build(p), nrhs=NB)
    X, info = S.solve(dev_copy(torch_cuda, Bi), rtol=r, ntol=r, damp=damp, maxiter=400)
    xh = X.cpu().numpy()
    check_columns(info, runs, A, xh, Bi, r, r, f"damped-{name(dtype)}", 2, damp=damp)
    Aw = A.astype(np.complex128)
    ref = np.linalg.solve(Aw.conj().T @ Aw + damp * damp * np.eye(N400), Aw.conj().T @ Bi.astype(np.complex128))
    for c in range(NB):
        own, got = np.linalg.norm(runs[c].x - ref[:, c]), np.linalg.norm(xh[:, c] - ref[:, c])
        print(f"LSSTAT damped-{name(dtype)} column {c}: distance to the closed form {got:.3e}, the twin's {own:.3e}")
        assert got <= 4 * own


def test_numpy_arrays_a_callers_stream_and_the_one_shot(torch_cuda, bsm):
    torch, dtype = torch_cuda, np.float64
    A, B, rule = leg_of(dtype, "inconsistent")
    runs = twins(dtype, "inconsistent")
    H = bsm.synthetic.build(lsqr_problem("vbcrs", dtype)[0])
    # numpy arrays in: host-staged, numpy out
    xh, info = solve_600(None, bsm, H, B, dtype)
    assert isinstance(xh, np.ndarray) and xh.shape == (N400, NB)
    check_columns(info, runs, A, xh, B, 1e-8, 1e-8, "host", rule)
    # a vector in, a vector out; the one-shot form
    x1, i1 = bsm.lsqr(H, B[:, 0].copy(), rtol=1e-8, ntol=1e-8)
    assert x1.shape == (N400,)
    check_columns(i1, runs[:1], A, x1, B[:, :1], 1e-8, 1e-8, "one-shot vector", rule)
    # a caller's stream
    st = torch.cuda.Stream()
    S = bsm.Lsqr(H, nrhs=NB)
    Bd = dev_copy(torch, B)
    torch.cuda.synchronize()
    X, i2 = S.solve(Bd, rtol=1e-8, ntol=1e-8, maxiter=400, stream=st)
    check_columns(i2, runs, A, X.cpu().numpy(), B, 1e-8, 1e-8, "stream", rule)
    # the under-determined system through the one-shot form on device tensors
    Au, Bu, _ = leg_of(dtype, "adjoint")
    Xu, iu = bsm.lsqr(bsm.adjoint(H), dev_copy(torch, Bu), rtol=1e-8, ntol=1e-8, maxiter=400)
    assert tuple(Xu.shape) == (M600, NB)
    check_columns(iu, twins(dtype, "adjoint"), Au, Xu.cpu().numpy(), Bu, 1e-8, 1e-8, "one-shot adjoint", 1)


def test_one_solver_across_update_blocks(torch_cuda, bsm):
    torch, dtype = torch_cuda, np.float64
    p, A, _, _, Bi, _ = lsqr_problem("vbcrs", dtype)
    H = bsm.synthetic.build(copied(p))  # (update_blocks writes into the blocks a handle was built from; the problem is shared)
    S = bsm.Lsqr(H, nrhs=NB)
    Bd = dev_copy(torch, Bi)
    X, info = S.solve(Bd, rtol=1e-8, ntol=1e-8, maxiter=400)
    check_columns(info, twins(dtype, "inconsistent"), A, X.cpu().numpy(), Bi, 1e-8, 1e-8, "before the update", 2)
    A2 = A.copy()
    # block 1 of the 6 x 4 grid negated: an operator of the same distribution, on which the twin keeps its counts (71, 71, 71,
    # 71, 72 under four permuted orders; with the block tripled they moved by 2).  Stale values show in the true criterion
    A2[:100, :100] = -A[:100, :100]
    bsm.update_blocks(H, [np.asfortranarray(A2[:100, :100])], ids=[1])
    runs = [lsqr_twin(A2, Bi[:, c], 1e-8, 0.0, 1e-8, 0.0, 400, dtype) for c in range(NB)]
    X, info = S.solve(Bd, rtol=1e-8, ntol=1e-8, maxiter=400)
    check_columns(info, runs, A2, X.cpu().numpy(), Bi, 1e-8, 1e-8, "after the update", 2)


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals(torch_cuda, bsm):
    torch, dtype = torch_cuda, np.float64
    from bsm_amd import _lib as L
    f64, c128 = CODE[np.dtype(np.float64)], CODE[np.dtype(np.complex128)]
    p, A, _, _, Bi, _ = lsqr_problem("blocksparse", dtype)
    H = bsm.synthetic.build(p)

    def refused(code, *args):
        rc, out = raw_lsqr_create(*args)
        assert rc == code and not out.value, (args[1:], rc, out.value)

    refused(ERR_INVALID, None, 0, f64, 4)
    assert L.lib().bsm_lsqr_create(H._h.ptr, 0, f64, 4, None) == ERR_INVALID and L.lib().bsm_lsqr_destroy(None) == 0
    for op in (3, -1):
        refused(ERR_INVALID, H, op, f64, 4)
    refused(ERR_INVALID, H, 0, 7, 4)
    for kmax in (0, MAX_RHS + 1):
        refused(ERR_INVALID, H, 0, f64, kmax)
    refused(ERR_INVALID, H, 0, CODE[np.dtype(np.complex64)], 4)  # a real handle of the other precision
    Hc = bsm.synthetic.build(lsqr_problem("vbcrs", np.complex128)[0])
    refused(ERR_INVALID, Hc, 0, f64, 4)  # a complex handle under real vectors
    refused(ERR_UNSUPPORTED, Hc, 1, c128, 4)  # op T on a complex handle: its adjoint is conj(A)
    assert "conj(A)" in L.lib().bsm_last_error().decode()
    with pytest.raises(bsm._lib.BsmError, match="conj"):
        bsm.Lsqr(bsm.transpose(Hc))
    refused(ERR_UNSUPPORTED, ctor_build(bsm, "blocksparse", p, devices=[0, 0]), 0, f64, 4)
    with pytest.raises(bsm._lib.BsmError, match="multi-device"):
        bsm.Lsqr(ctor_build(bsm, "blocksparse", p, devices=[0, 0]))
    refused(ERR_DEVICE, bsm.synthetic.build(p, device=-2), 0, f64, 4)
    pv = lsqr_problem("vbcrs", dtype)[0]
    keep = [i for i, r0 in enumerate(pv["rowstart"]) if 101 <= r0 <= 201]
    sub = dict(kind="vbcrs", blocks=[pv["blocks"][i] for i in keep], rowstart=pv["rowstart"][keep], colstart=pv["colstart"][keep], size=pv["size"])
    refused(ERR_UNSUPPORTED, bsm.synthetic.build(sub, own=(101, 300)), 0, f64, 4)
    assert "own a row range" in L.lib().bsm_last_error().decode()
    for args in ((H, 0, f64), (H, 1, f64), (H, 2, f64), (H, 0, c128), (Hc, 0, c128), (Hc, 2, c128), (bsm.synthetic.build(p, storage=np.float32), 0, f64)):
        rc, ptr = raw_lsqr_create(*args, 4)
        assert rc == 0 and ptr.value and raw_lsqr_destroy(ptr) == 0, args[1:]
    rc, ptr = raw_lsqr_create(H, 0, f64, MAX_RHS)
    assert rc == 0 and ptr.value
    try:
        Bd = dev_copy(torch, np.asfortranarray(np.concatenate([Bi] * 4, axis=1)))  # 20 columns of 600
        Xd = torch.full((20, N400), 7.0, dtype=Bd.dtype, device="cuda").t()
        st = torch.cuda.current_stream().cuda_stream
        b, x, es = Bd.data_ptr(), Xd.data_ptr(), 8
        good = (NB, b, M600, x, N400)
        ok = raw_lsqr_solve(ptr, *good, maxiter=400, stream=st)
        assert ok[0] == 0 and ok[1].status == 0 and np.all(ok[4][:NB] >= 0) and np.all(ok[5][:NB] > 0) and ok[1].a_products == 2 * ok[1].iterations + 1
        Xd.fill_(7.0)
        for what, args, kw in [("nrhs 0", (0, b, M600, x, N400), {}), ("nrhs 17", (17, b, M600, x, N400), {}),
                               ("ldx < n", (NB, b, M600, x, N400 - 1), {}), ("ldb < m", (NB, b, M600 - 1, x, N400), {}),
                               ("ldb = n < m", (NB, b, N400, x, N400), {}), ("X is B", (NB, b, M600, b, N400), {}),
                               ("X overlaps the last column of B", (NB, b, M600, b + (NB * M600 - 8) * es, N400), {}),
                               ("null B", (NB, None, M600, x, N400), {}), ("null X", (NB, b, M600, None, N400), {}),
                               ("negative rtol", good, dict(rtol=-1.0)), ("NaN rtol", good, dict(rtol=float("nan"))),
                               ("negative atol", good, dict(atol=-1e-3)), ("NaN atol", good, dict(atol=float("nan"))),
                               ("negative ntol", good, dict(ntol=-1e-3)), ("NaN ntol", good, dict(ntol=float("nan"))),
                               ("negative damp", good, dict(damp=-2.0)), ("NaN damp", good, dict(damp=float("nan"))),
                               ("negative maxiter", good, dict(maxiter=-1, capacity=0)), ("bad memspace", good, dict(memspace=2)),
                               ("struct size of bsm_cg_params", good, dict(struct_size=40)), ("struct size", good, dict(struct_size=8))]:
            assert raw_lsqr_solve(ptr, *args, stream=st, **kw)[0] == ERR_INVALID, what
        assert raw_lsqr_solve(None, *good, stream=st)[0] == ERR_INVALID  # null S
        # a capturing stream
        torch.cuda.synchronize()
        scratch = torch.zeros(4, device="cuda")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            scratch.zero_()
            rc = raw_lsqr_solve(ptr, *good, stream=torch.cuda.current_stream().cuda_stream)[0]
            why = L.lib().bsm_last_error().decode()
        assert rc == ERR_INVALID and "graph-captured" in why
        torch.cuda.synchronize()
        assert bool((Xd == 7.0).all()), "a refused solve wrote X"
        # X just behind the columns of B that are read is no overlap; no columns / history / estimates
        prm = L.BsmLsqrParams(C.sizeof(L.BsmLsqrParams), 0, 1e-8, 0.0, 1e-8, 0.0, 400, 0)
        info = L.BsmCgInfo()
        assert L.lib().bsm_lsqr_solve(ptr, NB, b, M600, b + NB * M600 * es, N400, C.byref(prm), C.byref(info), None, None, None, None, 1, st) == 0
        assert info.status == 0 and info.columns_converged == NB and info.iterations == ok[1].iterations
    finally:
        assert raw_lsqr_destroy(ptr) == 0
    # Python: the operands' lengths
    S = bsm.Lsqr(H, nrhs=2)
    with pytest.raises(ValueError, match="DimensionMismatch"):
        S.solve(torch.zeros((2, N400), dtype=torch.float64, device="cuda").t())
    with pytest.raises(ValueError, match="columns"):
        S.solve(dev_copy(torch, Bi))
    # m == 0 or n == 0: status 0, nothing touched, B and X may be null
    for shape in ((0, 0), (0, 5), (5, 0)):
        rc, ptr = raw_lsqr_create(bsm.BlockSparseMatrix([], [], [], shape), 0, f64, 2)
        assert rc == 0
        try:
            rc, info, cols, _, arn, an = raw_lsqr_solve(ptr, 2, None, max(shape[0], 1), None, max(shape[1], 1), stream=torch.cuda.current_stream().cuda_stream)
            assert rc == 0 and info.status == 0 and info.columns_converged == 2 and info.iterations == 0 and not arn[:2].any() and not an[:2].any()
        finally:
            assert raw_lsqr_destroy(ptr) == 0
