"""CPU suite behind test_gpu_lockstep_grid.py: the mirrors of the grid rule say what the kernel source says, every twin run
the GPU file compares against ends the way that file needs it to (so that no GPU test rests on a reference that fails
alone), and the iterate check is SHARP where the older checks are not -- a twin whose forms lose the last workgroup's share
is rejected by `MARGIN x spread` on every (type, n) of the table, and accepted by "count +-1 and true residual <= 2 tol"
on the two large shapes of test_gpu_cg.py / test_gpu_bicgstab.py.  That is the gap the GPU file closes."""
import os
import re

import numpy as np
import pytest

from _bicgstab import edge_problem
from _cg import column_tol, is_complex, spd_problem
from _jacobi import DTYPES, uniform
from _krylov import exact_minv
from _lockstep import (COLUMNS, ITS, MARGIN, MAX_GRID, METHODS, RANGE_BYTES, ROWS, TABLE, TABLE_IDS, block_solve, bnorm_roundings,
                       deviation, grid_case, half_sets, krylov_grid, last_range_rows, path_rtol, reference, rows_of, run_twin, spread, staggered6,
                       workspace_bytes)

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "blocksparsematrices.jl_amd", "csrc")
# the twin's counts on the six columns of test_decisions_across_workgroups (G = 65): four different ones, a zero column, a NaN
STAGGERED = {("cg", "complex128"): [57, 40, 24, 7, 0, 0], ("bicgstab", "complex128"): [69, 47, 25, 7, 0, 0],
             ("cg", "float32"): [19, 15, 10, 6, 0, 0], ("bicgstab", "float32"): [19, 16, 8, 4, 0, 0]}
# the twin's counts on 3 columns in complex128 at G = 2, 3 (n = 513, 1027) and path_rtol = 1e-6: (plain, half-block M, initial
# guess, the float64 operator under complex128 vectors); COCG's: on the complex symmetric problem with CSYM_IMAG = 0.3
PATHS = {("cg", 2): ([32, 32, 32], [25, 25, 25], [24, 24, 24], [24, 24, 24]), ("cg", 3): ([33, 33, 33], [27, 27, 27], [25, 25, 25], [25, 25, 25]),
         ("cocg", 2): ([34, 35, 34], [29, 26, 26], [25, 27, 26], None), ("cocg", 3): ([37, 39, 35], [27, 27, 27], [27, 28, 28], None),
         ("bicgstab", 2): ([31, 32, 32], [21, 21, 22], [25, 23, 23], [21, 21, 22]),
         ("bicgstab", 3): ([33, 34, 34], [20, 20, 22], [23, 24, 24], [22, 23, 22])}
COCG_C64 = {2: [26, 23, 21], 3: [22, 22, 26]}  # complex64, n = 1025, 2051, rtol 1e-4


# ---- the mirrors --------------------------------------------------------------------------------------------------------
def test_the_mirror_is_the_grid_rule_of_the_source():
    src = re.sub(r"\s+", " ", open(os.path.join(CSRC, "bsm_krylov.h")).read())
    assert f"constexpr int kKrylovMaxGrid = {MAX_GRID};" in src
    assert "inline int krylov_grid(long long n, int es) { const long long per = 512LL * (16 / es); const long long g = (n + per - 1) / per;" in src
    assert RANGE_BYTES == 512 * 16
    dev = re.sub(r"\s+", " ", open(os.path.join(CSRC, "bsm_lockstep_device.h")).read())
    assert "const long long per = (ng + G - 1) / G; g0 = per * wg;" in dev and "for (int g = lane; g < G; g += 64)" in dev
    for dt in DTYPES:
        es = np.dtype(dt).itemsize
        r0 = RANGE_BYTES // es
        assert [krylov_grid(n, es) for n in (1, r0, r0 + 1, 255 * r0 + 1, 256 * r0 + 1, 10 ** 7)] == [1, 1, 2, 256, 256, 256]
        assert [G for _, G in rows_of(dt)] == ([2, 3, 64, 65, 256] if np.finfo(dt).eps < 1e-10 else [2, 65, 256])
        assert [n for n, _ in rows_of(dt)] == [a * r0 + b for i, (a, b, _, _) in enumerate(ROWS) if np.finfo(dt).eps < 1e-10 or i in (0, 3, 4)]
    assert max(n for dt, n, _ in TABLE if dt == np.complex128) == 131073 and len(TABLE) == 16 and COLUMNS == [1, 3, 16]
    # per = ceil(groups / G): the last range of the capped row holds 258 complex128 rows, its workgroups walk 513 groups
    assert last_range_rows(131073, 16) == 131073 - 255 * 513 and last_range_rows(513, 16) == 256
    assert [bnorm_roundings(n, dt) for dt, n, _ in TABLE] == [20, 20, 20, 21, 25, 20, 20, 20, 21, 25, 24, 25, 31, 24, 25, 31]
    # the size of the workspace tells G for every row
    for method in ("cg", "bicgstab"):
        for dt, n, G in TABLE:
            assert all(workspace_bytes(method, n, dt, G=g) != workspace_bytes(method, n, dt) for g in (1, G - 1, G + 1))


def test_block_diagonal_products_in_permuted_column_order():
    _, Dop, B = grid_case("cocg", 1027, np.complex64)
    v = B[:, 0]
    a, b = Dop @ v, Dop.times(v, np.random.default_rng(0).permutation(1027))
    assert np.array_equal(a, Dop.times(v)) and np.allclose(a, Dop.dense() @ v, rtol=1e-5)
    assert not np.array_equal(a, b) and np.max(np.abs(a - b)) <= 8 * np.finfo(np.float32).eps * np.max(np.abs(a))
    assert np.allclose(block_solve(Dop, a), v, rtol=1e-4)


# ---- the twins the GPU file relies on -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype, n, G", TABLE, ids=TABLE_IDS)
def test_twins_reach_four_iterations(dtype, n, G):
    for method in METHODS:
        if method == "cocg" and not (is_complex(dtype) and G >= 65):
            continue
        _, Dop, B = grid_case(method, n, dtype)
        ref = reference(method, Dop, B[:, 0], ITS, dtype)
        assert ref.status == 1 and ref.iterations == ITS and np.all(np.isfinite(ref.history)) and np.all(ref.history > 0), method


@pytest.mark.parametrize("dtype", [np.complex128, np.float32], ids=["complex128", "float32"])
@pytest.mark.parametrize("method", ["cg", "bicgstab"])
def test_twins_on_the_staggered_columns(method, dtype):
    n = 64 * (RANGE_BYTES // np.dtype(dtype).itemsize) + 1
    _, Dop, B = grid_case(method, n, dtype)
    tau, step = (1e-4, 10.0) if dtype == np.float32 else (1e-10, 1000.0)
    Bs, atol = staggered6(B, dtype, tau, step)
    assert n - last_range_rows(n, np.dtype(dtype).itemsize) <= n - 1 and np.isnan(Bs[n - 1, 5])  # the NaN: in the last range
    runs = [run_twin(method, Dop, Bs[:, c], dtype, 0.0, 200, atol=atol) for c in range(6)]
    counts = [r.iterations for r in runs]
    assert [r.status for r in runs] == [0, 0, 0, 0, 0, 2] and counts == STAGGERED[method, np.dtype(dtype).name], counts
    assert len(set(counts[:4])) == 4
    order = np.random.default_rng(1).permutation(n)
    assert all(abs(run_twin(method, Dop, Bs[:, c], dtype, 0.0, 200, atol=atol, order=order).iterations - counts[c]) <= 1 for c in range(4))
    Dw = Dop.astype(np.complex128)
    for c in range(4):
        assert float(np.linalg.norm(Bs[:, c].astype(np.complex128) - Dw @ runs[c].x.astype(np.complex128))) <= atol


def path_counts(method, Dop, B, dtype, seed=None, **kw):
    order = None if seed is None else np.random.default_rng(seed).permutation(len(B))
    runs = [run_twin(method, Dop, B[:, c], dtype, path_rtol(dtype), 200, order=order, **{k: (v[:, c] if k == "x0" else v) for k, v in kw.items()})
            for c in range(3)]
    assert all(r.status == 0 for r in runs), (method, seed, list(kw))
    return [r.iterations for r in runs]


@pytest.mark.parametrize("G", [2, 3])
@pytest.mark.parametrize("method", METHODS)
def test_twins_on_the_selected_paths(method, G):
    """complex128 at G = 2, 3: plain, with the half-block preconditioner (not the inverse: 20 .. 29 iterations, fewer than
    plain) and from the initial guess, every run to status 0 -- COCG neither breaks down nor stalls -- with the pinned
    counts, and the same counts +-1 under permuted sums (the GPU file allows the device +-1)"""
    dtype, n = np.complex128, {2: 513, 3: 1027}[G]
    _, Dop, B = grid_case(method, n, dtype)
    Minv = exact_minv(Dop.dense(), half_sets(n))
    sol = block_solve(Dop, B[:, :3])
    X0 = (sol + 1e-2 * np.max(np.abs(sol)) * uniform(np.random.default_rng(8900 + n), sol.shape, dtype)).astype(dtype)
    assert sum(len(s) for s in half_sets(n)) == n and max(len(s) for s in half_sets(n)) == 4
    cases = [(Dop, B, dtype, {}), (Dop, B, dtype, dict(Minv=Minv)), (Dop, B, dtype, dict(x0=X0))]
    if method == "cocg":
        _, D64, B64 = grid_case("cocg", {2: 1025, 3: 2051}[G], np.complex64)
        assert np.array_equal(D64.main, D64.main.transpose(0, 2, 1)) and not np.array_equal(D64.main, D64.main.conj().transpose(0, 2, 1))
        cases.append((D64, B64, np.complex64, {}))
    else:  # the float64 operator under complex128 vectors
        cases.append((grid_case(method, n, np.float64)[1].astype(dtype), grid_case(method, n, dtype)[2], dtype, {}))
    want = list(PATHS[method, G][:3]) + [COCG_C64[G] if method == "cocg" else PATHS[method, G][3]]
    for (D, Bk, dt, kw), counts in zip(cases, want):
        assert path_counts(method, D, Bk, dt, **kw) == counts, (list(kw), np.dtype(dt).name)
        assert all(abs(a - b) <= 1 for a, b in zip(path_counts(method, D, Bk, dt, seed=0, **kw), counts)), list(kw)
        first = run_twin(method, D, Bk[:, 0], dt, 0.0, ITS, **{k: (v[:, 0] if k == "x0" else v) for k, v in kw.items()})
        assert first.status == 1 and first.iterations == ITS
    assert all(m < p for m, p in zip(want[1], want[0])) and min(want[1]) > ITS


# ---- the check is sharp ---------------------------------------------------------------------------------------------------
SHARP = [(m, dt, n, G) for m in METHODS for dt, n, G in TABLE if m == "cg" or dt == np.complex128]


@pytest.mark.parametrize("method, dtype, n, G", SHARP, ids=[f"{m}-{np.dtype(dt).name}-n{n}-G{G}" for m, dt, n, G in SHARP])
def test_a_lost_share_is_rejected_by_the_iterate_check(method, dtype, n, G):
    """the twin IN dtype whose forms lose (1) the last 1 / G of their terms, (2) exactly the rows of the last workgroup's
    range, against the reference and the bound of test_iterate_and_history_after_four_iterations: out by orders of
    magnitude in the iterate or in the history, while the honest twin in dtype (the device's stand-in) is inside.
    CG in all four types, COCG and BiCGSTAB in complex128"""
    _, Dop, B = grid_case(method, n, dtype)
    b = B[:, 0]
    ref = reference(method, Dop, b, ITS, dtype)
    sx, sh = spread(method, Dop, b, ITS, dtype)
    honest = run_twin(method, Dop, b, dtype, 0.0, ITS)
    hx, hh = deviation(honest.x, honest.history, ref, ITS, dtype)
    assert 0 < sx <= 64 and hx <= MARGIN * sx and hh <= MARGIN * sh, (hx, sx, hh, sh)
    for keep in (n - n // G, n - last_range_rows(n, np.dtype(dtype).itemsize)):
        mut = run_twin(method, Dop, b, dtype, 0.0, ITS, keep=keep)
        mx, mh = deviation(mut.x, mut.history, ref, ITS, dtype)
        print(f"LOCKSTAT sharp {method} {np.dtype(dtype).name} n={n} G={G}: {n - keep} terms lost: iterate {mx:.3g} eps max|x| against a "
              f"bound of {MARGIN * sx:.2f}, history {mh:.3g} against {MARGIN * sh:.3g}; honest {hx:.2f}, {hh:.3g}")
        assert mx > 10 * MARGIN * sx or mh > 10 * MARGIN * sh, (keep, mx, sx, mh, sh)


@pytest.mark.parametrize("method, n", [("cg", 300000), ("bicgstab", 600000)], ids=["cg-n300000", "bicgstab-n600000"])
def test_a_lost_share_passes_the_older_large_n_checks(method, n):
    """the shapes of test_a_workgroup_walks_several_tiles in test_gpu_cg.py / test_gpu_bicgstab.py (float64, one column,
    G = 256): the twin whose forms lose the last 1 / 256 of their terms converges in the honest twin's count +-1 to a true
    residual <= 2 tol -- what those tests assert -- although its third iterate is off by 1e9 eps and more"""
    dtype = np.float64
    if method == "cg":
        rng = np.random.default_rng(5100)
        _, Dop = spd_problem(rng, n, dtype)
    else:
        _, Dop, rng = edge_problem(n, dtype)
    b = uniform(rng, (n,), dtype)
    assert krylov_grid(n, 8) == 256
    honest = run_twin(method, Dop, b, dtype, 1e-10, 200)
    lost = run_twin(method, Dop, b, dtype, 1e-10, 200, keep=n - n // 256)
    true = float(np.linalg.norm(b - Dop @ lost.x))
    off = np.max(np.abs(lost.iterates[2] - honest.iterates[2])) / (np.finfo(dtype).eps * np.max(np.abs(honest.iterates[2])))
    print(f"LOCKSTAT old check {method} n={n}: {honest.iterations} iterations, {lost.iterations} with the lost share, true residual / tol "
          f"{true / column_tol(b, 1e-10):.3f}, third iterate off by {off:.3g} eps max|x|")
    assert honest.status == 0 and lost.status == 0 and abs(lost.iterations - honest.iterations) <= 1
    assert true <= 2 * column_tol(b, 1e-10)
    assert off > 1e6
