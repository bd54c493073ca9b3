"""CPU companion of test_gpu_lsqr_handles.py: what that suite takes for granted, shown without a GPU.

  1. The pairs it accepts against.  For every (operand, leg, type) of _lsqr.py's table that the GPU suite solves and that
     test_lsqr_cpu.py does not pin already: the twin's counts as pinned below, its own true criterion <= 1 x the threshold
     (the GPU suite allows 2 x), and the counts of columns 0 and 4 within +-1 under four permuted summation orders.
  2. Stale values are visible: the twin's solution on the old values misses the criterion of the new operator by more than
     100 thresholds and the other way round, on every column of every update leg.
  3. A half refill is visible: with the new values in the forward product and the old ones in the adjoint product (and the
     reverse) -- a transpose_image handle whose refill reached one image -- LSQR does not converge in 400 iterations and
     misses the criterion by more than 100 thresholds.
  4. Every (problem, handle mode) the GPU suite builds exists as an analysis-only handle whose entries, A[I, J] and
     transpose(A)[I, J], read back as the dense operator to the bit (every entry lies in at most one block); the partial
     update of the update legs reaches both images of a transpose_image handle.
Figures are printed in LSHSTAT lines."""
import numpy as np
import pytest

from _cg import is_complex
from _common import NODEV
from _lsqr import (BORDER, LEGS, M600, N400, NB, Half, bordered_problem, largest_row_set, leg_runs, leg_system, lsqr_problem, lsqr_rtol, lsqr_twin,
                   new_values, operand, orders, single_of, symmetric_problem, true_criteria)

DTYPES = [np.float32, np.float64, np.complex64, np.complex128]
WIDE = [np.float64, np.complex128]


def name(dtype):
    return np.dtype(dtype).name


# the twin's iterations on the five columns, rtol = ntol = lsqr_rtol(dtype), maxiter 400
COUNTS = {
    ("cvec", "complex128", "inconsistent"): [73, 72, 71, 72, 73], ("cvec", "complex128", "adjoint"): [84, 83, 83, 83, 84],
    ("cvec", "complex64", "adjoint"): [44, 41, 43, 41, 44],
    ("rounded", "float64", "inconsistent"): [71, 72, 71, 72, 73], ("rounded", "float64", "adjoint"): [81, 81, 83, 82, 83],
    ("rounded", "complex128", "inconsistent"): [71, 71, 71, 71, 72], ("rounded", "complex128", "adjoint"): [82, 81, 84, 84, 83],
    ("bordered", "float64", "inconsistent"): [71, 72, 71, 73, 72], ("bordered", "float64", "adjoint"): [83, 81, 82, 83, 82],
    ("bordered", "complex64", "inconsistent"): [32, 32, 31, 32, 32], ("bordered", "complex64", "adjoint"): [41, 41, 41, 42, 42],
    ("symmetric", "float64", "adjoint"): [27, 27, 27, 27, 27], ("symmetric", "float32", "adjoint"): [14, 14, 14, 14, 14],
    ("vbcrs2", "float32", "inconsistent"): [33, 31, 32, 32, 32], ("vbcrs2", "float32", "adjoint"): [41, 42, 42, 42, 42],
    ("vbcrs2", "float64", "inconsistent"): [71, 71, 71, 71, 72], ("vbcrs2", "float64", "adjoint"): [83, 83, 79, 83, 82],
    ("vbcrs2", "complex64", "inconsistent"): [32, 31, 31, 31, 31], ("vbcrs2", "complex64", "adjoint"): [41, 41, 41, 41, 39],
    ("vbcrs2", "complex128", "inconsistent"): [70, 70, 71, 70, 71], ("vbcrs2", "complex128", "adjoint"): [81, 81, 81, 81, 80],
    ("blocksparse2", "float32", "inconsistent"): [31, 32, 33, 31, 32], ("blocksparse2", "float32", "adjoint"): [44, 40, 43, 41, 41],
    ("blocksparse2", "float64", "inconsistent"): [70, 72, 72, 72, 73], ("blocksparse2", "float64", "adjoint"): [81, 81, 83, 82, 83],
    ("blocksparse2", "complex64", "inconsistent"): [32, 31, 32, 32, 31], ("blocksparse2", "complex64", "adjoint"): [40, 42, 42, 42, 41],
    ("blocksparse2", "complex128", "inconsistent"): [71, 71, 71, 71, 71], ("blocksparse2", "complex128", "adjoint"): [82, 81, 84, 84, 83],
}
DT = {name(d): d for d in DTYPES}
PAIRS = [(n, DT[d], leg) for n, d, leg in COUNTS]
UPDATES = [p for p in PAIRS if p[0] in ("vbcrs2", "blocksparse2")]


def pair_id(p):
    return f"{p[0]}-{name(p[1])}-{p[2]}"


def criterion(A, t, b, r, rule):
    return true_criteria(A, t.x, b, t.tol, r, t.anorm)[rule - 1]


def test_the_base_pairs_are_pinned_elsewhere():
    """the operand `base` IS the order-600 x 400 problem of test_lsqr_cpu.py (its legs "inconsistent" and "under"), and the
    symmetric operand has one system: both legs are (D, B)"""
    for dtype in DTYPES:
        _, A0, _, _, Bi, Bu = lsqr_problem("vbcrs", dtype)
        for leg, want in (("inconsistent", (A0, Bi, 2)), ("adjoint", (A0.conj().T, Bu, 1))):
            A, B, rule = leg_system("base", dtype, leg)
            assert np.array_equal(A, want[0]) and B is want[1] and rule == want[2]
    for dtype in (np.float32, np.float64):
        D, B, rule = leg_system("symmetric", dtype, "inconsistent")
        assert np.array_equal(D, D.T) and rule == 1 and leg_system("symmetric", dtype, "adjoint")[0] is D
        assert np.array_equal(np.sign(np.linalg.eigvalsh(D.astype(np.float64))), np.repeat([-1.0, 1.0], N400 // 2))


@pytest.mark.parametrize("pair", PAIRS, ids=pair_id)
def test_the_twin_on_the_pairs_of_the_handle_suite(pair):
    op, dtype, leg = pair
    A, B, rule = leg_system(op, dtype, leg)
    r = lsqr_rtol(dtype)
    runs = leg_runs(op, dtype, leg)
    crit = [criterion(A, t, B[:, c], r, rule) for c, t in enumerate(runs)]
    moved = []
    for seed in range(4):
        o = orders(seed, *A.shape)
        for c in (0, 4):
            t = lsqr_twin(A, B[:, c], r, 0.0, r, 0.0, 400, dtype, order=o)
            assert t.status == 0
            moved.append(t.iterations - runs[c].iterations)
    print(f"LSHSTAT twin {pair_id(pair)}: counts {[t.iterations for t in runs]}, rule {rule} criterion / threshold at most {max(crit):.3f}, "
          f"columns 0 and 4 under four permuted orders moved by {min(moved)} .. {max(moved)}")
    assert all(t.status == 0 for t in runs) and [t.iterations for t in runs] == COUNTS[op, name(dtype), leg]
    assert max(crit) <= 1.0, crit
    assert max(abs(d) for d in moved) <= 1, moved


def test_the_bordered_and_new_value_operands():
    for dtype in (np.float64, np.complex64):
        p, A, B, Bu = bordered_problem(dtype)
        assert A.shape == p["size"] == (M600 + BORDER, N400 + BORDER) and B.shape == (M600 + BORDER, NB) and Bu.shape == (N400 + BORDER, NB)
        assert not A[M600:].any() and not A[:, N400:].any() and np.array_equal(A[:M600, :N400], lsqr_problem("blocksparse", dtype)[1])
        assert not Bu[N400:].any() and np.all(Bu[:N400] != 0) and np.all(B[M600:] != 0)
        # the twin's iterates are exactly zero where no block reaches
        assert all(not t.x[N400:].any() for t in leg_runs("bordered", dtype, "inconsistent"))
        assert all(not t.x[M600:].any() for t in leg_runs("bordered", dtype, "adjoint"))
    pos, rows, ids = largest_row_set()
    assert len(rows) == 252 and len(ids) == 10 and 1 not in ids and lsqr_problem("blocksparse", np.float64)[0]["blocks"][0].shape == (1, 1)
    for kind in ("vbcrs", "blocksparse"):
        for dtype in DTYPES:
            p, A = lsqr_problem(kind, dtype)[:2]
            ids, new, p2, op = new_values(kind, dtype)
            A2 = operand(op, dtype).A
            assert 0 < len(ids) < len(p["blocks"]) and len(new) == len(ids)
            changed = [k + 1 for k, (a, b) in enumerate(zip(p["blocks"], p2["blocks"])) if not np.array_equal(a, b)]
            assert changed == list(ids) and all(np.array_equal(p2["blocks"][k - 1], b) for k, b in zip(ids, new))
            if kind == "vbcrs":
                D2 = np.block([[p2["blocks"][4 * a + b] for b in range(4)] for a in range(6)])
            else:
                D2 = np.zeros_like(A)
                for blk, ri, ci in zip(p2["blocks"], p2["rowindices"], p2["colindices"]):
                    D2[np.ix_(ri - 1, ci - 1)] = blk
            assert np.array_equal(D2, A2) and not np.array_equal(A2, A)


@pytest.mark.parametrize("pair", UPDATES, ids=pair_id)
def test_stale_values_are_visible(pair):
    op, dtype, leg = pair
    r = lsqr_rtol(dtype)
    A1, B, rule = leg_system("base", dtype, leg)
    A2, B2, _ = leg_system(op, dtype, leg)
    assert B2 is B
    old, new = leg_runs("base", dtype, leg), leg_runs(op, dtype, leg)
    old_on_new = min(criterion(A2, t, B[:, c], r, rule) for c, t in enumerate(old))
    new_on_old = min(criterion(A1, t, B[:, c], r, rule) for c, t in enumerate(new))
    print(f"LSHSTAT stale {pair_id(pair)}: rule {rule} criterion / threshold of the old solution on the new operator at least {old_on_new:.2e}, "
          f"of the new one on the old operator {new_on_old:.2e}")
    assert old_on_new > 100 and new_on_old > 100


HALVES = [(k, leg, which) for k in ("vbcrs2", "blocksparse2") for leg in LEGS for which in ("forward-new", "adjoint-new")]


@pytest.mark.parametrize("op, leg, which", HALVES, ids=[f"{k}-{leg}-{w}" for k, leg, w in HALVES])
def test_a_half_refill_is_visible(op, leg, which):
    dtype, r = np.float64, 1e-8
    A1, B, rule = leg_system("base", dtype, leg)
    A2 = leg_system(op, dtype, leg)[0]
    half = Half(A2, A1) if which == "forward-new" else Half(A1, A2)
    runs = [lsqr_twin(half, B[:, c], r, 0.0, r, 0.0, 400, dtype) for c in range(NB)]
    crit = [criterion(A2, t, B[:, c], r, rule) for c, t in enumerate(runs)]
    print(f"LSHSTAT half refill {op} {leg} {which}: statuses {[t.status for t in runs]}, iterations {[t.iterations for t in runs]}, rule {rule} "
          f"criterion / threshold on the new operator {min(crit):.2e} .. {max(crit):.2e}")
    assert [t.status for t in runs] == [1] * NB and [t.iterations for t in runs] == [400] * NB
    assert min(crit) > 100


# ---- analysis-only builds of every mode the GPU suite uses ----------------------------------------------------------------
MODES = {"default": {}, "gather": dict(accumulate="gather"), "colored": dict(accumulate="colored"), "transpose_image": dict(transpose_image=True),
         "own-all": dict(own=(1, M600)), "storage": None}
BUILDS = [(k, dt, m) for k in ("vbcrs", "blocksparse") for dt in DTYPES for m in MODES if m != "storage" or dt in WIDE]
BUILDS += [("symmetric", dt, m) for dt in (np.float32, np.float64) for m in ("default", "gather", "colored")]
BUILDS += [("bordered", dt, m) for dt in (np.float64, np.complex64) for m in ("default", "gather", "colored", "transpose_image")]


def read_back(bsm, A, D):
    """A[I, J] and transpose(A)[I, J] over the whole index range against the dense operator, to the bit"""
    m, n = D.shape
    assert A.size == (m, n) and A.device is None
    assert np.array_equal(A[np.arange(m), np.arange(n)], D), "A[I, J] is not the dense operator"
    assert np.array_equal(bsm.transpose(A)[np.arange(n), np.arange(m)], D.T), "transpose(A)[I, J] is not its transpose"


@pytest.mark.parametrize("kind, dtype, mode", BUILDS, ids=[f"{k}-{name(dt)}-{m}" for k, dt, m in BUILDS])
def test_every_mode_builds_analysis_only(bsm, kind, dtype, mode):
    kw = dict(storage=single_of(dtype)) if mode == "storage" else MODES[mode]
    if kind == "symmetric":
        p, D, _ = symmetric_problem(dtype)
    elif kind == "bordered":
        p, D = bordered_problem(dtype)[:2]
    else:
        p = lsqr_problem(kind, dtype)[0]
        D = operand("rounded" if mode == "storage" else "base", dtype).A
    A = bsm.synthetic.build(p, device=NODEV, **kw)
    read_back(bsm, A, D)
    assert A.dtype == np.dtype(dtype) and A.storage_dtype == (single_of(dtype) if mode == "storage" else np.dtype(dtype))
    if mode in ("gather", "colored"):
        assert A.stats()["exclusive"] == 0


@pytest.mark.parametrize("kind", ["vbcrs", "blocksparse"])
@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("timage", [False, True], ids=["one-image", "two-images"])
def test_the_partial_update_reaches_both_images(bsm, kind, dtype, timage):
    """update_blocks(A, the new blocks, ids=...) as the GPU legs call it, on the host image(s): op(A)[I, J] read back is the new
    operator for op = N and T (the second image of a transpose_image handle answers T)"""
    from _values import copied
    ids, new, _, op = new_values(kind, dtype)
    A = bsm.synthetic.build(copied(lsqr_problem(kind, dtype)[0]), device=NODEV, **(dict(transpose_image=True) if timage else {}))
    read_back(bsm, A, operand("base", dtype).A)
    bsm.update_blocks(A, new, ids=ids)
    read_back(bsm, A, operand(op, dtype).A)
    assert is_complex(dtype) == np.iscomplexobj(new[0])
