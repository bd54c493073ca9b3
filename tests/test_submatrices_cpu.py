"""CPU suite of bsm_submatrices / bsm_diag (A[I, J] and diag(A) read out of the packed image): analysis-only handles
answer from their host image by a plain loop over the wave records the kernel walks, so the decode -- rows from rbase or
the rows pool, columns from the inline segments or the cols pool, the transposed role of symmetric off-diagonal columns
-- is checked here without a GPU, on the layout-edge operators of tests/_fuzz.py, against dense arrays built from
_fuzz.coo_triples (the whole operator and diag(A) also from _common.coo_of).  The acceptance rule is derived in
tests/_submat.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from _common import NODEV, WORK_PANEL, Cc, N, T, coo_of, get_image, wrap
from _fuzz import GEN, rounded, seed_of
from _submat import Truth, accept, check_sets, disjoint_rounds, partition_sets, raw_submatrices
from _values import NOPS, assert_coverage, value_operators

KINDS = ["blocksparse", "vbcrs", "symmetric"]
DTYPES = [np.float32, np.float64, np.complex64, np.complex128]
# (element type, storage=): the four element types and the two mixed-storage pairs
TYPES = [(d, None) for d in DTYPES] + [(np.float64, np.float32), (np.complex128, np.complex64)]
TYPE_IDS = [np.dtype(d).name + ("" if s is None else "_as_" + np.dtype(s).name) for d, s in TYPES]
OPS = (N, T, Cc)
NOPER = NOPS  # the operators of the value fuzz, whose coverage of the layout edges is asserted below


def build(bsm, p, storage=None, **kw):
    return bsm.synthetic.build(p, device=NODEV, **({} if storage is None else {"storage": storage}), **kw)


def one_based(n):
    return np.arange(1, n + 1, dtype=np.int64)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype,storage", TYPES, ids=TYPE_IDS)
def test_full_shuffled_and_partitioned_selections(bsm, kind, dtype, storage):
    ops = value_operators(kind, dtype)
    assert_coverage(kind, dtype, ops[:NOPER])  # the operators used reach every layout edge of the kind
    rng = np.random.default_rng(seed_of(kind, dtype) + 9100)
    nsets = entries = 0
    for case, p in enumerate(ops[:NOPER]):
        A, tr = build(bsm, p, storage), Truth(p, storage)
        for op in OPS:
            Aop = wrap(bsm, A, op)
            m, n = bsm.size(Aop)
            tag = (kind, np.dtype(dtype).name, case, op)
            # everything, as one set
            I, J = [one_based(m)], [one_based(n)]
            check_sets(tr, op, bsm.submatrices(Aop, I, J), I, J, tag + ("full",))
            # a shuffled half of the rows against a shuffled half of the columns
            I, J = [rng.permutation(m)[:m // 2] + 1], [rng.permutation(n)[:n // 2] + 1]
            check_sets(tr, op, [bsm.submatrix(Aop, I[0], J[0])], I, J, tag + ("halves",))
            # a partition into sets of the edge sizes, with an ni = 0 and an nj = 0 pair
            I, J = partition_sets(rng, (m, n))
            assert any(len(i) == 0 and len(j) > 0 for i, j in zip(I, J)) and any(len(j) == 0 and len(i) > 0 for i, j in zip(I, J))
            outs = bsm.submatrices(Aop, I, J)
            assert [o.shape for o in outs] == [(len(i), len(j)) for i, j in zip(I, J)]
            check_sets(tr, op, outs, I, J, tag + ("partition",))
            nsets += len(I) + 2
            entries += sum(o.size for o in outs)
    print(f"SUBSTAT selections {kind} {TYPE_IDS[TYPES.index((dtype, storage))]} operators {NOPER} sets {nsets} entries {entries}")


def column_forms(A):
    """how the wave records of an analysis-only handle name their columns: "pool" (the cols pool; "pool_flag": with a
    column whose sign bit takes it out of the piece's kind) and "inline1" .. "inline3" (that many inline segments;
    "inline_mixed": of different kinds)"""
    _, _, cols, waves = get_image(A)
    out = set()
    for W in waves:
        if W["work"] != WORK_PANEL or W["npieces"] == 0:
            continue
        P, n = W["first"], W["first"]["ncols"]
        if P["xbase"] < 0:
            out.add("pool")
            if np.any(cols[P["col_off"]:P["col_off"] + n] < 0):
                out.add("pool_flag")
        else:
            nseg = 1 + int(W["seg1_w"] < n) + int(W["seg2_w"] < n)
            out.add(f"inline{nseg}")
            if len({(P["kind"] >> (2 * s)) & 3 for s in range(nseg)}) > 1:
                out.add("inline_mixed")
    return out


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype,storage", TYPES, ids=TYPE_IDS)
def test_whole_operator_and_diag_against_the_dense_sum_of_coo_of(bsm, kind, dtype, storage):
    """A[all rows, all columns] and diag(A) of every layout-edge operator against the dense sum of _common.coo_of, the
    reference's own oracle path: the host walker over the columns of a wave record on every branch it has"""
    forms = set()
    for case, p in enumerate(value_operators(kind, dtype)):
        A = build(bsm, p, storage)
        forms |= column_forms(A)
        r, c, v = coo_of(rounded(p, storage) if storage is not None else p)
        D, Ab, Cn = np.zeros(p["size"], dtype=dtype), np.zeros(p["size"]), np.zeros(p["size"], dtype=np.int64)
        np.add.at(D, (r - 1, c - 1), v)
        np.add.at(Ab, (r - 1, c - 1), np.abs(v))
        np.add.at(Cn, (r - 1, c - 1), 1)
        m, n = p["size"]
        accept(bsm.submatrix(A, one_based(m), one_based(n)), D, Ab, Cn, (kind, case, "whole operator"))
        k = np.arange(min(m, n))
        accept(bsm.diag(A), D[k, k], Ab[k, k], Cn[k, k], (kind, case, "diag"))
    want = {"pool", "inline1", "inline2", "inline3"} | ({"pool_flag", "inline_mixed"} if kind == "symmetric" else set())
    assert forms == want, (kind, sorted(forms))


@pytest.mark.parametrize("dtype,storage", TYPES, ids=TYPE_IDS)
def test_symmetric_own_sets_and_off_diagonal_pairs(bsm, dtype, storage):
    """the operator's own diagonalindices as row and column sets (the block-Jacobi blocks, perm-scattered sets included),
    and every off-diagonal block's (rowindices, colindices) -- and swapped, which only the transposed role fills.  The pairs
    of one call must be disjoint, so they are spread first-fit over as few calls as that takes."""
    ops = value_operators("symmetric", dtype)[:NOPER]
    assert any(np.any(np.diff(d) != 1) for p in ops for d in p["diagonalindices"] if len(d) > 1)  # a scattered own set
    pairs = 0
    for case, p in enumerate(ops):
        A, tr = build(bsm, p, storage), Truth(p, storage)
        for op in OPS:
            Aop = wrap(bsm, A, op)
            own = [bsm.diagonalindices(Aop, d) for d in bsm.eachdiagonalindex(Aop)]
            check_sets(tr, op, bsm.submatrices(Aop, own), own, own, ("symmetric", case, op, "own sets"))
            rl = [bsm.rowindices(Aop, b) for b in bsm.eachoffdiagonalindex(Aop)]
            cl = [bsm.colindices(Aop, b) for b in bsm.eachoffdiagonalindex(Aop)]
            for ids in disjoint_rounds(rl, cl):
                I, J = [rl[b] for b in ids], [cl[b] for b in ids]
                check_sets(tr, op, bsm.submatrices(Aop, I, J), I, J, ("symmetric", case, op, "off-diagonal pairs"))
                check_sets(tr, op, bsm.submatrices(Aop, J, I), J, I, ("symmetric", case, op, "swapped pairs"))
                pairs += 2 * len(ids)
    assert pairs > 0


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype,storage", TYPES, ids=TYPE_IDS)
def test_diag(bsm, kind, dtype, storage):
    shapes = set()
    for case, p in enumerate(value_operators(kind, dtype)[:NOPER]):
        A, tr = build(bsm, p, storage), Truth(p, storage)
        k = min(p["size"])
        shapes.add(p["size"][0] == p["size"][1])
        d = bsm.diag(A)
        assert d.shape == (k,) and d.dtype == np.dtype(dtype)
        ix = np.arange(k)
        accept(d, tr.D[ix, ix], tr.Abs[ix, ix], tr.Cnt[ix, ix], (kind, case, "diag"))
        assert bsm.diag(bsm.transpose(A)).tobytes() == d.tobytes()
        assert bsm.diag(bsm.adjoint(A)).tobytes() == d.conj().tobytes()  # a real handle: the same bits
    assert shapes == ({True} if kind == "symmetric" else {False}), shapes  # square and non-square operators are both run


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype,storage", [TYPES[1], TYPES[2], TYPES[4]], ids=[TYPE_IDS[1], TYPE_IDS[2], TYPE_IDS[4]])
def test_padding_is_kept_and_incoming_nan_is_not(bsm, kind, dtype, storage):
    """ldo > ni, every buffer NaN beforehand: the windows hold the result, every byte outside them is unchanged"""
    rng = np.random.default_rng(seed_of(kind, dtype) + 9200)
    p = value_operators(kind, dtype)[0]
    A, tr = build(bsm, p, storage), Truth(p, storage)
    for op in OPS:
        m, n = bsm.size(wrap(bsm, A, op))
        I, J = partition_sets(rng, (m, n))
        ldo = [len(i) + 3 for i in I]
        bufs = [np.full(ld * len(j) + 5, np.nan, dtype=dtype) for ld, j in zip(ldo, J)]
        before = [b.copy() for b in bufs]
        assert raw_submatrices(A, op, I, J, bufs, ldo) == 0
        outs = []
        for b, b0, ld, i, j in zip(bufs, before, ldo, I, J):
            body = b[:ld * len(j)].reshape(len(j), ld).T  # column-major, leading dimension ld
            outs.append(np.array(body[:len(i), :]))
            inside = np.zeros(len(b), dtype=bool)
            inside[:ld * len(j)].reshape(len(j), ld)[:, :len(i)] = True
            assert b[~inside].tobytes() == b0[~inside].tobytes(), (kind, op, "a byte outside a window was written")
            assert not np.any(np.isnan(outs[-1]))
        check_sets(tr, op, outs, I, J, (kind, op, "padded"))


KEYS = [(3, 5), (-1, 0), (slice(None), 7), (2, slice(None)), (slice(10, 60, 3), slice(None, None, -1)),
        (np.array([4, 9, 4, 0, 9]), slice(5, 40)), (slice(0, 30, 2), np.array([7, 7, 1, -2])), "mask", "two arrays"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype,storage", [TYPES[0], TYPES[3], TYPES[4]], ids=[TYPE_IDS[0], TYPE_IDS[3], TYPE_IDS[4]])
def test_getitem_is_numpy_indexing_of_the_dense_operator(bsm, kind, dtype, storage):
    rng = np.random.default_rng(seed_of(kind, dtype) + 9300)
    p = value_operators(kind, dtype)[1]
    A, tr = build(bsm, p, storage), Truth(p, storage)
    for op in OPS:
        Aop = wrap(bsm, A, op)
        D, Ab, Cn = tr.of(op)
        m, n = D.shape
        for key in KEYS:
            if isinstance(key, str) and key == "mask":
                mask = rng.random(m) < 0.3
                key, dense_key = (mask, slice(1, None, 5)), (mask, slice(1, None, 5))
            elif isinstance(key, str):  # two index arrays select the sub-matrix, as the reference's A[I, J] does
                a, b = rng.integers(0, m, 9), rng.integers(-n, n, 12)
                key, dense_key = (a, b), np.ix_(a, b)
            else:
                dense_key = key
            got = Aop[key]
            accept(got, D[dense_key], Ab[dense_key], Cn[dense_key], (kind, op, str(key)))
        for bad in [(m, 0), (0, -n - 1), (np.array([0, m]), 0), (np.zeros(m + 1, dtype=bool), 0), (1.5, 0), 3, (1, 2, 3)]:
            with pytest.raises(IndexError):
                Aop[bad]


@pytest.mark.parametrize("kind", KINDS)
def test_construction_options_do_not_change_what_is_read(bsm, kind):
    """accumulate= reorders the wave records, transpose_image= adds a second image: the entries read are those of the
    default handle -- exactly where at most two stored values meet (a + b = b + a in floating point), within the bound
    of _submat.accept where three or more do (their order follows the records)"""
    p = value_operators(kind, np.float64)[2]
    tr = Truth(p)
    m, n = p["size"]
    I, J = [one_based(m)], [one_based(n)]
    base = bsm.submatrices(build(bsm, p), I, J)[0]
    dbase = bsm.diag(build(bsm, p))
    variants = [dict(accumulate=a) for a in ("atomic", "gather", "direct")]
    if kind != "symmetric":
        variants.append(dict(transpose_image=1))
    few = tr.Cnt <= 2
    for kw in variants:
        B = build(bsm, p, **kw)
        got = bsm.submatrices(B, I, J)[0]
        assert got[few].tobytes() == base[few].tobytes(), (kind, kw)
        accept(got, tr.D, tr.Abs, tr.Cnt, (kind, kw))
        k = np.arange(min(m, n))
        assert bsm.diag(B)[few[k, k]].tobytes() == dbase[few[k, k]].tobytes(), (kind, kw)


def test_refusals_leave_the_buffers_untouched(bsm):
    from bsm_amd import _lib as L
    p = value_operators("blocksparse", np.float64)[0]
    A = build(bsm, p)
    m, n = p["size"]
    a, b = np.array([1, 2, 3], dtype=np.int64), np.array([4, 5], dtype=np.int64)
    c, d = np.array([7, 8], dtype=np.int64), np.array([1, 9, 3], dtype=np.int64)

    def refused(I, J, ldo=None, op=N, outs=None, memspace=0, nsets=None):
        bufs = [np.full(max(len(i), 1) * len(j) + 4, np.nan) for i, j in zip(I, J)] if outs is None else outs
        before = [x.copy() if isinstance(x, np.ndarray) else x for x in bufs]
        rc = raw_submatrices(A, op, I, J, bufs, [max(len(i), 1) for i in I] if ldo is None else ldo, memspace, None, nsets)
        assert rc == -1, rc  # BSM_ERR_INVALID
        assert L.lib().bsm_last_error()
        for x, y in zip(bufs, before):
            if isinstance(x, np.ndarray):
                assert x.tobytes() == y.tobytes()

    assert raw_submatrices(A, N, [a, c], [b, d], [np.empty(6), np.empty(6)], [3, 2]) == 0  # the calls below differ in one thing
    refused([np.array([0, 2, 3]), c], [b, d])                # an index of 0
    refused([a, c], [b, np.array([1, n + 1, 3])])            # an index of n + 1
    refused([np.array([1, m + 1])], [b])
    refused([a, np.array([7, 2])], [b, d])                   # a row in two sets
    refused([np.array([1, 2, 1]), c], [b, d])                # a row twice in one set
    refused([a, c], [b, np.array([1, 5, 3])])                # a column in two sets
    refused([a, c], [b, d], ldo=[2, 2])                      # ldo < ni
    refused([a, c], [b, d], op=3)                            # a bad op
    refused([a, c], [b, d], op=-1)
    refused([a, c], [b, d], outs=[np.full(6, np.nan), None])  # a null window that is not empty
    refused([a, c], [b, d], memspace=1)                      # BSM_MEM_DEVICE on an analysis-only handle
    refused([a, c], [b, d], memspace=2)
    refused([a, c], [b, d], nsets=-1)
    # op T: the bounds are those of the transposed operator
    assert raw_submatrices(A, T, [np.array([n])], [np.array([m])], [np.empty(1)], [1]) == 0
    if m != n:
        refused([np.array([max(m, n)])], [np.array([max(m, n)])], op=T if m > n else N)
    # an empty window may have no buffer; nsets = 0 is a legal call
    assert raw_submatrices(A, N, [a, np.zeros(0, np.int64)], [b, d], [np.empty(6), None], [3, 1]) == 0
    assert raw_submatrices(A, N, [], [], [], []) == 0
    # bsm_diag
    assert L.lib().bsm_diag(None, None, 0, None) == -1
    assert L.lib().bsm_diag(A._h.ptr, None, 0, None) == -1
    buf = np.full(min(m, n), np.nan)
    assert L.lib().bsm_diag(A._h.ptr, buf.ctypes.data, 1, None) == -1 and np.all(np.isnan(buf))
    assert L.lib().bsm_diag(A._h.ptr, buf.ctypes.data, 5, None) == -1 and np.all(np.isnan(buf))


def test_the_two_prototypes_are_declared_and_bound():
    from bsm_amd import _lib as L
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "bsm_rocm.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    assert ("int bsm_submatrices(bsm_matrix_t A, int op, int64_t nsets, const int64_t *const *I, const int64_t *ni, "
            "const int64_t *const *J, const int64_t *nj, void *const *out, const int64_t *ldo, int memspace, void *stream);") in flat
    assert "int bsm_diag(bsm_matrix_t A, void *d, int memspace, void *stream);" in flat
    lib = L.lib()
    PP, IP = C.POINTER(C.c_void_p), C.POINTER(C.c_int64)
    assert "bsm_submatrices" in L.EXPORTS and "bsm_diag" in L.EXPORTS
    assert lib.bsm_submatrices.restype is C.c_int and list(lib.bsm_submatrices.argtypes) == [
        C.c_void_p, C.c_int, C.c_int64, PP, IP, PP, IP, PP, IP, C.c_int, C.c_void_p]
    assert lib.bsm_diag.restype is C.c_int and list(lib.bsm_diag.argtypes) == [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    assert GEN.keys() == set(KINDS)
