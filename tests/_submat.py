"""What the two submatrix suites (test_submatrices_cpu.py, test_gpu_submatrices.py) share: the dense ground truth of a
problem built from `_fuzz.coo_triples` (no library code), the elementwise acceptance rule, the index-set legs and a raw
ctypes driver of bsm_submatrices / bsm_diag.  Test code only.

Acceptance (derived, not tuned).  D, Abs and Cnt are the sums of the values, of their moduli and of ones per position.
  * Cnt <= 1: the window holds one stored entry added to zero, or the zero itself -> BIT-identical to 0 + D.
    (`0 + x` is what "zeroed, then summed" does to a value: it turns the -0.0 that conj() leaves in the imaginary part of
    an untouched entry of D.conj().T, and a stored -0.0, into +0.0.)
  * elsewhere |got - D| <= Cnt * eps(T) * Abs: either summation order is within (Cnt - 1) * eps / 2 * Abs of the exact
    sum, the bound absorbs the second-order terms."""
import ctypes as C

import numpy as np

from _common import N, T
from _fuzz import coo_triples, rounded

SIZES = (1, 2, 7, 8, 9, 63, 64, 65, 129)  # set sizes of the partition leg; the rest forms the last set


class Truth:
    """D / Abs / Cnt of a problem; storage: the stored type of a mixed handle (the blocks are rounded once first)"""

    def __init__(self, problem, storage=None):
        p = rounded(problem, storage) if storage is not None else problem
        r, c, v = coo_triples(p)
        self.dtype = v.dtype
        self.D = np.zeros(p["size"], dtype=v.dtype)
        self.Abs = np.zeros(p["size"], dtype=np.float64)
        self.Cnt = np.zeros(p["size"], dtype=np.int64)
        np.add.at(self.D, (r - 1, c - 1), v)
        np.add.at(self.Abs, (r - 1, c - 1), np.abs(v).astype(np.float64))
        np.add.at(self.Cnt, (r - 1, c - 1), 1)

    def of(self, op):
        """(D, Abs, Cnt) of op(A)"""
        if op == N:
            return self.D, self.Abs, self.Cnt
        return (self.D.T if op == T else self.D.conj().T), self.Abs.T, self.Cnt.T


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize // (2 if a.dtype.kind == "c" else 1)])


def accept(got, want, ab, cnt, what):
    """the acceptance rule of the module docstring on arrays of one shape"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.size == 0:
        return
    got, want, ab, cnt = (np.atleast_1d(v) for v in (got, np.zeros((), dtype=want.dtype) + want, ab, cnt))
    one = cnt <= 1
    same = bits(got).reshape(got.shape + (-1,)) == bits(want).reshape(want.shape + (-1,))
    assert np.all(same.all(axis=-1)[one]), (what, "an entry with at most one stored value is not bit-identical",
                                            int(np.sum(~same.all(axis=-1)[one])))
    eps = np.finfo(got.dtype).eps
    err, bound = np.abs(got - want), cnt * eps * ab
    assert np.all(err[~one] <= bound[~one]), (what, float(np.max(err[~one] - bound[~one])))


def check_sets(truth, op, outs, rowsets, colsets, what):
    D, Ab, Cn = truth.of(op)
    assert len(outs) == len(rowsets)
    for s, (o, I, J) in enumerate(zip(outs, rowsets, colsets)):
        sel = np.ix_(np.asarray(I, dtype=np.int64) - 1, np.asarray(J, dtype=np.int64) - 1)
        accept(o, D[sel], Ab[sel], Cn[sel], (what, "set", s))


def cut(rng, n):
    """1..n shuffled and cut into sets of the sizes SIZES (as far as n reaches) and the rest"""
    perm = rng.permutation(n).astype(np.int64) + 1
    sets, pos = [], 0
    for k in SIZES:
        if pos + k > n:
            break
        sets.append(perm[pos:pos + k])
        pos += k
    sets.append(perm[pos:])
    return sets


def partition_sets(rng, shape):
    """rows and columns of an operator of this shape, each shuffled and cut (`cut`), paired by position -- the longer
    list's surplus joins its last set --, plus a pair with ni = 0 and one with nj = 0 (`with_empties`)"""
    rs, cs = cut(rng, shape[0]), cut(rng, shape[1])
    k = min(len(rs), len(cs))
    rs, cs = rs[:k - 1] + [np.concatenate(rs[k - 1:])], cs[:k - 1] + [np.concatenate(cs[k - 1:])]
    return with_empties(rs, cs)


def with_empties(rs, cs):
    """appends a pair with ni = 0 (its column taken off the largest column set) and one with nj = 0 (its row off the largest
    row set)"""
    rs, cs = [np.array(r) for r in rs], [np.array(c) for c in cs]
    none = np.zeros(0, np.int64)
    kr, kc = int(np.argmax([len(r) for r in rs])), int(np.argmax([len(c) for c in cs]))
    row, col = rs[kr][:1], cs[kc][:1]
    rs[kr], cs[kc] = rs[kr][1:], cs[kc][1:]
    return rs + [none, row], cs + [col, none]


def disjoint_rounds(rowlists, collists):
    """the (row list, column list) pairs spread first-fit over calls in which the row lists are pairwise disjoint and so
    are the column lists (the contract of bsm_submatrices) -> [[pair ids]]; empty lists are left out"""
    rounds = []
    for b, (r, c) in enumerate(zip(rowlists, collists)):
        if len(r) == 0 or len(c) == 0:
            continue
        for rd in rounds:
            if not (rd["r"] & set(r.tolist())) and not (rd["c"] & set(c.tolist())):
                break
        else:
            rd = dict(r=set(), c=set(), ids=[])
            rounds.append(rd)
        rd["r"] |= set(r.tolist())
        rd["c"] |= set(c.tolist())
        rd["ids"].append(b)
    return [rd["ids"] for rd in rounds]


def raw_submatrices(A, op, I, J, outs, ldo, memspace=0, stream=None, nsets=None):
    """bsm_submatrices as C sees it -> return code.  I / J: int64 arrays; outs: numpy buffers, device addresses or None"""
    from bsm_amd import _lib as L
    n = len(I) if nsets is None else nsets
    I = [np.ascontiguousarray(v, dtype=np.int64) for v in I]
    J = [np.ascontiguousarray(v, dtype=np.int64) for v in J]
    ip, jp, op_ = (C.c_void_p * max(len(I), 1))(), (C.c_void_p * max(len(J), 1))(), (C.c_void_p * max(len(outs), 1))()
    for k, v in enumerate(I):
        ip[k] = v.ctypes.data
    for k, v in enumerate(J):
        jp[k] = v.ctypes.data
    for k, o in enumerate(outs):
        op_[k] = o.ctypes.data if isinstance(o, np.ndarray) else o
    ni = np.array([len(v) for v in I], dtype=np.int64)
    nj = np.array([len(v) for v in J], dtype=np.int64)
    ld = np.ascontiguousarray(ldo, dtype=np.int64)
    P = C.POINTER(C.c_int64)
    return L.lib().bsm_submatrices(A._h.ptr, op, n, ip, ni.ctypes.data_as(P), jp, nj.ctypes.data_as(P), op_, ld.ctypes.data_as(P),
                                   memspace, stream)
