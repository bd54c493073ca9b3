"""CPU suite of bsm_invert_blocks (batched in-place inverse of dense blocks) and of block_jacobi on analysis-only
handles: the BSM_MEM_HOST path runs the elimination the device kernel runs, serially in plain C++, so the algorithm, the
info convention, the refusals and the Python composition (submatrices -> invert_blocks -> BlockSparseMatrix) are checked
here without a GPU.  Blocks, the accuracy figure rho and the bound RHO_MAX = 4 are derived in tests/_jacobi.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from _common import NODEV
from _jacobi import CODE, DTYPES, KINDS, NOP, RHO_MAX, SIZES, good_block, jacobi_problem, outside, padded, raw_invert, rho, set_blocks
from _submat import Truth
from _values import src_list

IDS = [np.dtype(d).name for d in DTYPES]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_host_inverse_of_padded_blocks(bsm, dtype):
    """every size in one call, ld = n + 3 with NaN padding that must come back bit-identical, an n = 0 block with a NULL
    pointer in the middle"""
    rng = np.random.default_rng(1800 + CODE[np.dtype(dtype)])
    worst = 0.0
    for draw in range(3):
        B = [good_block(rng, n, dtype) for n in SIZES]
        bufs = [padded(b, 3) for b in B]
        before = [outside(buf, b.shape[0], b.shape[0] + 3) for (buf, _), b in zip(bufs, B)]
        ptrs = [buf for buf, _ in bufs]
        ptrs.insert(4, None)
        ns = [b.shape[0] for b in B]
        ns.insert(4, 0)
        rc, info = raw_invert(CODE[np.dtype(dtype)], ptrs, ns, [n + 3 for n in ns])
        assert rc == 0 and not info.any(), (rc, info)
        for (buf, view), b, was in zip(bufs, B, before):
            assert outside(buf, b.shape[0], b.shape[0] + 3) == was, "a byte outside a window was written"
            r = rho(view, b)
            print(f"  host {np.dtype(dtype).name} n {b.shape[0]} draw {draw}: rho {r:.3f}")
            worst = max(worst, r)
            assert r <= RHO_MAX, (b.shape[0], r)
    print(f"INVSTAT host {np.dtype(dtype).name} worst rho {worst:.3f}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_the_python_entry_inverts_in_place_and_returns_info(bsm, dtype):
    rng = np.random.default_rng(1810)
    B = [good_block(rng, n, dtype) for n in (0, 1, 9, 64)]
    X = [b.copy(order="F") for b in B]
    info = bsm.invert_blocks(X)
    assert info.dtype == np.int64 and info.tolist() == [0, 0, 0, 0]
    assert all(rho(x, b) <= RHO_MAX for x, b in zip(X, B))
    assert bsm.invert_blocks([]).shape == (0,)
    with pytest.raises(ValueError):
        bsm.invert_blocks([np.zeros((2, 3), dtype=dtype, order="F")])
    with pytest.raises(TypeError):
        bsm.invert_blocks([np.zeros((3, 3), dtype=dtype)[::-1].T[:, :2][:2]])  # not Fortran order
    with pytest.raises(TypeError):
        bsm.invert_blocks([np.eye(2, dtype=dtype, order="F"), np.eye(2, dtype=np.int32, order="F")])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_info_names_the_step_and_spares_the_neighbours(bsm, dtype):
    rng = np.random.default_rng(1820)
    n = 9
    good = [good_block(rng, k, dtype) for k in (7, n, 65)]
    zero = np.zeros((n, n), dtype=dtype, order="F")
    dup = good_block(rng, n, dtype)
    dup[5] = dup[2]  # one row duplicated: rank n - 1
    nan = good_block(rng, n, dtype)
    nan[3, 4] = np.nan
    batch = [good[0], zero, good[1], dup, nan, good[2]]
    X = [b.copy(order="F") for b in batch]
    rc, info = raw_invert(CODE[np.dtype(dtype)], X, [b.shape[0] for b in X], [b.shape[0] for b in X])
    assert rc == 0
    assert info[1] == 1, info            # an all-zero block: the first pivot
    assert 1 <= info[3] <= n, info       # a duplicated row: some step runs out of pivots
    assert info[4] != 0, info            # a NaN entry
    for k in (0, 2, 5):
        assert info[k] == 0 and rho(X[k], batch[k]) <= RHO_MAX, (k, info)
    # info == NULL is allowed: the good blocks are inverted all the same
    Y = [b.copy(order="F") for b in batch]
    rc, _ = raw_invert(CODE[np.dtype(dtype)], Y, [b.shape[0] for b in Y], [b.shape[0] for b in Y], info=False)
    assert rc == 0 and all(Y[k].tobytes() == X[k].tobytes() for k in (0, 2, 5))


def test_refusals_leave_the_buffers_untouched(bsm):
    from bsm_amd import _lib as L
    rng = np.random.default_rng(1830)
    a, b = good_block(rng, 3, np.float64), good_block(rng, 5, np.float64)

    def refused(blocks, n, ld, want=-1, code=1, **kw):
        bufs = [x.copy(order="F") if isinstance(x, np.ndarray) else x for x in blocks]
        rc, info = raw_invert(code, bufs, n, ld, **kw)
        assert rc == want, (rc, want)
        assert L.lib().bsm_last_error()
        assert np.all(info == -77), "info was written by a refused call"
        for x, y in zip(bufs, blocks):
            if isinstance(x, np.ndarray):
                assert x.tobytes() == y.tobytes()

    x, y = a.copy(order="F"), b.copy(order="F")
    assert raw_invert(1, [x, y], [3, 5], [3, 5])[0] == 0  # the calls below differ from this one in one thing
    refused([a, b], [3, 5], [3, 5], null=("blocks",))
    refused([a, b], [3, 5], [3, 5], null=("n",))
    refused([a, b], [3, 5], [3, 5], null=("ld",))
    refused([a, b], [3, 5], [3, 5], nblocks=-1)
    refused([a, b], [3, -5], [3, 5])                      # a negative size
    refused([a, b], [3, 5], [3, 4])                       # ld < n
    refused([a, None], [3, 0], [3, 0])                    # ld < 1 on an empty block
    refused([a, None], [3, 5], [3, 5])                    # a NULL block with n > 0
    for code in (4, 5, -1, 6):                            # the mixed storage codes, and no dtype at all
        refused([a, b], [3, 5], [3, 5], code=code)
    refused([a, b], [3, 5], [3, 5], memspace=2)
    refused([a, b], [3, 5], [3, 5], memspace=-1)
    big = np.zeros((1025, 1025), order="F")
    refused([a, big], [3, 1025], [3, 1025], want=-2)      # BSM_ERR_UNSUPPORTED, and block 1 is not inverted first
    # legal edges: no blocks at all (with NULL arrays), an empty block without a pointer
    assert raw_invert(1, [], [], [], null=("blocks", "n", "ld"))[0] == 0
    rc, info = raw_invert(1, [None, a.copy(order="F")], [0, 3], [1, 3])
    assert rc == 0 and info.tolist() == [0, 0]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_block_jacobi_of_an_analysis_only_handle(bsm, kind, dtype):
    """scattered sets of sizes 1 .. 129 and a rest; every A[I_s, I_s] a good block once its overlapping extra block is
    added; coupling blocks between the sets, which must be ignored"""
    rng = np.random.default_rng(1840 + 10 * KINDS.index(kind) + CODE[np.dtype(dtype)])
    p, sets = jacobi_problem(rng, kind, dtype)
    A, tr = bsm.synthetic.build(p, device=NODEV), Truth(p)
    assert np.count_nonzero(tr.Cnt > 1) > 0 and np.count_nonzero(tr.D) > sum(len(s) ** 2 for s in sets)  # overlap, couplings
    M = bsm.block_jacobi(A, sets)
    assert isinstance(M, bsm.BlockJacobi) and isinstance(M, bsm.BlockSparseMatrix)
    assert M.device is None and M.source is A and bsm.size(M) == (NOP, NOP) and bsm.eltype(M) == np.dtype(dtype)
    assert len(M.sets) == len(sets) and all(np.array_equal(a, b) and a.dtype == np.int64 for a, b in zip(M.sets, sets))
    worst = 0.0
    for s, want in enumerate(set_blocks(tr.D, sets)):
        got = bsm.block(M, s + 1)
        assert got.shape == want.shape and got.dtype == np.dtype(dtype)
        r = rho(got, want)
        worst = max(worst, r)
        assert r <= RHO_MAX, (kind, s, r)
        assert np.array_equal(bsm.rowindices(M, s + 1), sets[s]) and np.array_equal(bsm.colindices(M, s + 1), sets[s])
    print(f"INVSTAT block_jacobi host {kind} {np.dtype(dtype).name} worst rho {worst:.3f}")
    # M[I, J] reads the inverse blocks back out of M's own image; entries between two sets are zero
    i, j = sets[5] - 1, sets[6] - 1
    assert M[i, i].tobytes() == np.ascontiguousarray(bsm.block(M, 6)).tobytes()
    assert not M[i, j].any()
    # the transposed operator gives the transposed inverse blocks
    Mt = bsm.block_jacobi(bsm.transpose(A), sets)
    for s, want in enumerate(set_blocks(tr.D.T, sets)):
        assert rho(bsm.block(Mt, s + 1), want) <= RHO_MAX, (kind, s, "transpose")


@pytest.mark.parametrize("kind", KINDS)
def test_refresh_follows_new_values_of_the_source(bsm, kind):
    rng = np.random.default_rng(1860 + KINDS.index(kind))
    p, sets = jacobi_problem(rng, kind, np.float64)
    q, sets2 = jacobi_problem(np.random.default_rng(1860 + KINDS.index(kind)), kind, np.float64, scale=-0.5)
    assert all(np.array_equal(a, b) for a, b in zip(sets, sets2))
    A = bsm.synthetic.build(p, device=NODEV)
    M = bsm.block_jacobi(A, sets)
    kept = [id(b) for b in M.blocks]
    bsm.update_blocks(A, src_list(q))
    M.refresh()
    assert [id(b) for b in M.blocks] == kept
    for s, want in enumerate(set_blocks(Truth(q).D, sets)):
        assert rho(bsm.block(M, s + 1), want) <= RHO_MAX, (kind, s)
        assert bsm.submatrix(M, sets[s], sets[s]).tobytes() == np.ascontiguousarray(bsm.block(M, s + 1)).tobytes()  # the image too


def test_sets_defaults_and_errors(bsm):
    rng = np.random.default_rng(1870)
    p, sets = jacobi_problem(rng, "symmetric", np.complex128)
    S = bsm.synthetic.build(p, device=NODEV)
    for op in (S, bsm.transpose(S), bsm.adjoint(S)):  # sets=None: the diagonalindices, of the wrapped operator too
        M = bsm.block_jacobi(op)
        assert all(np.array_equal(a, b) for a, b in zip(M.sets, S.diagonalindices)) and M.source is op
    Ma = bsm.block_jacobi(bsm.adjoint(S))
    for s, want in enumerate(set_blocks(Truth(p).D.conj().T, sets)):
        assert rho(bsm.block(Ma, s + 1), want) <= RHO_MAX
    pb, setsb = jacobi_problem(rng, "blocksparse", np.float32)
    B = bsm.synthetic.build(pb, device=NODEV)
    with pytest.raises(ValueError):
        bsm.block_jacobi(B)  # no sets of its own
    with pytest.raises(RuntimeError):
        bsm.block_jacobi(B, [setsb[3], setsb[3][:2]])  # overlapping sets: what bsm_submatrices refuses
    # rows in no set are zero rows of M
    M = bsm.block_jacobi(B, setsb[:3])
    rest = np.concatenate(setsb[3:]) - 1
    assert not M[rest, :].any() and M[setsb[2] - 1, setsb[2] - 1].any()
    # a rectangular operator
    R = bsm.BlockSparseMatrix([np.ones((2, 3))], [[1, 2]], [[1, 2, 3]], (4, 5), device=NODEV)
    with pytest.raises(ValueError):
        bsm.block_jacobi(R, [[1, 2]])
    # a singular set: named with its step, and no handle
    pz, setsz = jacobi_problem(rng, "blocksparse", np.float64)
    pz["blocks"][2] = np.zeros_like(pz["blocks"][2])  # the 7-set (nothing overlaps it)
    Z = bsm.synthetic.build(pz, device=NODEV)
    with pytest.raises(np.linalg.LinAlgError, match=r"set 3 .*step 1"):
        bsm.block_jacobi(Z, setsz)
    # refresh after the source turned singular raises and leaves M as it was
    G = bsm.synthetic.build(jacobi_problem(np.random.default_rng(5), "blocksparse", np.float64)[0], device=NODEV)
    gs = jacobi_problem(np.random.default_rng(5), "blocksparse", np.float64)[1]
    M = bsm.block_jacobi(G, gs)
    was = [b.copy() for b in M.blocks]
    new = [b.copy(order="F") for b in src_list(jacobi_problem(np.random.default_rng(5), "blocksparse", np.float64)[0])]
    new[2][...] = 0
    bsm.update_blocks(G, new)
    with pytest.raises(np.linalg.LinAlgError):
        M.refresh()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(was, M.blocks))
    # a storage= M refuses the refill as update_blocks does
    Mm = bsm.block_jacobi(bsm.synthetic.build(jacobi_problem(np.random.default_rng(5), "blocksparse", np.float64)[0], device=NODEV),
                          gs, storage=np.float32)
    assert Mm.storage_dtype == np.dtype(np.float32)
    with pytest.raises(NotImplementedError):
        Mm.refresh()


def test_the_prototype_is_declared_and_bound():
    from bsm_amd import _lib as L
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "bsm_rocm.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    assert ("int bsm_invert_blocks(int dtype, int64_t nblocks, void *const *blocks, const int64_t *n, const int64_t *ld, "
            "int64_t *info, int memspace, void *stream);") in flat
    assert f"#define BSM_INVERT_LDS_BYTES {L.BSM_INVERT_LDS_BYTES} " in flat and f"#define BSM_INVERT_MAX_N {L.BSM_INVERT_MAX_N}" in flat
    lib = L.lib()
    PP, IP = C.POINTER(C.c_void_p), C.POINTER(C.c_int64)
    assert "bsm_invert_blocks" in L.EXPORTS
    assert lib.bsm_invert_blocks.restype is C.c_int and list(lib.bsm_invert_blocks.argtypes) == [
        C.c_int, C.c_int64, PP, IP, IP, IP, C.c_int, C.c_void_p]
