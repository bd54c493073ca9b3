"""bsm_update_blocks on analysis-only handles (BSM_DEVICE_NONE): the host image a refill writes through the
replayable plan must be BYTE-identical to the image of a handle freshly created from the new values -- for every
constructor, both orderings (bsm_options.transpose_image), all four element types -- and a failing call must leave
the handle untouched."""
import ctypes as C

import numpy as np
import pytest

from _common import NODEV, get_image
from _values import update_rc

DTYPES = (np.float32, np.float64, np.complex64, np.complex128)


def rand_block(rng, m, n, dt):
    a = rng.standard_normal((m, n))
    if np.dtype(dt).kind == "c":
        a = a + 1j * rng.standard_normal((m, n))
    return np.asfortranarray(a.astype(dt))


def cuts(sizes):
    starts = np.concatenate([[1], 1 + np.cumsum(sizes)[:-1]])
    return [(int(s), int(k)) for s, k in zip(starts, sizes)]


# every constructor as (name, shapes of the blocks in constructor order, make(values) -> mirror object)
def constructors(bsm, rng, dt, tim):
    S = bsm
    out = []
    # a grid of contiguous blocks: tall (> 64 rows: several chunks), odd widths (16-byte units shared by two blocks)
    rp = cuts([70, 5, 33, 64, 9])
    cp = cuts([3, 70, 17, 64, 1])
    n = sum(k for _, k in rp)
    cells = [(i, j) for i in range(len(rp)) for j in range(len(cp)) if rng.random() < 0.7]
    order = rng.permutation(len(cells))
    cells = [cells[k] for k in order]  # given unsorted
    shapes = [(rp[i][1], cp[j][1]) for i, j in cells]
    rs = [rp[i][0] for i, _ in cells]
    cs = [cp[j][0] for _, j in cells]
    out.append(("vbcrs", shapes, lambda v: S.VariableBlockCompressedRowStorage(
        v, rs, cs, (n, n), device=NODEV, transpose_image=tim)))
    rl = [np.arange(rp[i][0], rp[i][0] + rp[i][1]) for i, _ in cells]
    cl = [np.arange(cp[j][0], cp[j][0] + cp[j][1]) for _, j in cells]
    out.append(("vbcrs_from_blocksparse", shapes, lambda v: S.VariableBlockCompressedRowStorage(
        S.BlockSparseMatrix(v, rl, cl, (n, n), device=NODEV), device=NODEV, transpose_image=tim)))
    # symmetric on the row partition: diagonals, then the upper off-diagonal blocks
    offc = [(i, j) for i in range(len(rp)) for j in range(i + 1, len(rp)) if rng.random() < 0.6]
    dshapes = [(k, k) for _, k in rp]
    oshapes = [(rp[i][1], rp[j][1]) for i, j in offc]
    nd = len(rp)

    def sym_lists(perm):
        dl = [perm[s - 1:s - 1 + k] for s, k in rp]
        return dl, [dl[i] for i, _ in offc], [dl[j] for _, j in offc]
    dl, orl, ocl = sym_lists(np.arange(1, n + 1))
    out.append(("vbcrs_from_symmetric", dshapes + oshapes, lambda v: S.VariableBlockCompressedRowStorage(
        S.SymmetricBlockMatrix(v[:nd], dl, v[nd:], orl, ocl, (n, n), device=NODEV), device=NODEV)))
    # scattered, unsorted index lists with blocks taller than 64 rows (permuted placement, multi-chunk blocks)
    ns = 900
    sh = [(70, 33), (5, 130), (64, 64), (130, 7), (3, 3), (66, 1)]
    srows = [rng.permutation(ns)[:m] + 1 for m, _ in sh]
    scols = [rng.permutation(ns)[:k] + 1 for _, k in sh]
    out.append(("blocksparse", sh, lambda v: S.BlockSparseMatrix(
        v, srows, scols, (ns, ns), device=NODEV, transpose_image=tim)))
    sdl, sorl, socl = sym_lists(rng.permutation(n) + 1)
    out.append(("symmetric", dshapes + oshapes, lambda v: S.SymmetricBlockMatrix(
        v[:nd], sdl, v[nd:], sorl, socl, (n, n), device=NODEV)))
    return out


def images(A, tim):
    imgs = {w: get_image(A, timage=False, multi=(w == 8)) for w in (0, 8)}
    out = {"values": imgs[0][0].tobytes(), "rows": imgs[0][1].tobytes(), "cols": imgs[0][2].tobytes(),
           "waves": imgs[0][3].tobytes(), "waves_multi": imgs[8][3].tobytes()}
    if tim:
        t = get_image(A, timage=True)
        out.update({"t_values": t[0].tobytes(), "t_rows": t[1].tobytes(), "t_cols": t[2].tobytes(),
                    "t_waves": t[3].tobytes()})
    return out


def has_t(A):
    from bsm_amd import _lib as L
    n = C.c_int64(0)
    return L.lib().bsm_get_image(A._h.ptr, 16, None, C.byref(n)) == 0


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
def test_full_and_subset_update_equal_a_fresh_handle(bsm, dt):
    rng = np.random.default_rng(20 + DTYPES.index(dt))
    for tim in (False, True):
        for name, shapes, make in constructors(bsm, rng, dt, tim):
            va = [rand_block(rng, m, k, dt) for m, k in shapes]
            vb = [rand_block(rng, m, k, dt) for m, k in shapes]
            A = make([a.copy(order="F") for a in va])
            before = images(A, has_t(A))
            if tim and name in ("vbcrs", "vbcrs_from_blocksparse", "blocksparse"):
                assert has_t(A), name
            # full update through the mirror
            bsm.update_blocks(A, vb)
            after = images(A, has_t(A))
            fresh = images(make(vb), has_t(A))
            for k in after:
                if k in ("values", "t_values"):
                    assert after[k] == fresh[k], (name, k)
                else:  # metadata is never touched
                    assert after[k] == before[k], (name, k)
            # subset update: random ids, random order, ld > m, through the C ABI
            nb = len(shapes)
            ids = rng.permutation(nb)[: max(1, nb // 3)] + 1
            newv, lds, mixed = [], [], list(vb)
            for i in ids:
                m, k = shapes[i - 1]
                big = rand_block(rng, m + 3, k, dt)  # ld = m + 3
                newv.append(big)
                lds.append(m + 3)
                mixed[i - 1] = np.asfortranarray(big[:m, :])
            assert update_rc(A, ids, newv, lds) == 0
            got = images(A, has_t(A))
            want = images(make(mixed), has_t(A))
            for k in ("values", "t_values"):
                if k in got:
                    assert got[k] == want[k], (name, "subset", k)


def test_errors_leave_the_handle_unchanged(bsm):
    from bsm_amd import _lib as L
    rng = np.random.default_rng(5)
    dt = np.float64
    name, shapes, make = constructors(bsm, rng, dt, True)[0]
    A = make([rand_block(rng, m, k, dt) for m, k in shapes])
    before = images(A, True)
    nb = len(shapes)
    good = [rand_block(rng, m, k, dt) for m, k in shapes]
    lds = [m for m, _ in shapes]
    I = C.POINTER(C.c_int64)
    cases = [
        lambda: L.lib().bsm_update_blocks(None, 1, None, None, None, 0, None),   # null handle
        lambda: update_rc(A, [1, nb + 1], good[:2], lds[:2]),                   # id out of range
        lambda: update_rc(A, [0], good[:1], lds[:1]),                           # ids are 1-based
        lambda: update_rc(A, [2, 1, 2], good[:3], lds[:3]),                     # duplicate id
        lambda: update_rc(A, None, good[:-1], lds[:-1]),                        # ids == NULL needs every block
        lambda: update_rc(A, [1, 2], good[:2], [lds[0], shapes[1][0] - 1]),    # ld < m
        lambda: update_rc(A, None, good, lds, memspace=7),                      # bad memspace
        lambda: update_rc(A, None, good, lds, memspace=1),                      # device blocks, no device
        lambda: L.lib().bsm_update_blocks(A._h.ptr, nb, None, None, np.ascontiguousarray(lds, dtype=np.int64).ctypes.data_as(I), 0, None),
        lambda: update_rc(A, [1], good[:1], lds[:1], nupd=-1),                  # negative count
    ]
    for k, call in enumerate(cases):
        assert call() == -1, k  # BSM_ERR_INVALID
        assert images(A, True) == before, k
    assert update_rc(A, [], [], []) == 0  # nothing to do is not an error
    assert images(A, True) == before


@pytest.mark.parametrize("dt", (np.float64, np.complex64), ids=lambda d: np.dtype(d).name)
def test_refresh_after_in_place_edit_equals_update_blocks(bsm, dt):
    rng = np.random.default_rng(9)
    for name, shapes, make in constructors(bsm, rng, dt, True):
        va = [rand_block(rng, m, k, dt) for m, k in shapes]
        A = make([a.copy(order="F") for a in va])
        Bm = make([a.copy(order="F") for a in va])
        i = int(rng.integers(len(shapes))) + 1
        new = rand_block(rng, *shapes[i - 1], dt)
        src = A._src()
        src[i - 1][...] = new  # copyto!(block(A, i), new) on the mirror's own field
        assert images(A, has_t(A))["values"] == images(Bm, has_t(Bm))["values"]  # not pushed yet
        bsm.refresh(A)
        bsm.update_blocks(Bm, [new], ids=[i])
        assert images(A, has_t(A)) == images(Bm, has_t(Bm)), name
        # the wrapped operators update their .lmap
        j = 1 + (i % len(shapes))
        new2 = rand_block(rng, *shapes[j - 1], dt)
        bsm.update_blocks(bsm.transpose(Bm), [new2], ids=[j])
        A._src()[j - 1][...] = new2
        bsm.refresh(bsm.adjoint(A), ids=[j])
        assert images(A, has_t(A)) == images(Bm, has_t(Bm)), name


def test_vbcrs_mirror_edit_of_sorted_blocks(bsm):
    """A.blocks of a VBCRS is the SORTED view of the constructor's list: an in-place edit of A.blocks[k] is an edit of
    constructor block perm[k], and refresh pushes it there."""
    rng = np.random.default_rng(3)
    name, shapes, make = constructors(bsm, rng, np.float64, False)[0]
    va = [rand_block(rng, m, k, np.float64) for m, k in shapes]
    A = make([a.copy(order="F") for a in va])
    k = len(shapes) // 2
    p = int(A.perm[k])
    A.blocks[k][...] = 7.0
    bsm.refresh(A)
    vb = list(va)
    vb[p - 1] = np.full(shapes[p - 1], 7.0, order="F")
    assert images(A, False)["values"] == images(make(vb), False)["values"]


def test_materialized_symmetric_vbcrs_refuses_updates(bsm):
    """a VBCRS that materialised a SymmetricBlockMatrix holds every off-diagonal block twice; one new value cannot
    reach both copies through the block list, so the mirror refuses instead of leaving the transposes stale"""
    rng = np.random.default_rng(8)
    d = [rand_block(rng, 3, 3, np.float64), rand_block(rng, 2, 2, np.float64)]
    o = [rand_block(rng, 3, 2, np.float64)]
    S = bsm.SymmetricBlockMatrix(d, [np.arange(1, 4), np.arange(4, 6)], o, [np.arange(1, 4)], [np.arange(4, 6)], (5, 5),
                                 device=NODEV)
    V = bsm.VariableBlockCompressedRowStorage(S, device=NODEV, materialize=True)
    with pytest.raises(NotImplementedError):
        bsm.refresh(V)
    with pytest.raises(NotImplementedError):
        bsm.update_blocks(V, [np.zeros((3, 2))], ids=[3])
