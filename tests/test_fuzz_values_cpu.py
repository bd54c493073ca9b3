"""CPU suite: the VALUES of layout-edge operators (tests/_fuzz.py) through the host side of the value-moving code.
Analysis-only handles refilled through bsm_update_blocks (the host replay of the refill plan the GPU's refill_kernel
walks) hold byte for byte the image of a fresh handle; the host mirror's rowcolvals(A) is the set of triples
_fuzz.coo_triples builds straight from the numpy blocks -- the reference test_gpu_fuzz_values.py holds the device
export to; and the twelve operators of every (type, element type) reach every layout edge the type can reach."""
import numpy as np
import pytest

from _common import NODEV
from _fuzz import canonical, coo_triples, edge_features
from _values import (NOPS, SPECIAL, assert_coverage, copied, explain, image_parts, new_values, options, raw_update, seeded,
                     src_list, subset_of, value_operators, value_seed, with_values)

KINDS = ["blocksparse", "vbcrs", "symmetric"]
DTYPES = [np.float32, np.float64, np.complex64, np.complex128]
VALUE_KEYS = ("values", "t_values")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_the_operators_reach_every_layout_edge(kind, dtype):
    ops = value_operators(kind, dtype)
    assert len(ops) == NOPS
    count = assert_coverage(kind, dtype, ops)
    print(f"VALSTAT coverage {kind} {np.dtype(dtype).name} operators {len(ops)} "
          + " ".join(f"{f} {c}" for f, c in count.items()))


def test_helpers_on_a_hand_made_operator():
    """coo_triples / canonical / edge_features on operators small enough to write their triples down"""
    b = np.asfortranarray(np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]]))
    p = dict(kind="vbcrs", blocks=[b, b[:1, :1].copy(order="F")], rowstart=np.array([2, 2]), colstart=np.array([3, 3]),
             size=(5, 6))
    r, c, v = coo_triples(p)
    assert sorted(zip(r.tolist(), c.tolist(), v.tolist())) == [(2, 3, 1.0), (2, 3, 1.0), (2, 4, 2.0), (2, 5, 3.0),
                                                                (3, 3, 4.0), (3, 4, 5.0), (3, 5, 6.0)]
    assert edge_features(p) == {"thin", "shared"}
    o = np.asfortranarray(np.array([[1 + 2j, 3 + 4j]]))
    d = np.asfortranarray(np.array([[7 + 0j]]))
    s = dict(kind="symmetric", diagonals=[d], diagonalindices=[np.array([4])], offdiagonals=[o], rowindices=[np.array([4])],
             colindices=[np.array([3, 1])], size=(4, 4))
    r, c, v = coo_triples(s)
    assert sorted(zip(r.tolist(), c.tolist(), v.tolist()), key=lambda t: t[:2]) == [
        (1, 4, 3 + 4j), (3, 4, 1 + 2j), (4, 1, 3 + 4j), (4, 3, 1 + 2j), (4, 4, 7 + 0j)]  # transposed, not conjugated
    assert edge_features(s) == {"thin", "shared", "scattered"}
    e = dict(kind="blocksparse", blocks=[np.zeros((0, 2), order="F"), np.zeros((70, 1), order="F")],
             rowindices=[np.zeros(0, np.int64), np.arange(1, 71)], colindices=[np.array([1, 2]), np.array([5])], size=(80, 9))
    assert edge_features(e) == {"empty", "tall", "thin"} and len(coo_triples(e)[0]) == 70
    # the order of the triples does not matter, the bits of a value do: -0.0 is not 0.0, a NaN equals itself
    rows, cols = np.array([2, 1, 1]), np.array([1, 3, 3])
    a = canonical(rows, cols, np.array([np.nan, -0.0, 5.0]))
    assert np.array_equal(a, canonical(rows[::-1], cols[::-1], np.array([5.0, -0.0, np.nan])))
    assert not np.array_equal(a, canonical(rows, cols, np.array([np.nan, 0.0, 5.0])))
    assert a[:, 0].tolist() == [(1 << 32) | 3, (1 << 32) | 3, (2 << 32) | 1] and a[0, 1] < a[1, 1]
    z = canonical(np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.complex64))
    assert z.shape == (0, 3)


def test_special_values_round_as_the_header_promises():
    """what the converting-pack leg of the GPU test seeds, on the host: nearest-even differs from truncation, subnormals
    stay, magnitudes beyond the range become inf (include/bsm_rocm.h, the mixed-precision codes)"""
    sp = np.array(SPECIAL)
    with np.errstate(over="ignore"):
        f = sp.astype(np.float32)
    trunc = (sp.view(np.uint64) & ~np.uint64((1 << 29) - 1)).view(np.float64)  # the double with its low 29 bits cut
    assert f[0] == 1 and f[1] == np.float32(1 + 2.0 ** -22) and f[2] == -np.float32(1 + 2.0 ** -23)
    assert all(np.float64(f[k]) != trunc[k] for k in (1, 2))
    assert all(0 < abs(f[k]) < np.finfo(np.float32).tiny for k in (3, 4, 5)) and f[6] == 0 and f[7] == np.float32(2.0 ** -148)
    assert f[8] == np.inf and f[9] == -np.inf and f[10] == np.inf and np.float32(np.nextafter(sp[10], 0)) < np.inf
    for kind in KINDS:  # every operator has a block that takes at least eight of them, the subnormal and the overflowing included
        for dt in (np.float64, np.complex128):
            for p in value_operators(kind, dt):
                q = seeded(p)
                big = max(src_list(q), key=lambda a: a.size).reshape(-1, order="F")
                k = min(len(sp), len(big))
                assert k > 8 and np.array_equal(big[:k].real, sp[:k])
                assert [b.shape for b in src_list(p)] == [b.shape for b in src_list(q)]
                if np.dtype(dt).kind == "c":
                    assert np.array_equal(big[:k].imag, sp[:k][::-1])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_analysis_only_refill_is_bytewise_a_fresh_handle(bsm, kind, dtype):
    """full update through the mirror, then a subset through the C ABI (a random third of the ids in random order,
    ld = m + 3): the values of both images are those of a handle built from the new values, the metadata is untouched"""
    rng = np.random.default_rng(value_seed(kind, dtype) + 1)
    seed = value_seed(kind, dtype)
    for case, p in enumerate(value_operators(kind, dtype)):
        kw = dict(options(kind, case), device=NODEV)
        A = bsm.synthetic.build(copied(p), **kw)
        before = image_parts(A)
        assert ("t_values" in before) == bool(kw.get("transpose_image")), (seed, case)
        vb = new_values(p, rng)
        bsm.update_blocks(A, vb)
        after = image_parts(A)
        fresh = image_parts(bsm.synthetic.build(with_values(p, vb), **kw))
        assert after.keys() == fresh.keys() == before.keys()
        for k in after:
            assert after[k] == (fresh[k] if k in VALUE_KEYS else before[k]), (seed, case, "full", k)
        ids, blocks, cur = subset_of(rng, p, vb)
        big, lds = [], []
        for b in blocks:
            a = np.asfortranarray(np.concatenate([b, np.full((3, b.shape[1]), np.nan, dtype=b.dtype)]))
            big.append(a)
            lds.append(b.shape[0] + 3)
        raw_update(A, ids, big, lds, 0)
        got = image_parts(A)
        want = image_parts(bsm.synthetic.build(with_values(p, cur), **kw))
        for k in got:
            assert got[k] == (want[k] if k in VALUE_KEYS else before[k]), (seed, case, "subset", k)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_host_mirror_triples_are_the_triples_of_the_blocks(bsm, kind, dtype):
    seed = value_seed(kind, dtype)
    total = 0
    for case, p in enumerate(value_operators(kind, dtype)):
        A = bsm.synthetic.build(p, device=NODEV, **options(kind, case))
        want = canonical(*coo_triples(p))
        got = canonical(*bsm.rowcolvals(A))
        assert len(want) == bsm.nnz(A), (seed, case, len(want), bsm.nnz(A))
        assert np.array_equal(got, want), explain(p, seed, case, got, want)
        assert sum(b.size for b in src_list(p)) <= len(want)
        total += len(want)
    print(f"VALSTAT mirror {kind} {np.dtype(dtype).name} operators {NOPS} triples {total}")
